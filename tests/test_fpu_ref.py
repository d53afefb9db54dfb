"""The restatement tests/fpuref.py (first-play urgency for unvisited children) on the CPU: with the option off it is forcedref bit for bit on
forcedref's own scenarios; ABSOLUTE 0 at both sites builds the trees of the option switched off; selections worked by hand, the clamp at
both ends included; args["fpu"] as selfplay.fpu_options_of reads it; the C ABI's struct and exports; and the scenarios and hook cases
tests/test_gpu_fpu.py runs on the device reach every condition they are there for."""
import collections
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import forcedref as FR
import fpuref as FP
from fpuref import ABSOLUTE, REDUCTION, REFERENCE, Fpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trees_equal(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ option off, ABSOLUTE 0
@pytest.mark.parametrize("L,solver", FR.OPTIONS)
def test_is_forcedref_with_the_option_off(L, solver):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        n_searches = 0
        for sc in FR.scenarios():
            sc = sc._replace(plies=min(sc.plies, 3), boards=sc.boards[:3])
            want, gam = FR.play(sc, L, solver), FR.gammas(sc)
            for fpu in (None, Fpu(REFERENCE, 0.0, REFERENCE, 0.0)):
                for b, (bd, w) in enumerate(zip(sc.boards, want)):
                    g = FP.Game(bd.make(), sc.S, sc.edges_per_board, reuse=sc.reuse, L=L, lam=1.0, solver=solver, c=2.0, learning=sc.learning, mode=bd.mode,
                                salt=bd.salt, fpu=fpu)
                    for ply in range(sc.plies):
                        if g.live:
                            FR.begin_ply(sc, g, bd, b, ply, gam)
                            g.run()
                            g.play(bd.u(ply))
                    tag = "%s %s L=%d solver=%d" % (sc.name, bd.name, L, solver)
                    assert g.starts == w.starts and g.chosen == w.chosen and g.goals == w.goals and g.error == w.error, tag
                    assert all(getattr(g, k) == getattr(w, k) for k in FR.Game.COUNTERS), tag
                    assert (g.forced_selections, g.pruned_visits) == (w.forced_selections, w.pruned_visits) and g.fpu_plies == [None] * len(g.searches), tag
                    n_searches += len(g.searches)
                    for a, s in zip(g.searches, w.searches):
                        assert type(a) is type(s) and type(a) is not FP.Search, tag          # it IS forcedref's search, not a copy of it
                        assert _trees_equal(a.tree(), s.tree()) and _trees_equal(a.begin_tree, s.begin_tree), tag
                        assert len(a.steps) == len(s.steps) and all(np.array_equal(x, y) for x, y in zip(a.steps, s.steps)), tag
        assert n_searches >= 30


@pytest.mark.parametrize("L,solver,reuse", [(1, False, True), (4, True, True), (4, False, False)])
def test_absolute_0_builds_the_trees_of_the_option_switched_off(L, solver, reuse):
    """q0 = (0 + 1) / 2 = 0.5f is what get_ucb yields for an unvisited child; the restatement goes through select() all the same"""
    sc = FP.scenarios()[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        off = FP.play(sc, L, solver, reuse, fpu=None)
        on = FP.play(sc, L, solver, reuse, fpu=Fpu(ABSOLUTE, 0.0, ABSOLUTE, 0.0))
        other = FP.play(sc, L, solver, reuse)
    for a, b in zip(on, off):
        assert a.chosen == b.chosen and len(a.searches) == len(b.searches) >= 1
        assert all(type(s) is FP.Search for s in a.searches) and not any(type(s) is FP.Search for s in b.searches)
        for s, t in zip(a.searches, b.searches):
            assert _trees_equal(s.tree(), t.tree()) and _trees_equal(s.tree_proven(), t.tree_proven())
            assert len(s.steps) == len(t.steps) and all(np.array_equal(x, y) for x, y in zip(s.steps, t.steps))
        assert sum(v for k, v in a.cov.items() if k.startswith("changed_")) == 0
    assert sum(len(a.searches) for a in on) >= 2 * len(on)
    # ... and the scenario's own setting does build other trees
    assert any(not _trees_equal(s.tree(), t.tree()) for a, b in zip(other, off) for s, t in zip(a.searches[:1], b.searches[:1]))


# ------------------------------------------------------------------------------------------------ selections by hand
def test_selections_worked_by_hand():
    # a parent with n_p = 16 (sq = 4), c_puct = 2: u_c = 8 * P_c / (n_c + 1).  Stored edge N_p = 16, W_p = -4: vp = -0.25.
    # children: 0 visited (N 5, W -1: q = 1 - (-0.2 + 1) / 2 = 0.6, u = 8 * .5 / 6 = .667 -> 1.267), 1 visited (N 2, W 1: q = 0.25, u = 8 * .25 / 3
    # = .667 -> .917), 2 and 3 unvisited with P = .125 (u = 1) and P = .0625 (u = .5); mass = .5 + .25 = .75, sqrt = .8660
    N, K, W, P = [5, 2, 0, 0], [0, 0, 0, 0], [-1.0, 1.0, 0.0, 0.0], [0.5, 0.25, 0.125, 0.0625]
    sel = lambda fp, root=False, **kw: FP.select(kw.get("N", N), kw.get("K", K), W, P, kw.get("R"), 16, 16, kw.get("W_p", -4.0), 2.0, 1.0, root, fp)
    near = lambda s, want: np.allclose(s, want, atol=2e-3)
    # reference: unvisited q = 0.5: scores 1.267, .917, 1.5, 1.0 -> child 2
    i, s, _ = sel(Fpu(REFERENCE, 0.0, REFERENCE, 0.0))
    assert i == 2 and near(s, [1.267, 0.917, 1.5, 1.0])
    # absolute -1 in the tree: q0 = 0: 1.0 and 0.5 -> child 0, which FPU changed; at the root the setting is REFERENCE: child 2 again
    fp = Fpu(ABSOLUTE, -1.0, REFERENCE, 0.0)
    i, s, info = sel(fp)
    assert i == 0 and near(s, [1.267, 0.917, 1.0, 0.5]) and info["changed_absolute_tree"] == 1
    assert sel(fp, root=True)[0] == 2
    # reduction 0.5: v0 = -0.25 - 0.5 * .866 = -.683, q0 = .1585: 1.1585 and .6585 -> child 0
    i, s, info = sel(Fpu(REDUCTION, 0.5, REFERENCE, 0.0))
    assert i == 0 and near(s, [1.267, 0.917, 1.1585, 0.6585]) and info["changed_reduction_tree"] == 1 and info["clamp_low"] == 0
    # reduction 2 at the root: v0 = -0.25 - 1.732 = -1.98 -> clamped to -1, q0 = 0: as absolute -1
    i, s, info = sel(Fpu(REFERENCE, 0.0, REDUCTION, 2.0), root=True)
    assert i == 0 and near(s, [1.267, 0.917, 1.0, 0.5]) and info["clamp_low"] == 1 and info["changed_reduction_root"] == 1
    # vp = 1.5 (no search stores one, the rule clamps it all the same): v0 = 1.5 - 0.25 * .866 = 1.28 -> +1, q0 = 1: 2.0 and 1.5 -> child 2
    i, s, info = sel(Fpu(REDUCTION, 0.25, REFERENCE, 0.0), W_p=24.0)
    assert i == 2 and near(s, [1.267, 0.917, 2.0, 1.5]) and info["clamp_high"] == 1
    # a child with N = 0 and one descent in flight is visited: it is scored by get_ucb on n = 1, W = lam (q = 0, u = 8 * .125 / 2 = .5) and adds
    # its prior to the mass: sqrt(.875) = .9354, v0 = -0.25 - 0.5 * .9354 = -.7177, q0 = .1411 for child 3
    i, s, info = sel(Fpu(REDUCTION, 0.5, REFERENCE, 0.0), K=[0, 0, 1, 0])
    assert i == 0 and near(s, [1.267, 0.917, 0.5, 0.6411]) and info["inflight_only_visited"] == 1
    # the solver skips a WIN child whatever FPU gives the others; with every child WIN nothing is skipped
    i, s, info = sel(Fpu(ABSOLUTE, 1.0, REFERENCE, 0.0), R=np.array([0, 0, 1, 0], np.int8))
    assert i == 3 and near(s, [1.267, 0.917, 2.0, 1.5]) and info["win_skipped"] == 1
    assert sel(Fpu(ABSOLUTE, 1.0, REFERENCE, 0.0), R=np.ones(4, np.int8))[0] == 2
    # equal scores: the first maximum
    i, s, info = FP.select([0, 0, 0], [0, 0, 0], [0.0] * 3, [0.25, 0.5, 0.5], None, 4, 4, 0.0, 2.0, 1.0, True, Fpu(REFERENCE, 0.0, ABSOLUTE, 0.5))
    assert i == 1 and s[1] == s[2] and info["tie_first_maximum"] == 1


def test_the_mass_is_summed_lane_strided():
    """above 64 children a lane adds several priors before the butterfly: the sum differs from a sequential one in the last bits for some
    inputs, and the restatement must take the kernel's order"""
    rng = np.random.default_rng(3)
    differs = 0
    for _ in range(50):
        P = rng.dirichlet(np.full(218, 0.3)).astype(np.float32)
        visited = rng.random(218) < 0.5
        m = FP.visited_mass(P, visited)
        seq = np.float32(0.0)
        for c in range(218):
            if visited[c]:
                seq = seq + P[c]
        assert abs(float(m) - float(P[visited].astype(np.float64).sum())) < 1e-5
        differs += m != seq
    assert differs > 0
    P = np.array([0.5, 0.25, 0.125], np.float32)
    assert FP.visited_mass(P, [True, False, True]) == np.float32(0.625) and FP.visited_mass(P, [False] * 3) == 0.0


# ------------------------------------------------------------------------------------------------ args["fpu"]
def test_fpu_options_of_results_and_messages():
    from sigma_zero_amd.selfplay import fpu_options_of
    from sigma_zero_amd import _native as N
    assert fpu_options_of({}) is None and fpu_options_of({"fpu": None}) is None
    assert fpu_options_of({"fpu": {"mode": "reduction", "value": 0.33}}) == (N.SZ_FPU_REDUCTION, float(np.float32(0.33)), N.SZ_FPU_REDUCTION, float(np.float32(0.33)))
    assert fpu_options_of({"fpu": {"mode": "reduction", "value": 0.33, "root_mode": "absolute", "root_value": 1}}) == (2, float(np.float32(0.33)), 1, 1.0)
    assert fpu_options_of({"fpu": {"mode": "absolute", "value": -1, "root_mode": "reference"}}) == (1, -1.0, 0, 0.0)
    assert fpu_options_of({"fpu": {"mode": "reference", "root_mode": "reduction", "root_value": np.float32(2.0)}}) == (0, 0.0, 2, 2.0)
    assert fpu_options_of({"fpu": {"mode": "reference"}}) == (0, 0.0, 0, 0.0)
    assert fpu_options_of({"fpu": {"mode": "absolute", "value": 0.5, "root_value": -0.5}}) == (1, 0.5, 1, -0.5)
    bad = [
        ("reduction", "args['fpu'] must be a dict with keys from ('mode', 'value', 'root_mode', 'root_value'), got 'reduction'"),
        ({"mode": "absolute", "value": 0.0, "tree": 1}, "args['fpu'] must be a dict with keys from ('mode', 'value', 'root_mode', 'root_value'), got "),
        ({"value": 0.5}, "args['fpu'] needs 'mode'"),
        ({"mode": "lc0", "value": 0.5}, "args['fpu']['mode'] must be one of 'reference', 'absolute', 'reduction', got 'lc0'"),
        ({"mode": 1, "value": 0.5}, "args['fpu']['mode'] must be one of 'reference', 'absolute', 'reduction', got 1"),
        ({"mode": "absolute"}, "args['fpu']['mode'] = 'absolute' needs 'value'"),
        ({"mode": "absolute", "value": True}, "args['fpu']['value'] must be a number in [-1, 1] with 'absolute', got True"),
        ({"mode": "absolute", "value": float("nan")}, "args['fpu']['value'] must be a number in [-1, 1] with 'absolute', got nan"),
        ({"mode": "absolute", "value": 1.5}, "args['fpu']['value'] must be a number in [-1, 1] with 'absolute', got 1.5"),
        ({"mode": "reduction", "value": -0.1}, "args['fpu']['value'] must be a number in [0, 2] with 'reduction', got -0.1"),
        ({"mode": "reduction", "value": 2.5}, "args['fpu']['value'] must be a number in [0, 2] with 'reduction', got 2.5"),
        ({"mode": "reduction", "value": float("inf")}, "args['fpu']['value'] must be a number in [0, 2] with 'reduction', got inf"),
        ({"mode": "reduction", "value": "0.3"}, "args['fpu']['value'] must be a number in [0, 2] with 'reduction', got '0.3'"),
        ({"mode": "reference", "root_mode": "fast"}, "args['fpu']['root_mode'] must be one of 'reference', 'absolute', 'reduction', got 'fast'"),
        ({"mode": "reference", "root_mode": "absolute"}, "args['fpu']['root_mode'] = 'absolute' needs 'root_value'"),
        ({"mode": "reduction", "value": 1.5, "root_mode": "absolute"}, "args['fpu']['root_value'] must be a number in [-1, 1] with 'absolute', got 1.5"),
        ({"mode": "absolute", "value": 0.0, "root_value": False}, "args['fpu']['root_value'] must be a number in [-1, 1] with 'absolute', got False"),
        # a fixed order: the tree's site is checked before the root's
        ({"mode": "absolute", "value": 7, "root_mode": "nope"}, "args['fpu']['value'] must be a number in [-1, 1] with 'absolute', got 7"),
    ]
    for opt, message in bad:
        with pytest.raises(ValueError) as err:
            fpu_options_of({"fpu": opt})
        assert str(err.value).startswith(message), (opt, str(err.value))
    # search_options_of and its 4-tuple are what they were
    from sigma_zero_amd.selfplay import search_options_of
    assert search_options_of({"fpu": {"mode": "absolute", "value": 0.0}}) == (1, 1.0, False, False)


def test_abi_struct_and_exports():
    from sigma_zero_amd import _native as N
    assert C.sizeof(N.sz_fpu_options) == 16 and [f[0] for f in N.sz_fpu_options._fields_] == ["tree_mode", "tree_value", "root_mode", "root_value"]
    assert (N.SZ_FPU_REFERENCE, N.SZ_FPU_ABSOLUTE, N.SZ_FPU_REDUCTION) == (REFERENCE, ABSOLUTE, REDUCTION) == (0, 1, 2)
    with open(os.path.join(ROOT, "include", "sigmazero.h")) as f:
        hdr = f.read()
    assert re.search(r"enum \{ SZ_FPU_REFERENCE = 0, SZ_FPU_ABSOLUTE = 1, SZ_FPU_REDUCTION = 2 \};", hdr)
    assert re.search(r"int sz_set_fpu\(sz_engine\* e, const sz_fpu_options\* opt, void\* stream\);", hdr)
    m = re.search(r"int sz_debug_select_fpu\(([^;]*)\);", hdr)
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 17 and params[12] == "float virtual_loss" and params[15] == "int32_t n_cases" and all("*" in p for i, p in enumerate(params) if i not in (12, 15))
    assert N.EXPORTS["sz_set_fpu"] == (C.c_int, [C.c_void_p, C.POINTER(N.sz_fpu_options), C.c_void_p])
    assert N.EXPORTS["sz_debug_select_fpu"] == (C.c_int, [C.c_void_p] * 12 + [C.c_float] + [C.c_void_p] * 2 + [C.c_int32, C.c_void_p])
    L = N.lib()
    for name in ("sz_set_fpu", "sz_debug_select_fpu"):
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == N.EXPORTS[name][1]
    # the refusals that need no engine and no device
    assert L.sz_set_fpu(None, None, None) == N.SZ_ERR_INVALID
    assert L.sz_debug_select_fpu(*([None] * 12), C.c_float(1.0), None, None, 1, None) == N.SZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ scenarios and hook cases
_played = {}


def _play(sc, L, solver, reuse):
    key = (sc.name, L, solver, reuse)
    if key not in _played:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[key] = FP.play(sc, L, solver, reuse)
    return _played[key]


def test_changing_the_option_keeps_the_kept_subtree():
    sc = FP.scenarios()[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        g = FP.new_game(sc, sc.boards[2], 1, False, True)
        settings = [sc.fpu, FP.CONFIGS["ref_root_absm1_tree"], None]
        for ply in range(3):
            g.fpu = settings[ply]
            g.begin()
            g.run()
            g.play(-1.0)
    assert g.starts == ["new", "reused", "reused"] and g.fpu_plies == [FP.checked(sc.fpu), FP.checked(settings[1]), None]
    assert g.searches[1].n_kept > 1 and type(g.searches[2]) is not FP.Search


def test_scenarios_and_hook_cases_reach_every_condition():
    hook, widths = collections.Counter(), set()
    for solver in (False, True):
        hc = FP.hook_cases(solver=solver)
        scores, sel, cov = FP.hook_reference(hc)
        hook.update(cov)
        widths |= set(np.diff(hc.offsets).tolist())
        assert len(hc.parent) >= 3000 and np.isfinite(scores).all() and hc.opts.dtype.itemsize == 16
        nc = hc.N + hc.K
        assert ((hc.N == 0) & (hc.K > 0)).any() and (nc == 0).any()
    assert set(FP.HOOK_K) <= widths and max(widths) == FP.MAX_MOVES
    FP.assert_coverage(hook, FP.HOOK_COVERAGE)
    assert all(hook["site_%s_%s" % (site, mode)] > 0 for site in ("root", "tree") for mode in FP.MODE_NAMES.values())
    played = [_play(*run) for run in FP.runs()]
    cov = FP.coverage(played)
    print("coverage of the whole searches alone:", dict(cov))
    FP.assert_coverage(cov)
    for sc, L, solver, reuse in FP.runs():
        games = _play(sc, L, solver, reuse)
        assert all(g.error is None and len(g.searches) >= 1 for g in games)
        assert sum(len(g.searches) for g in games) >= 2 * len(games)
        if reuse:
            assert any(s == "reused" for g in games for s in g.starts), (sc.name, L, solver)
    # each configuration changes selections on its own, with and without leaf batching / the solver / reuse
    for sc, L, solver, reuse in FP.runs():
        c = FP.coverage([_play(sc, L, solver, reuse)])
        assert sum(v for k, v in c.items() if k.startswith("changed_")) > 0, (sc.name, L, solver, reuse)
        assert (c["inflight_only_visited"] > 0) == (L > 1), (sc.name, L, solver, reuse)
