"""The restatement tests/gumbeltreeref.py (completed-Q selection below the root of a Gumbel search) on the CPU: wsum leaves the same bits in
all 64 lanes; the rule's properties by hand; with the flag off it is gumbelref ply for ply; args["gumbel_tree"] as selfplay.gumbel_tree_of reads
it; the C ABI's declarations and exports; and the scenarios and hook cases tests/test_gpu_gumbel_tree.py runs on the device reach every
condition they are there for."""
import ctypes as C
import math
import os
import re
import warnings

import numpy as np
import pytest

import gumbelref as GB
import gumbeltreeref as GT
from gumbelref import Gumbel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_played = {}


def _play(sc):
    if sc.name not in _played:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[sc.name] = GT.play(sc)
    return _played[sc.name]


# ------------------------------------------------------------------------------------------------ wsum and the rule
def test_wsum_gives_identical_results_in_all_64_lanes():
    rng = np.random.default_rng(11)
    for K in (1, 2, 63, 64, 65, 128, 129, 218):
        for scale in (1.0, 1e-30, 1e30):
            t = (rng.standard_normal(K) * scale * 10.0 ** rng.integers(-8, 9, size=K)).tolist()
            lanes = GT.wsum_lanes(t)
            assert len(lanes) == 64 and len({GB._bits(v) for v in lanes}) == 1, (K, scale)
            assert GT.wsum(t) == lanes[0] and abs(lanes[0] - math.fsum(t)) <= 1e-12 * math.fsum(abs(x) for x in t)
    # not the sequential sum: an order in which the two differ
    t = [0.0] * 64
    t[0], t[1], t[33] = 1.0, 2.0 ** -53, 2.0 ** -53      # lanes 1 and 33 meet in the first stage: 2^-52 survives beside 1.0, 2^-53 alone does not
    seq = 0.0
    for x in t:
        seq = seq + x
    assert seq == 1.0 and GT.wsum(t) == 1.0 + 2.0 ** -52
    assert GT.wsum([0.25]) == 0.25 and GT.wsum([]) == 0.0


def test_rule_by_hand():
    ob = Gumbel(16, 50.0, 1.0)
    P = np.array([0.5, 0.25, 0.25], np.float32)
    # nothing visited: v_mix = v01, the scores are the softmax of the logits, the largest prior wins
    i, score, v_mix, info = GT.select_tree(np.zeros(3, np.int64), np.zeros(3), P, 0.5, ob)
    assert i == 0 and v_mix == 0.75 and info["sumN_0"] == 1 and np.allclose(score, [0.5, 0.25, 0.25], rtol=1e-12)
    # the first child has all the visits and a value equal to v_mix's: its share is used up, the next prior is chosen; equal priors tie by index
    i, score, v_mix, info = GT.select_tree(np.array([2, 0, 0]), np.array([-1.0, 0.0, 0.0]), P, 0.5, ob)
    assert v_mix == 0.75 and i == 1 and info["tree_tie_by_index"] == 1 and score[1] == score[2]
    assert np.allclose(score, [0.5 - 2.0 / 3.0, 0.25, 0.25], rtol=1e-12)
    # a child that looks won draws the visits until its count catches up with its share
    i, score, v_mix, _ = GT.select_tree(np.array([1, 1, 0]), np.array([1.0, -1.0, 0.0]), P, 0.0, ob)
    assert i == 1 and 0.0 < v_mix < 1.0
    # equal children: every score is the same and the first wins
    i, score, _, info = GT.select_tree(np.full(5, 2), np.full(5, -0.5), np.full(5, 0.2, np.float32), -1.0, ob)
    assert i == 0 and len(set(score)) == 1 and info["tree_tie_by_index"] == 1
    # c_scale 100: the worse child's e is exactly 0
    _, score, _, info = GT.select_tree(np.array([4, 4]), np.array([-3.0, 3.0]), P[:2], 0.0, Gumbel(16, 50.0, 100.0))
    assert info["e_exactly_0"] == 1 and score[1] == -4.0 / 9.0
    # one child: always chosen
    assert GT.select_tree(np.array([7]), np.array([7.0]), np.ones(1, np.float32), 1.0, ob)[0] == 0


# ------------------------------------------------------------------------------------------------ flag off
def test_is_gumbelref_with_the_flag_off():
    off = {}
    for sc in GT.scenarios():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            want = GB.play(next(s for s in GB.scenarios() if s.name == sc.name))
            got = off[sc.name] = GT.play(sc, tree=False)
        for bd, g, w in zip(sc.boards, got, want):
            assert g.chosen == w.chosen and g.error == w.error and g.tree_plies == [False] * len(g.searches) and g.tree_selections == 0, (sc.name, bd.name)
            assert len(g.searches) == len(w.searches)
            for ply, (a, s) in enumerate(zip(g.searches, w.searches)):
                assert type(a) is type(s) and type(a) is not GT.Search, (sc.name, bd.name, ply)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a.tree(), s.tree())), (sc.name, bd.name, ply)
                assert len(a.steps) == len(s.steps) and all(np.array_equal(x, y) for x, y in zip(a.steps, s.steps))
    # ... while the rule does build other trees from the same inputs
    sc = GT.scenarios()[0]
    same = lambda a, s: all(x.tobytes() == y.tobytes() for x, y in zip(a.tree(), s.tree()))
    assert any(not same(g.searches[0], w.searches[0]) for g, w in zip(_play(sc), off[sc.name]))


# ------------------------------------------------------------------------------------------------ args["gumbel_tree"]
def test_gumbel_tree_of_results_and_messages():
    from sigma_zero_amd.selfplay import gumbel_tree_of, gumbel_options_of, GUMBEL_KEYS
    assert gumbel_tree_of({}) is False and gumbel_tree_of({"gumbel_tree": False}) is False and gumbel_tree_of({"gumbel": {"m": 4}}) is False
    assert gumbel_tree_of({"gumbel": {}, "gumbel_tree": True}) is True and gumbel_tree_of({"gumbel": {"m": 4}, "gumbel_tree": np.bool_(True)}) is True
    assert gumbel_tree_of({"gumbel_tree": False, "fpu": {"mode": "absolute", "value": 0.0}}) is False
    for bad in (1, 0, None, "true", 1.0, {"on": True}):
        with pytest.raises(ValueError) as err:
            gumbel_tree_of({"gumbel": {"m": 4}, "gumbel_tree": bad})
        assert str(err.value) == "args['gumbel_tree'] must be True or False, got %r" % (bad,)
    for args in ({"gumbel_tree": True}, {"gumbel_tree": True, "gumbel": None}):
        before = repr(args)
        with pytest.raises(ValueError) as err:
            gumbel_tree_of(args)
        assert str(err.value) == "args['gumbel_tree'] needs args['gumbel']: the rule is a part of the Gumbel search" and repr(args) == before
    # a key of its own: the option dict and its reader are what they were
    assert GUMBEL_KEYS == ("m", "c_visit", "c_scale") and gumbel_options_of({"gumbel": {"m": 4}, "gumbel_tree": True}) == (4, 50.0, 1.0)
    with pytest.raises(ValueError):
        gumbel_options_of({"gumbel": {"m": 4, "tree": True}})


def test_abi_declarations_and_exports():
    from sigma_zero_amd import _native as N
    assert C.sizeof(N.sz_gumbel_options) == 12
    with open(os.path.join(ROOT, "include", "sigmazero.h")) as f:
        hdr = f.read()
    assert re.search(r"int sz_set_gumbel_tree\(sz_engine\* e, int32_t enable, void\* stream\);", hdr)
    assert re.search(r"int sz_gumbel_tree_stats\(sz_engine\* e, uint64_t out\[1\], void\* stream\);", hdr)
    assert re.search(r"int sz_debug_tree_values\(sz_engine\* e, int32_t board, int32_t max_nodes, float\* node_value, int32_t\* n_out, void\* stream\);", hdr)
    m = re.search(r"int sz_debug_gumbel_tree\(([^;]*)\);", hdr)
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 11 and params[9] == "int32_t n_cases" and all("*" in p for i, p in enumerate(params) if i != 9)
    assert [p.split("*")[-1].strip() for p in params[:9]] == ["offsets_dev", "vc_dev", "value_sum_dev", "prior_dev", "node_value_dev", "opts_dev", "score_out_dev",
                                                              "selected_out_dev", "v_mix_out_dev"]
    assert N.EXPORTS["sz_set_gumbel_tree"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p])
    assert N.EXPORTS["sz_gumbel_tree_stats"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p])
    assert N.EXPORTS["sz_debug_gumbel_tree"] == (C.c_int, [C.c_void_p] * 9 + [C.c_int32, C.c_void_p])
    assert N.EXPORTS["sz_debug_tree_values"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p])
    L = N.lib()
    for name in ("sz_set_gumbel_tree", "sz_gumbel_tree_stats", "sz_debug_gumbel_tree", "sz_debug_tree_values"):
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == N.EXPORTS[name][1]
    # the refusals that need no engine and no device
    out, n = (C.c_uint64 * 1)(), C.c_int32()
    assert L.sz_set_gumbel_tree(None, 1, None) == N.SZ_ERR_INVALID and L.sz_set_gumbel_tree(None, 0, None) == N.SZ_ERR_INVALID
    assert L.sz_gumbel_tree_stats(None, out, None) == N.SZ_ERR_INVALID
    assert L.sz_debug_tree_values(None, 0, 0, None, C.byref(n), None) == N.SZ_ERR_INVALID
    assert L.sz_debug_gumbel_tree(*([None] * 9), 1, None) == N.SZ_ERR_INVALID
    # the rule is in the header with every operator
    for text in ("v_l = v_l + v_(l xor off)", "(v01 + (double)sumN * (pq / pm)) / (1.0 + (double)sumN)", "(e_c / se) - ((double)N_c / (1.0 + (double)sumN))",
                 "slog((double)P_c) + sf * (N_c >= 1 ? q_c : v_mix)"):
        assert text in hdr, text


# ------------------------------------------------------------------------------------------------ scenarios and hook cases
def test_hook_cases_reach_every_condition():
    hc = GT.hook_cases()
    widths = np.diff(hc.offsets)
    assert len(hc.vhat) >= 500 and set(GT.HOOK_K) <= set(widths.tolist()) and widths.min() == 1 and widths.max() == GT.MAX_MOVES and hc.opts.dtype.itemsize == 12
    sel, score, vmix, cov = GT.hook_reference(hc)
    print("hook cases:", dict(cov))
    assert np.isfinite(score).all() and np.isfinite(vmix).all() and (vmix >= 0.0).all() and (vmix <= 1.0).all()
    assert all(0 <= sel[i] < widths[i] for i in range(len(sel))) and int(hc.N.max()) == 800 and (hc.P > 0).all()
    GT.assert_coverage(cov, GT.HOOK_COVERAGE)


def test_scenarios_reach_every_condition():
    scs = GT.scenarios()
    assert [sc.name for sc in scs] == ["m16_seeded", "m4_seeded_fpu", "m2_null", "m16_null_scale100", "m16_seeded_compact"]
    assert all(sc.S == 64 and sc.plies == 3 and len(sc.boards) == 8 and sc.tree for sc in scs) and {x for b in scs[0].boards for x in b.budgets} == {1, 2, 3, 9, 33, 64}
    assert any(sc.fpu is not None for sc in scs) and any(sc.compact for sc in scs)
    played = [_play(sc) for sc in scs]
    cov = GT.coverage(played)
    print("coverage of the whole searches alone:", {k: cov[k] for k in GT.COVERAGE})
    GT.assert_coverage(cov)
    assert cov["fallbacks"] == 0
    GT.assert_every_board_selects(scs, played)
    for sc, games in zip(scs, played):
        assert all(on for g in games for on in g.tree_plies), sc.name
        for g in games:
            for s in g.searches:                         # a value for exactly the expanded nodes, NaN elsewhere
                if type(s) is GT.Search and s.step_values:
                    tv = s.tree_values()
                    assert len(tv) == len(s.tree()[0]) and int((~np.isnan(tv)).sum()) == s.expansions and len(s.step_values) == len(s.step_trees)
    # the wide inner node: the grandchildren of the 218-move position, reached within 64 simulations
    wide = [g for sc, games in zip(scs, played) for bd, g in zip(sc.boards, games) if bd.name == "moves_218"]
    assert sum(g.cov["wide_inner"] for g in wide) >= 1
