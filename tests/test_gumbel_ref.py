"""The restatement tests/gumbelref.py (Gumbel root search, sequential halving, completed-Q policy target) on the CPU: the schedule against
a second, differently written statement; slog / sexp against libm within a measured bound; the improved policy's properties; with the option
off it is fpuref bit for bit; args["gumbel"] as selfplay.gumbel_options_of reads it; the C ABI's struct and exports; and the scenarios and
hook cases tests/test_gpu_gumbel.py runs on the device reach every condition they are there for, with no fall-back selection."""
import collections
import ctypes as C
import math
import os
import re
import warnings

import numpy as np
import pytest

import fpuref as FP
import gumbelref as GB
from gumbelref import Gumbel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the schedule
def level_walk(t, n, m_eff):
    """the device's closed walk over the phases (csrc/sz_gumbel.h sz_gumbel_level)"""
    L = 0
    while (1 << L) < m_eff:
        L += 1
    L = max(L, 1)
    c, t0, lv = m_eff, 0, 0
    while True:
        r = max(1, n // (L * c))
        if t < t0 + r * c:
            return lv + (t - t0) // c
        t0, lv, c = t0 + r * c, lv + r, max(2, c // 2)


def test_schedule_length_order_and_second_statement():
    for n in range(1, 131):
        for m in range(1, 33):
            seq = GB.schedule(n, m)[0]
            assert len(seq) == n and seq[0] == 0, (n, m)
            assert all(b - a in (0, 1) for a, b in zip(seq, seq[1:])), (n, m)                  # non-decreasing, no level skipped
            assert list(seq) == [level_walk(t, n, m) for t in range(n)], (n, m)
            assert all(GB.level(t, n, m) == seq[t] for t in (0, n // 2, n - 1))
    assert GB.schedule(7, 1)[0] == (0, 1, 2, 3, 4, 5, 6)                                        # m_eff = 1: every visit goes to that child
    # 16 considered, 63 visits: L = 4, c = 16 r = 1, c = 8 r = 1, c = 4 r = 3, c = 2 r = 7, then c = 2 again, cut after 13 visits
    assert GB.schedule(63, 16)[0] == (0,) * 16 + (1,) * 8 + (2,) * 4 + (3,) * 4 + (4,) * 4 + tuple(5 + i // 2 for i in range(14)) + tuple(12 + i // 2 for i in range(13))


@pytest.mark.parametrize("K", [1, 2, 3, 5, 16, 20, 218])
def test_schedule_always_finds_a_child_at_the_level(K):
    """a fresh root under the schedule: whatever the preference order, every visit finds a child at its level, and a child's visits are made at
    levels that never decrease (per child: level == its own count)"""
    rng = np.random.default_rng(K)
    for n in (1, 2, 3, 8, 15, 32, 63, 130):
        for m in (1, 2, 4, 16, 218):
            m_eff = min(m, K)
            pref = rng.permutation(K)
            N = np.zeros(K, np.int64)
            for t in range(n):
                lv = GB.level(t, n, m_eff)
                at = [c for c in pref if N[c] == lv]
                assert at, (K, n, m, t)
                N[at[0]] += 1
            assert N.sum() == n and (N > 0).sum() <= m_eff


# ------------------------------------------------------------------------------------------------ slog / sexp
def test_slog_sexp_accuracy_within_four_times_the_measured_error():
    x = np.concatenate([GB.powers_of_two_f32(), GB.random_priors(100000)])
    assert len(x) >= 100000 and (x > 0).all() and (x < 2.0 ** -126).sum() >= 64 and len(GB.powers_of_two_f32()) == 277
    worst_log = max(abs(GB.slog(v) - math.log(v)) / abs(math.log(v)) for v in x.tolist() if v != 1.0)
    assert GB.slog(1.0) == 0.0 and GB.slog(2.0) == GB.LN2 and GB.slog(0.5) == -GB.LN2
    y = GB.exp_grid()
    inside = [v for v in y.tolist() if v >= GB.EXP_CUTOFF]
    assert len(inside) >= 20000 and min(inside) == GB.EXP_CUTOFF and max(inside) == 0.0
    worst_exp = max(abs(GB.sexp(v) - math.exp(v)) / math.exp(v) for v in inside)
    assert GB.sexp(0.0) == 1.0 and GB.sexp(-0.0) == 1.0 and all(GB.sexp(v) == 0.0 for v in y.tolist() if v < GB.EXP_CUTOFF) and GB.sexp(float("nan")) == 0.0
    assert all(GB.sexp(v) >= 2.0 ** -1022 for v in inside)                                      # every result above the cutoff is a normal number
    print("largest relative error: slog %.3e, sexp %.3e; measured %.3e, bound %.3e" % (worst_log, worst_exp, GB.MEASURED_REL_ERR, GB.REL_ERR_BOUND))
    assert GB.REL_ERR_BOUND == 4 * GB.MEASURED_REL_ERR and GB.REL_ERR_BOUND < 2.0 ** -40       # a condition of the rule, not a measurement
    assert worst_log <= GB.REL_ERR_BOUND and worst_exp <= GB.REL_ERR_BOUND


def test_series_orders_leave_out_less_than_half_an_ulp():
    s_max = (GB.SQRT2 - 1.0) / (GB.SQRT2 + 1.0)
    assert s_max ** 20 / 21 < 2.0 ** -53 < s_max ** 18 / 19
    r_max = GB.LN2 / 2 + 1e-9
    assert r_max ** 14 / math.factorial(14) < 2.0 ** -53 < r_max ** 13 / math.factorial(13)


# ------------------------------------------------------------------------------------------------ the improved policy
def test_improved_policy_properties():
    rng = np.random.default_rng(3)
    ob = Gumbel(16, 50.0, 1.0)
    for K in (1, 2, 7, 64, 65, 218):
        P = rng.dirichlet(np.full(K, 0.3)).astype(np.float32) if K > 1 else np.ones(1, np.float32)
        P = np.maximum(P, np.float32(1e-30))
        N = rng.integers(0, 5, size=K)
        W = rng.uniform(-1, 1, size=K) * N
        pi, v_mix, _ = GB.improved_policy(N, W, P, 0.25, ob)
        assert pi.dtype == np.float32 and abs(float(pi.astype(np.float64).sum()) - 1.0) <= K * 2.0 ** -24 and 0.0 <= v_mix <= 1.0
        # no child visited: the softmax of the logits, the priors renormalised
        pi0, v0, _ = GB.improved_policy(np.zeros(K, np.int64), np.zeros(K), P, 0.25, ob)
        lg = [math.log(float(p)) for p in P]
        soft = np.array([math.exp(v - max(lg)) for v in lg])
        assert v0 == 0.5 + 0.5 * 0.25 and np.allclose(pi0, soft / soft.sum(), rtol=1e-6, atol=0.0)
    # a child whose q exceeds v_mix gains mass over its prior, one below loses it
    P = np.array([0.5, 0.3, 0.2], np.float32)
    N, W = np.array([4, 4, 0]), np.array([-3.0, 3.0, 0.0])          # q = 0.875, 0.125; W is from the child's side to move
    pi, v_mix, _ = GB.improved_policy(N, W, P, 0.0, ob)
    assert 0.125 < v_mix < 0.875 and pi[0] > P[0] and pi[1] < P[1]
    pi, _, info = GB.improved_policy(N, W, P, 0.0, Gumbel(16, 50.0, 100.0))
    assert info["e_exactly_0"] == 1 and pi[1] == 0.0 and pi[0] == 1.0


def test_selection_and_final_move_by_hand():
    ob = Gumbel(2, 50.0, 1.0)
    P = np.array([0.25, 0.5, 0.125, 0.125], np.float32)
    zero = np.zeros(4)
    # level 0 picks the top m by g + logit, first maximum on a tie
    assert GB.select_root(np.zeros(4, np.int64), zero, P, None, 0, 9, ob)[0] == 1
    assert GB.select_root(np.array([0, 1, 0, 0]), zero, P, None, 1, 9, ob)[0] == 0
    i, fb, info = GB.select_root(np.zeros(4, np.int64), zero, np.full(4, 0.25, np.float32), None, 0, 9, ob)
    assert (i, fb) == (0, False) and info["tie_by_index"] == 1
    g = np.array([0.0, 0.0, 5.0, 0.0])
    assert GB.select_root(np.zeros(4, np.int64), zero, P, g, 0, 9, ob)[0] == 2
    # visit 2 of 8 with m_eff = 2 is at level 1: only the two children with one visit match, the better q wins
    assert GB.level(2, 8, 2) == 1
    N, W = np.array([1, 1, 0, 0]), np.array([0.9, -0.9, 0.0, 0.0])
    assert GB.select_root(N, W, P, None, 2, 9, ob)[0] == 1
    assert GB.select_root(np.array([2, 2, 0, 0]), zero, P, None, 2, 9, ob)[1] is True            # no child at the level: the fall-back, counted
    assert GB.final_move(np.array([3, 3, 1, 0]), np.array([2.0, -2.0, 0.0, 0.0]), P, None, ob) == 1
    assert GB.final_move(np.array([3, 2, 1, 0]), np.array([2.0, -2.0, 0.0, 0.0]), P, None, ob) == 0


# ------------------------------------------------------------------------------------------------ option off
def test_is_fpuref_with_the_option_off():
    sc = FP.scenarios()[0]._replace(plies=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = FP.play(sc, 1, False, False)
        for bd, w in zip(sc.boards[:3], want):
            g = GB.Game(bd.make(), sc.S, None, reuse=False, L=1, lam=1.0, solver=False, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt, fpu=sc.fpu, gumbel=None)
            for ply in range(sc.plies):
                if g.live:
                    g.begin()
                    g.run()
                    g.play(bd.u(ply))
            assert g.chosen == w.chosen and g.gumbel_plies == [None] * len(g.searches) and g.gumbel_selections == 0
            for a, s in zip(g.searches, w.searches):
                assert type(a) is type(s) and type(a) is not GB.Search
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a.tree(), s.tree()))


# ------------------------------------------------------------------------------------------------ args["gumbel"]
def test_gumbel_options_of_results_and_messages():
    from sigma_zero_amd.selfplay import gumbel_options_of, search_options_of
    assert gumbel_options_of({}) is None and gumbel_options_of({"gumbel": None}) is None
    assert gumbel_options_of({"gumbel": {}}) == (16, 50.0, 1.0)
    assert gumbel_options_of({"gumbel": {"m": 4}}) == (4, 50.0, 1.0)
    assert gumbel_options_of({"gumbel": {"m": np.int64(218), "c_visit": 0, "c_scale": 0.1}}) == (218, 0.0, float(np.float32(0.1)))
    assert gumbel_options_of({"gumbel": {"c_scale": np.float32(2.5)}, "fpu": {"mode": "absolute", "value": 0.0}, "playout_cap": {"fast": 8, "p_full": 0.25}}) == (16, 50.0, 2.5)
    keys = "('m', 'c_visit', 'c_scale')"
    bad = [
        (16, "args['gumbel'] must be a dict with keys from %s, got 16" % keys),
        ({"m": 4, "n": 1}, "args['gumbel'] must be a dict with keys from %s, got " % keys),
        ({"m": 0}, "args['gumbel']['m'] must be an integer in 1..218, got 0"),
        ({"m": 219}, "args['gumbel']['m'] must be an integer in 1..218, got 219"),
        ({"m": 4.0}, "args['gumbel']['m'] must be an integer in 1..218, got 4.0"),
        ({"m": True}, "args['gumbel']['m'] must be an integer in 1..218, got True"),
        ({"c_visit": -1}, "args['gumbel']['c_visit'] must be a finite number >= 0, got -1"),
        ({"c_visit": float("nan")}, "args['gumbel']['c_visit'] must be a finite number >= 0, got nan"),
        ({"c_visit": "50"}, "args['gumbel']['c_visit'] must be a finite number >= 0, got '50'"),
        ({"c_scale": float("inf")}, "args['gumbel']['c_scale'] must be a finite number >= 0, got inf"),
        ({"c_scale": False}, "args['gumbel']['c_scale'] must be a finite number >= 0, got False"),
        # a fixed order: m before c_visit before c_scale
        ({"m": 0, "c_visit": -1, "c_scale": -1}, "args['gumbel']['m'] must be"),
        ({"c_visit": -1, "c_scale": -1}, "args['gumbel']['c_visit'] must be"),
    ]
    for opt, message in bad:
        with pytest.raises(ValueError) as err:
            gumbel_options_of({"gumbel": opt})
        assert str(err.value).startswith(message), (opt, str(err.value))
    for key, value in (("reuse_subtree", True), ("leaves_per_step", 4), ("solver", True), ("forced_playouts", 2.0),
                       ("endings", {"resign_value": -0.9, "resign_patience": 3}), ("root_dirichlet_alpha", 0.3)):
        args = {"gumbel": {"m": 4}, key: value}
        before = repr(args)
        with pytest.raises(ValueError) as err:
            gumbel_options_of(args)
        assert str(err.value) == "args['gumbel'] and args[%r] exclude each other" % key and repr(args) == before
    args = {"gumbel": {"m": 4, "c_visit": 1}, "leaves_per_step": 1, "solver": False, "reuse_subtree": False}
    before = repr(args)
    assert gumbel_options_of(args) == (4, 1.0, 1.0) and repr(args) == before                    # args left untouched
    assert search_options_of({"gumbel": {"m": 4}}) == (1, 1.0, False, False)


def test_abi_struct_and_exports():
    from sigma_zero_amd import _native as N
    assert C.sizeof(N.sz_gumbel_options) == 12 and [f[0] for f in N.sz_gumbel_options._fields_] == ["max_considered", "c_visit", "c_scale"]
    with open(os.path.join(ROOT, "include", "sigmazero.h")) as f:
        hdr = f.read()
    assert re.search(r"typedef struct sz_gumbel_options \{ int32_t max_considered; float c_visit; float c_scale; \} sz_gumbel_options;", hdr)
    assert re.search(r"int sz_set_gumbel\(sz_engine\* e, const sz_gumbel_options\* opt, const double\* g_dev, void\* stream\);", hdr)
    assert re.search(r"int sz_fetch_gumbel\(sz_engine\* e, float\* policy_target, double\* v_mix, float\* root_value, void\* stream\);", hdr)
    m = re.search(r"int sz_debug_gumbel\(([^;]*)\);", hdr)
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 21 and params[19] == "int32_t n_cases" and all("*" in p for i, p in enumerate(params) if i != 19)
    assert N.EXPORTS["sz_set_gumbel"] == (C.c_int, [C.c_void_p, C.POINTER(N.sz_gumbel_options), C.c_void_p, C.c_void_p])
    assert N.EXPORTS["sz_fetch_gumbel"] == (C.c_int, [C.c_void_p] * 5)
    assert N.EXPORTS["sz_debug_gumbel"] == (C.c_int, [C.c_void_p] * 19 + [C.c_int32, C.c_void_p])
    assert N.EXPORTS["sz_gumbel_stats"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p])
    L = N.lib()
    for name in ("sz_set_gumbel", "sz_fetch_gumbel", "sz_debug_gumbel", "sz_gumbel_stats"):
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == N.EXPORTS[name][1]
    # the refusals that need no engine and no device
    assert L.sz_set_gumbel(None, None, None, None) == N.SZ_ERR_INVALID
    assert L.sz_fetch_gumbel(None, None, None, None, None) == N.SZ_ERR_INVALID
    assert L.sz_debug_gumbel(*([None] * 19), 1, None) == N.SZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ scenarios and hook cases
def test_scenarios_and_hook_cases_reach_every_condition():
    hook = collections.Counter()
    hc = GB.hook_cases()
    widths = set(np.diff(hc.offsets).tolist())
    assert len(hc.visit) >= 500 and set(GB.HOOK_K) <= widths and max(widths) == GB.MAX_MOVES and hc.opts.dtype.itemsize == 12
    for with_g in (True, False):
        sel, fbk, fin, pol, vmix, cov = GB.hook_reference(hc, with_g)
        hook.update(cov)
        assert np.isfinite(pol).all() and np.isfinite(vmix).all() and 0 < fbk.sum() < len(fbk)
    GB.assert_coverage(hook, GB.HOOK_COVERAGE)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        played = [GB.play(sc) for sc in GB.scenarios()]
    cov = GB.coverage(played)
    print("coverage of the whole searches alone:", dict(cov))
    GB.assert_coverage(cov)
    assert {sc.gumbel.m for sc in GB.scenarios()} == {1, 2, 4, 16} and {sc.seeded for sc in GB.scenarios()} == {True, False}
    assert any(sc.fpu is not None for sc in GB.scenarios()) and any(sc.compact for sc in GB.scenarios())
    for sc, games in zip(GB.scenarios(), played):
        assert len(games) == 8 and sum(len(g.searches) for g in games) >= 16 and sum(g.gumbel_fallbacks for g in games) == 0, sc.name
        assert sum(g.error == "zero_visits" for g in games) >= 2, sc.name
