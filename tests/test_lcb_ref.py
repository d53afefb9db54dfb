"""The restatement of the value spread and of lower-confidence-bound move selection (tests/lcbref.py) on the CPU: ssqrt against math.sqrt and lcb
against the exact form within four times the deviation measured here, the properties of the rule (the clamp, zero spread, stdevs = 0,
min_visit_prop = 1, select = 0), the second moment against a direct sum over the backed-up values, bit for bit the host compilation of
csrc/sz_lcb.h, the conditions the hook cases and the engine configurations are there for, and the Python argument layer
(selfplay.lcb_options_of).  tests/test_gpu_lcb.py holds the device to the restatement."""
import math
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import lcbref as LR
from sigma_zero_amd.selfplay import lcb_options_of

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sigma-zero_amd", "csrc")
_played = {}


def _play(name, lcb="config"):
    if (name, lcb) not in _played:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[(name, lcb)] = LR.play(next(c for c in LR.configs() if c.name == name), lcb)
    return _played[(name, lcb)]


@pytest.fixture(scope="module")
def cases():
    hc = LR.hook_cases()
    return hc, LR.hook_reference(hc)


# ------------------------------------------------------------------------------------------------ 1. accuracy
def test_ssqrt_is_within_four_times_the_measured_deviation_of_math_sqrt(cases):
    rng = np.random.default_rng(5)
    xs = list(2.0 ** rng.uniform(-200.0, 200.0, size=200000))
    hc = cases[0]
    for i in range(len(hc.opts)):                          # the arguments the rule itself forms on the hook cases
        n, N, W, Q, o = LR.hook_case(hc, i)
        xs += [LR.spread(Q[c], N[c], LR.mean(W[c], N[c])) / float(int(N[c]) - 1) for c in range(len(N)) if N[c] >= 2]
    worst = 0.0
    for x in xs:
        y, bad = LR.ssqrt(x)
        assert bad == 0
        if x == 0.0:
            assert y == 0.0
            continue
        worst = max(worst, abs(y - math.sqrt(x)) / math.sqrt(x))
    print("ssqrt: worst relative deviation from math.sqrt %.3g over %d arguments (recorded %.3g)" % (worst, len(xs), LR.MEASURED_SSQRT_DEV))
    assert worst <= LR.SSQRT_BOUND
    assert worst >= LR.MEASURED_SSQRT_DEV / 4, "the recorded figure is the measured one"
    for k in range(1, 2000):                               # exact squares come out exact
        assert LR.ssqrt(float(k * k)) == (float(k), 0)
    assert LR.ssqrt(0.0) == (0.0, 0) and LR.ssqrt(-0.0) == (0.0, 0)
    for x in (-1.0, 5e-324, 1e-310, math.inf, -math.inf, math.nan):
        assert LR.ssqrt(x) == (0.0, 1), "treated as 0.0 and counted"
    assert LR.ssqrt(2.2250738585072014e-308)[1] == 0 and LR.ssqrt(1.7976931348623157e308)[1] == 0


def test_lcb_is_within_four_times_the_measured_deviation_of_the_exact_form(cases):
    hc, (move, cstar, ncand, bad, lcb, cov) = cases
    worst, n_vals = 0.0, 0
    for i in range(len(hc.opts)):
        n, N, W, Q, o = LR.hook_case(hc, i)
        lo = int(hc.offsets[i])
        for c in range(len(N)):
            if N[c] < 2:
                assert math.isnan(lcb[lo + c])
                continue
            ex = LR.exact_lcb(N[c], W[c], Q[c], o.stdevs)
            worst = max(worst, abs(lcb[lo + c] - ex) / max(1.0, abs(ex)))
            n_vals += 1
    print("lcb: worst deviation from the exact form %.3g of max(1, |exact|) over %d children (recorded %.3g)" % (worst, n_vals, LR.MEASURED_LCB_DEV))
    assert n_vals > 20000 and worst <= LR.LCB_BOUND
    assert worst >= LR.MEASURED_LCB_DEV / 4, "the recorded figure is the measured one"
    assert int(bad.sum()) == 0, "no ssqrt argument outside 0.0 and the positive normal numbers"


# ------------------------------------------------------------------------------------------------ 2. properties of the rule
def test_spread_is_never_negative_and_zero_for_equal_values():
    rng = np.random.default_rng(9)
    for _ in range(3000):
        N = int(rng.integers(2, 400))
        if rng.random() < 0.5:
            vals = np.clip(rng.uniform(-1, 1) + rng.normal(0.0, 10.0 ** rng.uniform(-8, -0.5), size=N), -1, 1).astype(np.float32).astype(np.float64)
        else:
            vals = np.full(N, np.float64(np.float32(rng.uniform(-1, 1))))       # equal values with a full f32 significand: Q / N - m * m can round below 0
        w, q = LR.moments(vals)
        m = LR.mean(w, N)
        raw = q / float(N) - m * m
        assert raw >= -(N + 4) * 2.0 ** -53 * max(q / float(N), m * m, 2.0 ** -1000), "beyond what the roundings of the two sums and the two quotients allow"
        s = LR.spread(q, N, m)
        assert s >= 0.0 and (s == raw or (s == 0.0 and not raw > 0.0))
        v, bad = LR.lcb_value(N, w, q, 5.0)
        assert bad == 0 and v <= m
    assert LR.spread(math.nan, 3, 0.5) == 0.0, "a NaN is clamped too"
    for x in LR.SHORT:                                     # equal values with short significands: the spread is exactly 0.0 and lcb == m
        for N in (2, 3, 7, 24, 800, 10 ** 5):
            w, q = LR.moments([x] * N)
            m = LR.mean(w, N)
            assert m == -x and LR.spread(q, N, m) == 0.0
            assert LR.lcb_value(N, w, q, 5.0) == (m, 0)
    assert math.isnan(LR.lcb_value(1, 0.5, 0.25, 5.0)[0]) and math.isnan(LR.lcb_value(0, 0.0, 0.0, 5.0)[0])


def test_stdevs_zero_picks_the_best_mean_and_prop_one_leaves_the_ties_with_cstar(cases):
    hc = cases[0]
    n_z0 = n_p1 = n_p0 = 0
    for i in range(len(hc.opts)):
        n, N, W, Q, o = LR.hook_case(hc, i)
        cs = LR.first_max(n)
        fd = LR.choose(n, N, W, Q, LR.options(0.0, o.min_visit_prop))
        cands = [c for c in range(len(n)) if LR.candidate(N[c], n[c], n[cs], o.min_visit_prop)]
        assert fd.cstar == cs and fd.n_candidates == len(cands)
        if cands:
            means = [LR.mean(W[c], N[c]) for c in cands]
            assert fd.move == cands[int(np.argmax(means))] and fd.lcb[fd.move] == max(means), "stdevs = 0: the first best mean among the candidates"
            n_z0 += 1
        else:
            assert fd.move == cs
        one = LR.choose(n, N, W, Q, LR.options(o.stdevs, 1.0))
        tied = [c for c in range(len(n)) if N[c] >= 2 and n[c] >= 1 and n[c] == n[cs]]
        assert one.n_candidates == len(tied) and (one.move in tied if tied else one.move == cs), "min_visit_prop = 1: only children tied with c*"
        n_p1 += len(tied) >= 2
        zero = LR.choose(n, N, W, Q, LR.options(o.stdevs, 0.0))
        assert zero.n_candidates == sum(1 for c in range(len(n)) if N[c] >= 2 and n[c] >= 1)
        n_p0 += zero.n_candidates > fd.n_candidates
        # the first maximum: every candidate before the move is strictly worse, none is better
        full = LR.choose(n, N, W, Q, o)
        cands = [c for c in range(len(n)) if LR.candidate(N[c], n[c], n[cs], o.min_visit_prop)]
        if cands:
            assert all(full.lcb[c] < full.lcb[full.move] for c in cands if c < full.move) and all(full.lcb[c] <= full.lcb[full.move] for c in cands)
    assert n_z0 > 1000 and n_p1 > 20 and n_p0 > 100


def test_hook_cases_reach_their_conditions(cases):
    hc, (move, cstar, ncand, bad, lcb, cov) = cases
    print({k: cov[k] for k in LR.HOOK_COVERAGE})
    LR.assert_coverage(cov, LR.HOOK_COVERAGE)
    ks = np.diff(hc.offsets)
    assert set(ks.tolist()) == set(LR.HOOK_K) == {1, 2, 63, 64, 65, 127, 128, 129, 218}
    zs, ps = {float(x) for x in hc.opts["stdevs"]}, {float(np.float32(x)) for x in hc.opts["min_visit_prop"]}
    assert zs == {0.0, 1.0, 5.0} and ps == {float(np.float32(x)) for x in LR.HOOK_P}
    assert len(set(lcb[~np.isnan(lcb)].tolist())) > 10000, "the cases are not a handful of values"


# ------------------------------------------------------------------------------------------------ 3. the engine configurations
@pytest.mark.parametrize("name", [c.name for c in LR.configs()])
def test_configuration_reaches_its_conditions_and_keeps_the_second_moment(name):
    cfg = next(c for c in LR.configs() if c.name == name)
    games, recs, lasts = _play(name)
    cov = LR.coverage(games)
    print(name, {k: cov[k] for k in LR.CONFIG_COVERAGE + LR.ENGINE_COVERAGE})
    LR.assert_coverage(cov, LR.CONFIG_COVERAGE)
    assert sum(g.lcb_stats[2] for g in games) == 0, "no ssqrt argument outside 0.0 and the positive normal numbers in an engine run"
    n_edges = 0
    for g in games:
        for s in g.searches:                               # Q against W and N: |W| <= Q <= N for values in [-1, 1], and Q * N >= W * W (Cauchy-Schwarz)
            ne = int(s.n_edges)
            W, N, Q = s.W[:ne], s.N[:ne].astype(np.float64), s.Q[:ne]
            N = N - (np.arange(ne) == 0)                  # the root's own count starts at 1
            assert (Q >= 0).all() and (Q <= N + 1e-9).all() and (Q * N >= W * W - 1e-9 * np.maximum(1.0, N * N)).all()
            assert (Q[N == 0] == 0.0).all(), "an edge without a backup keeps the zero it was created with"
            n_edges += ne
    assert n_edges > 10000
    for ply, (row, lrow) in enumerate(zip(recs, lasts)):   # the move played is the rule's where it decided
        for b, (rec, last) in enumerate(zip(row, lrow)):
            if rec is not None and last.decided:
                assert int(rec["chosen"]) == int(rec["action"][last.move])
            if rec is not None and rec["chosen"] < 0:
                assert last == LR.NO_LCB or math.isnan(last.lcb_move), "an ending that fires makes no choice"


def test_configurations_together_reach_the_engine_conditions():
    cov = LR.coverage([g for c in LR.configs() for g in _play(c.name)[0]])
    print({k: cov[k] for k in LR.ENGINE_COVERAGE})
    LR.assert_coverage(cov, LR.ENGINE_COVERAGE)


def test_select_zero_plays_as_without_the_option():
    name = LR.configs()[1].name
    cfg = next(c for c in LR.configs() if c.name == name)
    observe = _play(name, LR.options(5.0, 0.15, False))
    off = _play(name, None)
    for a, b in zip(observe[0], off[0]):
        assert a.chosen == b.chosen, "select = 0: c* or the sample, always"
        assert a.lcb_stats[0] == 0 and b.lcb_stats == [0, 0, 0]
    assert sum(g.lcb_stats[1] for g in observe[0]) > 0, "the rule's move differed from c* somewhere, and was not played"
    assert all(l == LR.NO_LCB for row in off[2] for l in row)
    on = _play(name)
    assert any(a.chosen != b.chosen for a, b in zip(on[0], off[0])), "with select the games differ"
    assert len(cfg.boards) == 8


def test_terminal_root_is_counted_out():
    import sigma_zero_amd as sz
    mated = sz.ChessTensor(fen="R5k1/5ppp/8/8/8/8/8/4K3 b - - 0 1")      # back-rank mate: the side to move has lost
    stale = sz.ChessTensor(fen="k7/8/1Q6/8/8/8/8/7K b - - 0 1")          # stalemate
    for game, tv in ((mated, -1.0), (stale, 0.0)):
        assert game.get_value_and_terminated() == (tv, True) or tuple(game.get_value_and_terminated()) == (tv, True)
        g = LR.Game(game, 24, None, reuse=False, L=1, lam=1.0, solver=False, c=2.0, learning=False, mode="dyadic", salt=1, lcb=LR.options())
        g.begin()
        s = g.run()
        assert int(s.N[0]) == 25 and float(s.W[0]) == tv * 24 and float(s.Q[0]) == (tv * tv) * 24.0
        assert s.tree_spread().tolist() == [(tv * tv) * 24.0]


# ------------------------------------------------------------------------------------------------ 4. the header's host build
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "sz_lcb.h"
typedef struct { float stdevs; float min_visit_prop; int select; } opt_t;
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int n = 0, cells = 0, nx = 0;
    if (fread(&n, 4, 1, f) != 1 || fread(&cells, 4, 1, f) != 1 || fread(&nx, 4, 1, f) != 1) return 4;
    int* off = (int*)malloc(4 * (size_t)(n + 1)); int* vc = (int*)malloc(4 * (size_t)cells); int* tn = (int*)malloc(4 * (size_t)cells);
    double* w = (double*)malloc(8 * (size_t)cells); double* q = (double*)malloc(8 * (size_t)cells); opt_t* o = (opt_t*)malloc(sizeof(opt_t) * (size_t)n);
    double* x = (double*)malloc(8 * (size_t)nx);
    if (fread(off, 4, n + 1, f) != (size_t)(n + 1) || fread(vc, 4, cells, f) != (size_t)cells || fread(tn, 4, cells, f) != (size_t)cells ||
        fread(w, 8, cells, f) != (size_t)cells || fread(q, 8, cells, f) != (size_t)cells || fread(o, sizeof(opt_t), n, f) != (size_t)n ||
        fread(x, 8, nx, f) != (size_t)nx) return 4;
    fclose(f);
    int* res = (int*)malloc(16 * (size_t)n); double* lcb = (double*)malloc(8 * (size_t)cells); double* sx = (double*)malloc(8 * (size_t)nx);
    int* bx = (int*)malloc(4 * (size_t)nx);
    for (int i = 0; i < n; i++) {
        const int lo = off[i], K = off[i + 1] - lo;
        if (K <= 0 || K > 218) return 6;
        int cs, nc, bad;
        res[i * 4] = sz_lcb_move_host(vc + lo, tn + lo, w + lo, q + lo, K, (double)o[i].stdevs, (double)o[i].min_visit_prop, lcb + lo, &cs, &nc, &bad);
        res[i * 4 + 1] = cs; res[i * 4 + 2] = nc; res[i * 4 + 3] = bad;
    }
    for (int i = 0; i < nx; i++) { bx[i] = 0; sx[i] = sz_ssqrt(x[i], &bx[i]); }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(res, 16, n, f) != (size_t)n || fwrite(lcb, 8, cells, f) != (size_t)cells || fwrite(sx, 8, nx, f) != (size_t)nx ||
        fwrite(bx, 4, nx, f) != (size_t)nx) return 5;
    fclose(f);
    return 0;
}
"""


def test_host_compilation_of_the_header_equals_the_restatement_bit_for_bit(tmp_path, cases):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")      # hipcc's own host compiler
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert gxx, "no host C++ compiler (g++, c++, clang++ or the ROCm clang++): the header's host build cannot be held to the restatement"
    assert os.path.exists(os.path.join(CSRC, "sz_lcb.h")), "csrc/sz_lcb.h: the rule's scalar functions"
    hc, (move, cstar, ncand, bad, lcb, cov) = cases
    n, cells = len(hc.opts), len(hc.n)
    x = LR.ssqrt_arguments()
    src, exe, fin, fout = (str(tmp_path / x_) for x_ in ("lcb_host.cpp", "lcb_host", "cases.bin", "out.bin"))
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([gxx, "-O2", "-ffp-contract=off", "-std=c++17", "-I", CSRC, src, "-o", exe])
    assert hc.opts.dtype.itemsize == 12
    with open(fin, "wb") as f:
        f.write(np.array([n, cells, len(x)], np.int32).tobytes() + hc.offsets.tobytes() + hc.n.tobytes() + hc.N.tobytes() + hc.W.tobytes() + hc.Q.tobytes() +
                hc.opts.tobytes() + x.tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, np.uint8)
    res = raw[:16 * n].view(np.int32).reshape(n, 4)
    got_lcb = raw[16 * n:16 * n + 8 * cells].view(np.float64)
    got_sx = raw[16 * n + 8 * cells:16 * n + 8 * cells + 8 * len(x)].view(np.float64)
    got_bx = raw[16 * n + 8 * cells + 8 * len(x):].view(np.int32)
    want = np.stack([move, cstar, ncand, bad], 1)
    wrong = np.argwhere(res != want)
    assert not len(wrong), "case %d field %d: host %r, restatement %r (%d differ)" % (wrong[0][0], wrong[0][1], res[tuple(wrong[0])], want[tuple(wrong[0])], len(wrong))
    wrong = np.nonzero(~LR.same_bits(got_lcb, lcb))[0]
    assert not len(wrong), "child %d: host lcb %r, restatement %r (%d differ)" % (wrong[0], got_lcb[wrong[0]], lcb[wrong[0]], len(wrong))
    ref = [LR.ssqrt(v) for v in x.tolist()]
    assert LR.same_bits(got_sx, np.array([r for r, _ in ref])).all() and got_bx.tolist() == [b for _, b in ref] and sum(b for _, b in ref) >= 6


# ------------------------------------------------------------------------------------------------ 5. the Python layer
def test_lcb_options_of():
    nan, inf = float("nan"), float("inf")
    base = {"num_searches": 800}
    f32 = lambda v: float(np.float32(v))
    assert lcb_options_of(base) is None and lcb_options_of(dict(base, lcb=None)) is None
    assert lcb_options_of(dict(base, lcb={})) == (5.0, f32(0.15), True)
    assert lcb_options_of(dict(base, lcb={"stdevs": 1, "min_visit_prop": np.float32(0.5), "select": False})) == (1.0, 0.5, False)
    assert lcb_options_of(dict(base, lcb={"stdevs": 0.1, "min_visit_prop": 1})) == (f32(0.1), 1.0, True), "rounded to f32"
    for bad in (0.5, [], "lcb", True, {"z": 5.0}, {"stdevs": 5.0, "nope": 1}):
        with pytest.raises(ValueError, match=r"\['lcb'\] must be a dict"):
            lcb_options_of(dict(base, lcb=bad))
    for v in (nan, inf, -inf, -1e-9, 1e39, True, "5", None, [5.0]):
        with pytest.raises(ValueError, match=r"\['lcb'\]\['stdevs'\]"):
            lcb_options_of(dict(base, lcb={"stdevs": v}))
    for v in (nan, inf, -1e-9, 1.0000001, True, "0.15", None, [0.15]):
        with pytest.raises(ValueError, match=r"\['lcb'\]\['min_visit_prop'\]"):
            lcb_options_of(dict(base, lcb={"min_visit_prop": v}))
    for v in (0, 1, "yes", None, 1.0):
        with pytest.raises(ValueError, match=r"\['lcb'\]\['select'\]"):
            lcb_options_of(dict(base, lcb={"select": v}))
    with pytest.raises(ValueError, match=r"\['lcb'\]\['stdevs'\]"):                        # the order: stdevs, min_visit_prop, select, the combinations
        lcb_options_of(dict(base, lcb={"stdevs": nan, "min_visit_prop": 2, "select": 1}, gumbel={"m": 4}))
    with pytest.raises(ValueError, match=r"\['lcb'\]\['min_visit_prop'\]"):
        lcb_options_of(dict(base, lcb={"min_visit_prop": 2, "select": 1}, gumbel={"m": 4}))
    with pytest.raises(ValueError, match=r"\['lcb'\]\['select'\]"):
        lcb_options_of(dict(base, lcb={"select": 1}, gumbel={"m": 4}))
    with pytest.raises(ValueError, match="gumbel.*exclude each other"):
        lcb_options_of(dict(base, lcb={}, gumbel={"m": 4}, reuse_subtree=True))
    with pytest.raises(ValueError, match="reuse_subtree.*exclude each other"):
        lcb_options_of(dict(base, lcb={}, reuse_subtree=True))
    assert lcb_options_of(dict(base, lcb={}, reuse_subtree=False)) == (5.0, f32(0.15), True)
