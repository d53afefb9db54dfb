"""The restatement of the search summary (tests/summaryref.py) on the CPU: root_q and the surprise against math.fsum / math.log formulas within
four times the deviation measured here, best_q against endingref's m on every ply of seeded runs, the sign and the exact zero of the surprise,
bit for bit the host compilation of csrc/sz_summary.h, the conditions the GPU configurations are there for, and the Python layer
(selfplay.search_targets_of, train_rl.surprise_weights / resample_by_weight / records_from_games, train_rl's flags).
tests/test_gpu_search_summary.py holds the device to the restatement."""
import math
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import endingref as ER
import summaryref as SR
from sigma_zero_amd.selfplay import search_targets_of

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sigma-zero_amd", "csrc")
_played = {}


def _play(name):
    if name not in _played:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[name] = SR.play(next(c for c in SR.configs() if c.name == name))
    return _played[name]


@pytest.fixture(scope="module")
def cases():
    hc = SR.hook_cases()
    return hc, SR.hook_reference(hc)


# ------------------------------------------------------------------------------------------------ 1. the rule against fsum / log
def test_values_and_surprise_are_within_four_times_the_measured_deviation_of_fsum_and_math_log(cases):
    """Measured here (printed below, recorded in summaryref's docstring and DESIGN.md 3.1p): root_q deviates from -(fsum(W) / total) by at most
    1.2e-16 of max(1, |exact|) (measured 1.11e-16; ten additions deep at K = 218 and one division), the surprise from fsum(t * log(t / P)) by at most 4.3e-16 of
    max(1, sum |term|) (measured 4.24e-16; slog's 3.7e-16 relative error per term and the same summation).  The bounds are four times those, as for tempref and
    puctref: the comparison value goes through the platform's libm.  best_q is one division and one negation: equal to the bit."""
    hc, want = cases
    n = len(hc.n_child)
    assert n >= 1700 and set(SR.WIDTHS) <= set(hc.n_child.tolist())
    worst_q = worst_s = 0.0
    n_q = n_s = n_pruned = n_zero_children = n_one_child = n_dropped = n_no_record = n_no_tree = 0
    for i in range(n):
        N, W, P, r = SR.hook_case(hc, i)
        v = SR.values(N, W)
        if v is None:
            n_no_tree += 1
            assert np.isnan(want[i, 0]) and np.isnan(want[i, 1]) and (len(N) == 0 or int(N.sum()) == 0)
        else:
            eq, eb = SR.exact_values(N, W)
            dq = abs(v[0] - eq) / max(1.0, abs(eq))
            worst_q, n_q = max(worst_q, dq), n_q + 1
            assert dq <= SR.ROOT_Q_BOUND, "case %d (K %d): root_q %r against %r" % (i, len(N), v[0], eq)
            assert SR.bits(v[1]) == SR.bits(eb), "case %d: best_q %r against %r" % (i, v[1], eb)
            n_zero_children += bool((N == 0).any())
            n_one_child += int((N > 0).sum()) == 1
        s, dropped = SR.surprise(r, P)
        n_dropped += dropped
        if int(r.sum()) == 0:
            n_no_record += 1
            assert np.isnan(s)
            continue
        es, mass = SR.exact_surprise(r, P)
        ds = abs(s - es) / max(1.0, mass)
        worst_s, n_s = max(worst_s, ds), n_s + 1
        assert ds <= SR.SURPRISE_BOUND, "case %d (K %d): surprise %r against %r, sum |term| %r" % (i, len(N), s, es, mass)
        if not dropped:
            assert s >= -SR.SURPRISE_BOUND * max(1.0, mass), "case %d: KL(target || prior) is not negative: %r" % (i, s)
        n_pruned += not np.array_equal(r, N)
    print("root_q against fsum: %d cases, worst deviation %.3e of max(1, |exact|); surprise against fsum / math.log: %d cases, worst %.3e of max(1, sum |term|)"
          % (n_q, worst_q, n_s, worst_s))
    print("%d pruned records, %d trees with zero-visit children, %d with all visits on one child, %d dropped terms, %d records without a visit, %d trees without"
          % (n_pruned, n_zero_children, n_one_child, n_dropped, n_no_record, n_no_tree))
    assert worst_q <= SR.MEASURED_ROOT_Q_DEV and worst_s <= SR.MEASURED_SURPRISE_DEV, "the measured deviations in summaryref are out of date"
    assert n_pruned >= 300 and n_zero_children >= 300 and n_one_child >= 40 and n_dropped >= 8 and n_no_record >= 40 and n_no_tree >= 40


def test_surprise_is_zero_exactly_when_target_equals_prior_at_one_child():
    assert SR.bits(SR.surprise([5], np.array([1.0], np.float32))[0]) == SR.bits(0.0)
    assert SR.bits(SR.surprise([1], np.array([1.0], np.float32))[0]) == SR.bits(0.0)
    assert SR.surprise([5], np.array([0.5], np.float32)) == (math.log(2.0), 0)
    assert SR.surprise([3, 1], np.array([0.75, 0.25], np.float32))[0] == 0.0, "dyadic fractions: t / P is exactly 1"
    s, d = SR.surprise([4, 0, 4], np.array([0.25, 0.5, 0.25], np.float32))
    assert d == 0 and abs(s - math.log(2.0)) < 1e-15, "an unvisited child has no term"
    for bad in (0.0, -0.5, 1e-40, float("inf"), float("nan")):
        s, d = SR.surprise([2, 2], np.array([0.5, bad], np.float32))
        assert d == 1 and s == 0.5 * SR.slog(0.5 / 0.5) == 0.0, bad
    assert SR.surprise([0, 2], np.array([float("nan"), 1.0], np.float32)) == (0.0, 0), "a child without a visit forms no term: nothing is dropped"
    assert np.isnan(SR.surprise([0, 0], np.array([0.5, 0.5], np.float32))[0]) and np.isnan(SR.surprise([], [])[0])
    assert SR.values([], []) is None and SR.values([0, 0], [0.0, 0.0]) is None
    rq, bq = SR.values([3, 1, 0], [-1.5, 0.5, 9.0])
    assert rq == 0.25 and bq == 0.5, "W is from the child's side to move; an unvisited child's W is not read"
    assert SR.values([2, 2], [1.0, -2.0])[1] == -0.5, "the first maximum"
    assert SR.plays(True, True, False, False) and not any(SR.plays(*x) for x in ((False, True, False, False), (True, False, False, False),
                                                                                  (True, True, True, False), (True, True, False, True)))


# ------------------------------------------------------------------------------------------------ 2. whole searches
@pytest.mark.parametrize("name", [c.name for c in SR.configs()])
def test_best_q_is_endingrefs_m_on_every_ply(name):
    cfg = next(c for c in SR.configs() if c.name == name)
    games, recs, sums, trees, priors = _play(name)
    n = n_normalised = 0
    for b, g in enumerate(games):
        played = [ply for ply in range(cfg.plies) if recs[ply][b] is not None]
        assert len(played) == len(g.searches)
        if cfg.endings is not None:
            assert len(g.values) == len(played), "endingref recorded an m for every ply played"
        for i, ply in enumerate(played):
            sm, N = sums[ply][b], trees[ply][b]
            assert sm.valid == 1 and sm.dropped == 0
            assert -1.0 <= sm.root_q <= 1.0 and -1.0 <= sm.best_q <= 1.0
            P, r = priors[ply][b], recs[ply][b]["visits"][:len(N)]
            es, mass = SR.exact_surprise(r, P)
            assert abs(sm.surprise - es) <= SR.SURPRISE_BOUND * max(1.0, mass)
            if float(np.sum(P, dtype=np.float64)) <= 1.0 + 1e-5:     # priors that sum to 1: a Kullback-Leibler divergence, not negative
                n_normalised += 1
                assert sm.surprise >= -SR.SURPRISE_BOUND * max(1.0, mass), (name, b, ply, sm.surprise)
            if cfg.endings is not None:
                assert SR.bits(sm.best_q) == SR.bits(g.values[i]), "%s board %d ply %d" % (name, b, ply)
            n += 1
        for ply in range(cfg.plies):
            if recs[ply][b] is None:
                assert sums[ply][b] is SR.NO_SUMMARY
    assert n >= 6 * 4
    print(name, "%d plies, %d with priors that sum to 1" % (n, n_normalised))
    if not cfg.learning or cfg.noise:                          # no noise, or Dirichlet root noise: every root's priors sum to 1
        assert n_normalised == n


def test_best_q_is_mover_value_on_the_hook_cases(cases):
    hc, want = cases
    n = 0
    for i in range(len(hc.n_child)):
        N, W, _, _ = SR.hook_case(hc, i)
        if len(N) and int(N.sum()) > 0:
            assert SR.bits(want[i, 1]) == SR.bits(float(ER.mover_value(N, W)[1])), i
            n += 1
    assert n >= 1600


def test_configurations_reach_their_conditions():
    by = {c.name: _play(c.name) for c in SR.configs()}
    games, recs, sums, trees, _ = by["forced_fpu_endings_noise"]
    cfg_plies = next(c for c in SR.configs() if c.name == "forced_fpu_endings_noise").plies
    pruned = SR.pruned_plies(recs, trees)
    print("forced: %d (ply, board) with pruned != tree counts, %d pruned visits" % (len(pruned), sum(g.pruned_visits for g in games)))
    assert len(pruned) >= 4, "the surprise is formed on other counts than the tree's"
    for ply, b in pruned:                                   # ... and is another number there
        N = trees[ply][b]
        f_rec = sums[ply][b].surprise
        assert sum(g.forced_selections for g in games) > 0 and int(recs[ply][b]["visits"].sum()) < int(N.sum()) and f_rec == f_rec
    ended = [(b, len(g.searches) - 1) for b, g in enumerate(games) if g.termination is not None]
    assert ended and any(ply < cfg_plies - 1 for _, ply in ended), "a rule ends a game, one of them early enough for the board to sit out a ply"
    for b, ply in ended:                                    # the ending fired instead of a move: the record exists and so does the summary
        assert int(recs[ply][b]["chosen"]) == -1 and sums[ply][b].valid == 1 and sums[ply][b].surprise == sums[ply][b].surprise
    for name in ("plain", "L4_solver_reuse", "playout_cap_budgets_kld"):
        assert not SR.pruned_plies(by[name][1], by[name][3])
    games = by["L4_solver_reuse"][0]
    assert any(s == "reused" for g in games for s in g.starts), "kept subtrees"
    games = by["playout_cap_budgets_kld"][0]
    assert sum(g.kld_stats[0] for g in games) > 0, "boards stopped early under the summary"
    for name, (games, recs, sums, trees, _) in by.items():
        dead = sum(1 for row in recs for r in row if r is None)
        print(name, "plies played", sum(len(g.searches) for g in games), "boards that did not play", dead)
    assert any(r is None for name in by for row in by[name][1] for r in row), "a board whose game is over: valid = 0"


# ------------------------------------------------------------------------------------------------ 3. the header on the host
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "sz_summary.h"
#define MAX_MOVES 218
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n <= 0) return 3;
    const size_t cells = (size_t)n * MAX_MOVES;
    int* k = (int*)malloc(4 * (size_t)n); int* tn = (int*)malloc(4 * cells); double* tw = (double*)malloc(8 * cells);
    float* pr = (float*)malloc(4 * cells); int* rv = (int*)malloc(4 * cells);
    double* out = (double*)malloc(8 * 4 * (size_t)n);
    if (fread(k, 4, n, f) != (size_t)n || fread(tn, 4, cells, f) != cells || fread(tw, 8, cells, f) != cells || fread(pr, 4, cells, f) != cells ||
        fread(rv, 4, cells, f) != cells) return 4;
    fclose(f);
    for (int i = 0; i < n; i++) {
        const int K = k[i];
        if (K < 0 || K > MAX_MOVES) return 6;
        const int* N = tn + (size_t)i * MAX_MOVES; const double* W = tw + (size_t)i * MAX_MOVES;
        const float* P = pr + (size_t)i * MAX_MOVES; const int* R = rv + (size_t)i * MAX_MOVES;
        double* o = out + (size_t)i * 4;
        o[0] = o[1] = o[2] = sz_summary_nan(); o[3] = 0.0;
        int total = 0, rtotal = 0, bi = 0;
        for (int c = 0; c < K; c++) { total += N[c]; rtotal += R[c]; if (N[c] > N[bi]) bi = c; }
        if (K > 0 && total != 0) {
            o[0] = sz_summary_root_q(sz_summary_wsum_host([&](int c) { return sz_summary_value_term(N[c], W[c]); }, K), total);
            o[1] = sz_summary_best_q(W[bi], N[bi]);
        }
        if (rtotal != 0) {
            int dropped = 0;
            o[2] = sz_summary_wsum_host([&](int c) { return sz_summary_term(R[c], rtotal, P[c], &dropped); }, K);
            o[3] = (double)dropped;
        }
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out, 8, 4 * (size_t)n, f) != 4 * (size_t)n) return 5;
    fclose(f);
    return 0;
}
"""


def test_host_compilation_of_the_header_equals_the_restatement_bit_for_bit(tmp_path, cases):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")      # hipcc's own host compiler
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert gxx, "no host C++ compiler (g++, c++, clang++ or the ROCm clang++): the header's host build cannot be held to the restatement"
    assert os.path.exists(os.path.join(CSRC, "sz_summary.h")), "csrc/sz_summary.h: the rule's scalar functions"
    hc, want = cases
    n = len(hc.n_child)
    src, exe, fin, fout = (str(tmp_path / x) for x in ("summary_host.cpp", "summary_host", "cases.bin", "out.bin"))
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([gxx, "-O2", "-ffp-contract=off", "-std=c++17", "-I", CSRC, src, "-o", exe])
    with open(fin, "wb") as f:
        f.write(np.int32(n).tobytes() + hc.n_child.tobytes() + hc.tree_vc.tobytes() + hc.value_sum.tobytes() + hc.prior.tobytes() + hc.record_vc.tobytes())
    subprocess.check_call([exe, fin, fout])
    got = np.fromfile(fout, np.float64).reshape(n, 4)
    bad = np.argwhere(~SR.same_bits(got[:, :3], want))
    assert not len(bad), "case %d value %d: host %r, restatement %r (%d differ)" % (bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
    dropped = [SR.surprise(SR.hook_case(hc, i)[3], SR.hook_case(hc, i)[2])[1] for i in range(n)]
    assert got[:, 3].astype(np.int64).tolist() == dropped and sum(dropped) >= 8
    assert len(set(want[~np.isnan(want)].tolist())) > 3000, "the cases are not a handful of values"


# ------------------------------------------------------------------------------------------------ 4. the Python layer
def test_search_targets_of():
    nan, inf = float("nan"), float("inf")
    base = {"num_searches": 800}
    assert search_targets_of(base) is None and search_targets_of(dict(base, search_targets=None)) is None
    assert search_targets_of(dict(base, search_targets={})) == (0.0, "root", 0.0)
    assert search_targets_of(dict(base, search_targets={"q_ratio": 1, "q_source": "best", "surprise_fraction": np.float32(0.5)})) == (1.0, "best", 0.5)
    for bad in (0.5, [], "root", {"ratio": 0.5}, {"q_ratio": 0.5, "nope": 1}):
        with pytest.raises(ValueError, match=r"\['search_targets'\] must be a dict"):
            search_targets_of(dict(base, search_targets=bad))
    for key in ("q_ratio", "surprise_fraction"):
        for v in (nan, inf, -inf, -1e-9, 1.0000001, True, "0.5", None, [0.5]):
            with pytest.raises(ValueError, match=r"\['search_targets'\]\[%r\]" % key):
                search_targets_of(dict(base, search_targets={key: v}))
    for v in ("Root", "", "mean", None, 0, True):
        with pytest.raises(ValueError, match=r"\['search_targets'\]\['q_source'\]"):
            search_targets_of(dict(base, search_targets={"q_source": v}))
    with pytest.raises(ValueError, match=r"\['search_targets'\]\['q_ratio'\]"):            # the order: q_ratio, q_source, surprise_fraction, the combination
        search_targets_of(dict(base, search_targets={"q_ratio": nan, "q_source": "x", "surprise_fraction": 2}, gumbel={"m": 4}))
    with pytest.raises(ValueError, match=r"\['search_targets'\]\['q_source'\]"):
        search_targets_of(dict(base, search_targets={"q_source": "x", "surprise_fraction": 2}, gumbel={"m": 4}))
    with pytest.raises(ValueError, match=r"\['search_targets'\]\['surprise_fraction'\]"):
        search_targets_of(dict(base, search_targets={"surprise_fraction": 2}, gumbel={"m": 4}))
    with pytest.raises(ValueError, match="exclude each other"):
        search_targets_of(dict(base, search_targets={}, gumbel={"m": 4}))


def test_surprise_weights():
    from sigma_zero_amd.train_rl import surprise_weights
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 1000):
        s = rng.gamma(0.5, 1.0, size=n).tolist()
        assert surprise_weights(s, 0.0) == [1.0] * n, "f = 0: all ones"
        for f in (0.25, 0.5, 1.0):
            w = surprise_weights(s, f)
            assert abs(math.fsum(w) - n) <= 1e-12 * n and min(w) >= 1.0 - f - 1e-15, (n, f)
            assert all(abs(x - ((1.0 - f) + f * n * y / math.fsum(s))) <= 1e-12 * max(1.0, x) for x, y in zip(w, s))
    assert surprise_weights([0.0, 0.0, 0.0], 0.5) == [1.0] * 3 and surprise_weights([], 0.5) == [], "sum(s) == 0: all ones"
    assert surprise_weights([float("nan"), float("nan")], 1.0) == [1.0, 1.0]
    assert surprise_weights([float("nan"), 2.0, -1e-17, 2.0], 1.0) == [0.0, 2.0, 0.0, 2.0], "a NaN and a rounding below 0 count as 0"
    assert surprise_weights([1.0, 3.0], 0.5) == [0.75, 1.25]
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            surprise_weights([1.0], bad)


def test_resample_by_weight():
    from sigma_zero_amd.train_rl import resample_by_weight, surprise_weights
    g = lambda seed=3: np.random.default_rng(seed)
    assert resample_by_weight(4, [1, 0, 3, 2], g()) == [0, 2, 2, 2, 3, 3], "integer weights: exact replication"
    assert resample_by_weight(3, [1.0, 1.0, 1.0], g()) == [0, 1, 2] and resample_by_weight(0, [], g()) == []
    s = np.random.default_rng(9).gamma(0.5, 1.0, size=500).tolist()
    w = surprise_weights(s, 0.5)
    a, b = resample_by_weight(500, w, g(11)), resample_by_weight(500, w, g(11))
    assert a == b and a == sorted(a), "the same generator gives the same list, in record order"
    assert a != resample_by_weight(500, w, g(12))
    lo, hi = sum(int(math.floor(x)) for x in w), sum(int(math.ceil(x)) for x in w)
    assert lo <= len(a) <= hi and lo < hi, "the length lies in the Bernoulli range"
    counts = np.bincount(a, minlength=500)
    assert all(math.floor(x) <= c <= math.ceil(x) for x, c in zip(w, counts))
    gen = g(11)                                             # one draw per record whatever its weight: the generator ends where 500 draws leave it
    resample_by_weight(500, w, gen)
    ref = g(11)
    ref.random(500)
    assert gen.random() == ref.random()
    for bad in ([1.0, -0.5], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError):
            resample_by_weight(2, bad, g())
    with pytest.raises(ValueError):
        resample_by_weight(3, [1.0, 1.0], g())


def test_records_from_games_takes_the_blended_targets_on_request():
    from sigma_zero_amd import train_rl
    packed = [np.zeros((119, 8), np.uint8), np.ones((119, 8), np.uint8)]
    game = dict(states=[None, None], packed_states=packed, actions=[{}, {}], rewards=[1, -1], value_targets=[0.75, -0.25], colours=[True, False])
    assert train_rl.records_from_games([game])[3] == [1, -1]
    assert train_rl.records_from_games([game], value_key="rewards")[3] == [1, -1]
    assert train_rl.records_from_games([game], value_key="value_targets")[3] == [0.75, -0.25]


def _move(k):
    """the k-th action index that names a move on the board, as a move"""
    from sigma_zero_amd.chess_tensor import action_index, index_to_move
    found = -1
    for idx in range(4672):
        try:
            mv = index_to_move(idx, True)
        except IndexError:
            continue
        if action_index(mv, True) == idx:
            found += 1
            if found == k:
                return mv
    raise AssertionError(k)


def _fake_games():
    """two games of 3 and 2 samples whose every field names its sample: packed state filled with the sample's number, one move per sample"""
    games, k = [], 0
    for n in (3, 2):
        g = dict(states=[None] * n, packed_states=[], actions=[], rewards=[], value_targets=[], surprises=[], colours=[])
        for _ in range(n):
            g["packed_states"].append(np.full((119, 8), k, np.uint8))
            g["actions"].append({_move(k): 1.0})
            g["rewards"].append(1 if k % 2 == 0 else -1)
            g["value_targets"].append(0.125 * k)
            g["colours"].append(True)
            k += 1
        games.append(g)
    for g, s in zip(games, ([0.0, 2.0, float("nan")], [0.0, 2.0])):
        g["surprises"] = s
    return games


def test_training_records_blend_and_resample_stay_aligned():
    """what run_cycle trains on: the value key, the surprises flattened in record order, and one resampling applied to all four lists"""
    from sigma_zero_amd import train_rl
    games = _fake_games()
    from sigma_zero_amd.chess_tensor import action_index
    number = {action_index(_move(k), True): k for k in range(5)}
    ident = lambda recs: [(int(p[0, 0]), number[int(i[0])], float(q[0]), r) for p, i, q, r in zip(*recs)]
    plain = ident(train_rl.training_records(games))
    assert [x[0] for x in plain] == [x[1] for x in plain] == [0, 1, 2, 3, 4] and [x[3] for x in plain] == [1, -1, 1, -1, 1]
    assert ident(train_rl.training_records(games, (0.0, "root", 0.0))) == plain and ident(train_rl.training_records(games, None, np.random.default_rng(1))) == plain
    blended = ident(train_rl.training_records(games, (0.5, "best", 0.0)))
    assert [x[:3] for x in blended] == [x[:3] for x in plain] and [x[3] for x in blended] == [0.0, 0.125, 0.25, 0.375, 0.5]
    # f = 1: w = 5 * s / 4 = (0, 2.5, 0, 0, 2.5): records 1 and 4 twice or three times, the others never; each copy carries its own fields
    seen = set()
    for seed in range(8):
        recs = ident(train_rl.training_records(games, (0.5, "root", 1.0), np.random.default_rng(seed)))
        ids = [x[0] for x in recs]
        assert ids == sorted(ids) and set(ids) == {1, 4} and all(ids.count(i) in (2, 3) for i in (1, 4))
        assert all(x[0] == x[1] and x[3] == 0.125 * x[0] for x in recs), "every list was resampled with the same indices"
        assert recs == ident(train_rl.training_records(games, (0.5, "root", 1.0), np.random.default_rng(seed)))
        seen.add(tuple(ids))
    assert len(seen) > 1, "the generator decides the fractional copies"
    # f = 0.5 keeps every record at least ... w = 0.5 + 0.5 * (0, 2.5, 0, 0, 2.5): rewards stay the value targets at q_ratio 0
    recs = ident(train_rl.training_records(games, (0.0, "root", 0.5), np.random.default_rng(0)))
    assert all(x[3] == (1 if x[0] % 2 == 0 else -1) for x in recs) and [x[0] for x in recs].count(1) in (1, 2)
    games[1]["surprises"] = [0.0]
    with pytest.raises(ValueError, match="4 surprises for 5 records"):
        train_rl.training_records(games, (0.0, "root", 0.5), np.random.default_rng(0))


def test_run_cycle_hands_the_search_targets_to_training_records():
    """run_cycle's own part: it reads args["search_targets"] and passes the games, the targets and the generator on"""
    import inspect
    from sigma_zero_amd import train_rl
    src = inspect.getsource(train_rl.run_cycle)
    assert "targets = search_targets_of(args)" in src and "training_records(games, targets, resample_generator)" in src
    assert "resample_generator" in inspect.signature(train_rl.run_cycle).parameters


def test_train_rl_flags():
    from sigma_zero_amd import train_rl
    flags = train_rl.flag_parser()
    assert "search_targets" not in train_rl.selfplay_args_of(flags.parse_args([]))
    a = train_rl.selfplay_args_of(flags.parse_args(["--q-ratio", "0.25"]))
    assert a["search_targets"] == {"q_ratio": 0.25} and search_targets_of(a) == (0.25, "root", 0.0)
    a = train_rl.selfplay_args_of(flags.parse_args(["--q-ratio", "0.5", "--q-source", "best", "--surprise-fraction", "0.5"]))
    assert a["search_targets"] == {"q_ratio": 0.5, "q_source": "best", "surprise_fraction": 0.5} and search_targets_of(a) == (0.5, "best", 0.5)
    assert search_targets_of(train_rl.selfplay_args_of(flags.parse_args(["--surprise-fraction", "1"]))) == (0.0, "root", 1.0)
    with pytest.raises(ValueError):
        search_targets_of(train_rl.selfplay_args_of(flags.parse_args(["--q-ratio", "0.5", "--gumbel", "8"])))
    with pytest.raises(SystemExit):
        flags.parse_args(["--q-source", "mean"])
