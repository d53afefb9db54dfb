"""The restatement of KLD-gain early stopping (tests/kldref.py) on the CPU: puctref while the option is off, gain() against math.fsum and
math.log, bit for bit the host compilation of csrc/sz_kldgain.h, the invariant (a board stopped at s is the board searched with goal s), the
conditions the GPU configurations are there for with thresholds no decision comes near, and the Python layer's validation
(selfplay.kld_stop_options_of, train_rl's flags).  tests/test_gpu_kld_stop.py holds the device to it."""
import math
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import kldref as KR
import puctref as PR
from kldref import KldStop
from sigma_zero_amd.selfplay import kld_stop_options_of

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sigma-zero_amd", "csrc")
_played = {}


def _play(name, **kw):
    key = (name, tuple(sorted(kw.items(), key=str)))
    if key not in _played:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[key] = KR.play(next(c for c in KR.all_configs() if c.name == name), **kw)
    return _played[key]


def _same_record(a, b):
    if a is None or b is None:
        return a is b
    return all(np.array_equal(a[k], b[k]) for k in ("packed", "action", "visits")) and \
        all(int(a[k]) == int(b[k]) for k in ("n_child", "colour", "chosen", "game_over", "result"))


def _same_tree(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. option off is puctref
def test_option_off_is_puctref_ply_after_ply():
    """kldref.Game turns every search into a Stepwise one, its _run a restatement of composeref's: with kld_stop None nothing else differs"""
    cfg = next(c for c in PR.configs() if c.name == "L4_solver_reuse")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want, wrecs = PR.play(cfg)
        games = [PR.new_game(cfg, b) for b in range(len(cfg.boards))]
        for g in games:
            g.__class__, g.kld_stop, g.kld_chunk, g.kld_plies, g.kld_stats = KR.Game, None, None, [], [0, 0, 0]
        for ply in range(cfg.plies):
            for b, (g, bd) in enumerate(zip(games, cfg.boards)):
                if g.live:
                    PR.begin_ply(cfg, g, b, ply, None)
                    g.run()
                    assert g.error is None and isinstance(g.search, KR.Stepwise) and g.search.kld is None
                    assert _same_record(g.play(bd.u(ply)), wrecs[ply][b]), (ply, b)
    n = 0
    for g, w in zip(games, want):
        assert g.starts == w.starts and g.chosen == w.chosen and all(getattr(g, k) == getattr(w, k) for k in g.COUNTERS)
        for s, t in zip(g.searches, w.searches):
            assert _same_tree(s.tree(), t.tree()) and _same_tree(s.begin_tree, t.begin_tree) and s.begin_rows == t.begin_rows
            assert len(s.steps) == len(t.steps) and all(np.array_equal(x, y) for x, y in zip(s.steps, t.steps))
            assert s.stopped_at == -1 and s.checks == 0 and not s.kld_log
            n += 1
    assert n >= 12 and any(x == "reused" for g in games for x in g.starts)


# ------------------------------------------------------------------------------------------------ 2. the gain
@pytest.fixture(scope="module")
def cases():
    gc = KR.gain_cases()
    return gc, [KR.terms(gc.prev[i, :k], gc.now[i, :k]) for i, k in enumerate(gc.n_child)]


def test_gain_is_within_the_derived_bound_of_fsum_and_math_log(cases):
    """|gain - exact| <= 2^-44 * sum |term_c|.  Derived: a term carries at most 8 roundings of 2^-53 (two int -> f64 conversions that are exact
    below 2^53, two divisions, the quotient, slog's error of a few 2^-53 of its result, the product), the summation is at most 10 additions
    deep (4 in a lane at K = 218, 6 butterfly levels), each adding 2^-53 of a partial sum that is at most sum |term|: together below 2^-48.
    The bound leaves 16x over that."""
    gc, ts = cases
    n = len(gc.n_child)
    assert n >= 19000 and set(KR.WIDTHS) <= set(gc.n_child.tolist())
    worst, n_zero, n_unvisited, n_single = 0.0, 0, 0, 0
    for i, k in enumerate(gc.n_child):
        prev, now = gc.prev[i, :k], gc.now[i, :k]
        got = KR.lane_sum(ts[i])
        want, mass = KR.gain_exact(prev, now)
        n_unvisited += bool((prev == 0).any())
        n_single += int(now.sum()) - int(prev.sum()) == 1
        if np.array_equal(prev, now):
            n_zero += 1
            assert got == 0.0 and all(t == 0.0 for t in ts[i]), "now == prev: every term is exactly 0 (case %d)" % i
        assert abs(got - want) <= 2.0 ** -44 * mass, "case %d (K %d): %r against %r, sum |term| %r" % (i, k, got, want, mass)
        if mass > 0:
            worst = max(worst, abs(got - want) / mass)
    print("gain against fsum / math.log: %d cases, worst |d| / sum |term| = 2^%.1f; %d with now == prev, %d with unvisited children, %d single visits"
          % (n, math.log2(worst) if worst else -math.inf, n_zero, n_unvisited, n_single))
    assert n_zero >= 30 and n_unvisited >= 1000 and n_single >= 1000
    assert max(int(gc.now[i, :k].sum()) for i, k in enumerate(gc.n_child)) >= 10 ** 5
    # the quantity itself: a distribution that does not move gains nothing, one that moves gains something positive
    assert KR.gain([5, 3, 2], [10, 6, 4]) == 0.0 and KR.gain([5, 3, 2], [5, 3, 12]) > 0.1


PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "sz_kldgain.h"
#define MAX_MOVES 218
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n <= 0) return 3;
    const size_t cells = (size_t)n * MAX_MOVES;
    int* prev = (int*)malloc(4 * cells); int* now = (int*)malloc(4 * cells); int* k = (int*)malloc(4 * (size_t)n);
    double* t = (double*)calloc(cells, 8);
    if (fread(prev, 4, cells, f) != cells || fread(now, 4, cells, f) != cells || fread(k, 4, n, f) != (size_t)n) return 4;
    fclose(f);
    for (int i = 0; i < n; i++) {
        const int* p = prev + (size_t)i * MAX_MOVES; const int* q = now + (size_t)i * MAX_MOVES;
        if (k[i] < 0 || k[i] > MAX_MOVES) return 6;
        int pt = 0, nt = 0;
        for (int c = 0; c < k[i]; c++) { pt += p[c]; nt += q[c]; }
        for (int c = 0; c < k[i]; c++) t[(size_t)i * MAX_MOVES + c] = sz_kld_term(p[c], pt, q[c], nt);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(t, 8, cells, f) != cells) return 5;
    fclose(f);
    return 0;
}
"""


def test_host_compilation_of_the_header_equals_term_bit_for_bit(tmp_path, cases):
    gxx = shutil.which("g++") or shutil.which("c++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    assert os.path.exists(os.path.join(CSRC, "sz_kldgain.h")), "csrc/sz_kldgain.h: the rule's scalar function"
    gc, ts = cases
    n = len(gc.n_child)
    src, exe, fin, fout = (str(tmp_path / x) for x in ("kld_host.cpp", "kld_host", "cases.bin", "terms.bin"))
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([gxx, "-O2", "-ffp-contract=off", "-std=c++17", "-I", CSRC, src, "-o", exe])
    with open(fin, "wb") as f:
        f.write(np.int32(n).tobytes() + gc.prev.tobytes() + gc.now.tobytes() + gc.n_child.tobytes())
    subprocess.check_call([exe, fin, fout])
    got = np.fromfile(fout, np.float64).reshape(n, KR.MAX_MOVES)
    want = np.zeros((n, KR.MAX_MOVES), np.float64)
    for i, t in enumerate(ts):
        want[i, :len(t)] = t
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert not len(bad), "case %d child %d: host %r, restatement %r (%d differ)" % (bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
    assert len(set(want[want != 0].tolist())) > 50000, "the cases are not a handful of values"


# ------------------------------------------------------------------------------------------------ 3. whole searches
def test_configurations_reach_their_conditions_and_no_decision_is_near_the_threshold():
    cfgs = KR.all_configs()
    by, n_evals, closest = {}, 0, math.inf
    for cfg in cfgs:
        games, _ = _play(cfg.name)
        by[cfg.name] = KR.coverage([games])
        for g in games:
            assert all(ks == KR.checked(cfg.kld, cfg.S) for ks in g.kld_plies)
            for s in g.searches:
                for prev, now, got, stopped in s.kld_evals:
                    exact = KR.gain_exact(prev, now)[0] / float(int(now.sum()) - int(prev.sum()))
                    rel = abs(exact - cfg.kld.min_gain) / cfg.kld.min_gain
                    closest, n_evals = min(closest, rel), n_evals + 1
                    assert rel > 1e-9 and (exact < cfg.kld.min_gain) == (got < cfg.kld.min_gain), (cfg.name, exact, got)
                assert s.stopped_at < 0 or (s.sims == s.stopped_at <= s.goal0 and s.stopped_at >= cfg.kld.min_simulations)
                assert s.stopped_at >= 0 or s.sims == s.goal0
        print(cfg.name, {k: by[cfg.name][k] for k in KR.COVERAGE}, "kld_stats", [sum(g.kld_stats[i] for g in games) for i in range(3)])
    print("%d gains formed; the closest lies a relative %.2e from its threshold" % (n_evals, closest))
    KR.assert_coverage(sum(by.values(), KR.collections.Counter()))
    assert n_evals >= 100
    assert by["L4_solver_reuse"]["kld_stop_with_several_in_flight"] > 0 and by["L4_solver_reuse"]["kld_stop_on_continued_search"] > 0
    assert by["L4_solver_reuse"]["kld_proven_root_done_before_any_check"] > 0
    assert by["forced_fpu_endings_noise_cpuct"]["kld_stop_withheld_by_min_simulations"] > 0
    assert by["budgets"]["kld_stop_below_num_searches_goal"] > 0 and by["visit_targets"]["kld_stop_on_continued_search"] > 0
    assert all(by[c.name]["kld_stop_at_second_check"] + by[c.name]["kld_stop_at_later_check"] > 0 for c in cfgs), "every configuration: a board stops early"


@pytest.mark.parametrize("name", ["plain", "budgets", "visit_targets", "visit_targets_L4"])
def test_a_board_stopped_at_s_is_the_board_searched_with_goal_s(name):
    """the invariant, on the restatement: the same plies with the option off and stopped_at as the budget (on a reuse engine the visit target
    stopped_at + N_kept - 1) give the same trees, records and counters"""
    cfg = next(c for c in KR.all_configs() if c.name == name)
    games, recs = _play(name)
    goals = []
    for ply in range(cfg.plies):
        row = []
        for b, g in enumerate(games):
            s = g.searches[ply] if ply < len(g.searches) else None
            row.append(0 if s is None else (s.sims + s.n_kept - 1 if cfg.reuse else s.sims))
        goals.append(row)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        off, orecs = KR.play(cfg, kld=None, goals=goals)
    n_stopped = 0
    for g, o in zip(games, off):
        assert g.starts == o.starts and g.chosen == o.chosen and all(getattr(g, k) == getattr(o, k) for k in g.COUNTERS), (name, g.starts, o.starts)
        for s, t in zip(g.searches, o.searches):
            assert _same_tree(s.tree(), t.tree()) and _same_tree(s.tree_proven(), t.tree_proven())
            assert len(s.steps) == len(t.steps) and all(np.array_equal(x, y) for x, y in zip(s.steps, t.steps))
            n_stopped += s.stopped_at >= 0
    assert all(_same_record(a, b) for ra, rb in zip(recs, orecs) for a, b in zip(ra, rb))
    assert n_stopped >= 2


def test_a_change_of_the_option_keeps_the_kept_subtree():
    cfg = next(c for c in KR.configs() if c.name == "visit_targets")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        games = [KR.new_game(cfg, b) for b in range(len(cfg.boards))]
        for ply, setting in enumerate([cfg.kld, None, KldStop(0.5, 8, 4), cfg.kld]):
            for b, (g, bd) in enumerate(zip(games, cfg.boards)):
                g.kld_stop = setting
                KR.begin_ply(cfg, g, b, ply, None)
                g.run()
                g.play(bd.u(ply))
    assert all(g.starts[1:] == ["reused"] * 3 for g in games), [g.starts for g in games]
    assert all(g.kld_plies[1] is None and g.searches[1].stopped_at == -1 for g in games)


# ------------------------------------------------------------------------------------------------ 4. the Python layer
def test_kld_stop_options_of():
    nan, inf = float("nan"), float("inf")
    base = {"num_searches": 800}
    assert kld_stop_options_of(base) is None and kld_stop_options_of(dict(base, kld_stop=None)) is None
    assert kld_stop_options_of(dict(base, kld_stop={})) == (5e-6, 100, 0)
    assert kld_stop_options_of({"num_searches": 32, "kld_stop": {}}) == (5e-6, 32, 0)
    assert kld_stop_options_of(dict(base, kld_stop={"min_gain": 1, "interval": np.int32(8), "min_simulations": 800})) == (1.0, 8, 800)
    for bad in (5e-6, [], {"gain": 1e-3}, {"min_gain": 1e-3, "nope": 1}):
        with pytest.raises(ValueError, match=r"\['kld_stop'\] must be a dict"):
            kld_stop_options_of(dict(base, kld_stop=bad))
    for key, values in (("min_gain", (nan, inf, -inf, 0, 0.0, -1e-6, 1.0000001, True, "1e-3", None)), ("interval", (0, -1, 801, 8.0, True, nan, None)),
                        ("min_simulations", (-1, 801, 0.5, False, inf, None))):
        for v in values:
            if v is None and key == "min_gain":
                continue
            with pytest.raises(ValueError, match=r"\['kld_stop'\]\[%r\]" % key):
                kld_stop_options_of(dict(base, kld_stop={key: v}))
    with pytest.raises(ValueError, match=r"\['kld_stop'\]\['min_gain'\]"):        # the order: min_gain before interval before the combinations
        kld_stop_options_of(dict(base, kld_stop={"min_gain": nan, "interval": 0}, gumbel={"m": 4}))
    with pytest.raises(ValueError, match=r"\['kld_stop'\]\['interval'\]"):
        kld_stop_options_of(dict(base, kld_stop={"interval": 0, "min_simulations": -1}, gumbel={"m": 4}))
    with pytest.raises(ValueError, match="exclude each other"):
        kld_stop_options_of(dict(base, kld_stop={}, gumbel={"m": 4}))


def test_train_rl_flags():
    from sigma_zero_amd import train_rl
    flags = train_rl.flag_parser()
    assert "kld_stop" not in train_rl.selfplay_args_of(flags.parse_args([]))
    a = train_rl.selfplay_args_of(flags.parse_args(["--kld-min-gain", "5e-6"]))
    assert a["kld_stop"] == {"min_gain": 5e-6} and kld_stop_options_of(a) == (5e-6, min(100, a["num_searches"]), 0)
    a = train_rl.selfplay_args_of(flags.parse_args(["--searches", "800", "--kld-min-gain", "1e-4", "--kld-interval", "50", "--kld-min-simulations", "200"]))
    assert a["kld_stop"] == {"min_gain": 1e-4, "interval": 50, "min_simulations": 200} and kld_stop_options_of(a) == (1e-4, 50, 200)
    a = train_rl.selfplay_args_of(flags.parse_args(["--searches", "800", "--kld-interval", "100"]))
    assert kld_stop_options_of(a) == (5e-6, 100, 0)
    with pytest.raises(ValueError):
        kld_stop_options_of(train_rl.selfplay_args_of(flags.parse_args(["--kld-min-gain", "5e-6", "--gumbel", "8"])))
