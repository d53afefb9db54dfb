"""The restatement tests/forcedref.py (forced playouts at the root, policy-target pruning of the record) on the CPU: with the option off it
is targetref bit for bit on targetref's own scenarios; the pruning rule on cases worked by hand; what the option leaves alone (the tree, the
subtree kept for the next ply); and the scenarios and hook cases tests/test_gpu_forced_playouts.py runs on the device reach every condition
they are there for."""
import collections
import math
import warnings

import numpy as np
import pytest

import forcedref as FR
import targetref as TR


# ------------------------------------------------------------------------------------------------ option off
@pytest.mark.parametrize("L,solver", TR.OPTIONS)
def test_is_targetref_with_the_option_off(L, solver):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        n_searches = 0
        for sc in TR.scenarios():
            sc = sc._replace(plies=min(sc.plies, 4), boards=sc.boards[:3])
            want, gam = TR.play(sc, L, solver), TR.gammas(sc)
            for b, (bd, w) in enumerate(zip(sc.boards, want)):
                g = FR.Game(bd.make(), sc.S, sc.edges_per_board, reuse=True, L=L, lam=1.0, solver=solver, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt)
                recs = []
                for ply in range(sc.plies):
                    if g.live:
                        g.set_root_noise(sc.noise[ply])
                        g.begin(bd.targets[ply], gam[ply][b] if sc.noise[ply] else None, bd.quiet[ply], forced_k=0.0)
                        g.run()
                        recs.append(g.play(bd.u(ply)))
                tag = "%s %s L=%d solver=%d" % (sc.name, bd.name, L, solver)
                assert g.starts == w.starts and g.chosen == w.chosen and g.goals == w.goals and g.error == w.error, tag
                assert all(getattr(g, k) == getattr(w, k) for k in TR.Game.COUNTERS), tag
                assert g.forced_selections == 0 and g.pruned_visits == 0 and len(recs) == len(w.chosen) >= 1, tag
                n_searches += len(g.searches)
                for a, s in zip(g.searches, w.searches):
                    assert type(a) is TR.Search, tag                        # it IS targetref's search, not a copy of it
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.tree(), s.tree())), tag
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.begin_tree, s.begin_tree)), tag
                    assert len(a.steps) == len(s.steps) and all(np.array_equal(x, y) for x, y in zip(a.steps, s.steps)), tag
        assert n_searches >= 30


# ------------------------------------------------------------------------------------------------ pruning by hand
def _hand(N, W, P, n_root, c, k):
    """the rule of include/sigmazero.h in plain Python floats; asserts that no comparison is closer than 1e-3, so that f32 rounding
    cannot decide any of them -> (counts, iterations run per child, whether the loop stopped at the PUCT bound)"""
    cs = max(range(len(N)), key=lambda i: (N[i], -i))
    sq = math.sqrt(n_root)
    q_of = lambda i: 1.0 - ((W[i] / (N[i] + 1e-6)) + 1.0) / 2.0
    best = q_of(cs) + (1.0 / (N[cs] + 1)) * sq * c * P[cs]
    out, iters, stopped = list(N), [0] * len(N), [False] * len(N)
    for i in range(len(N)):
        if i == cs or N[i] < 1:
            continue
        m = min(N[i], int(math.floor(math.sqrt(k * P[i] * (n_root - 1)))))
        n1 = N[i]
        for _ in range(m):
            x = q_of(i) + (1.0 / n1) * sq * c * P[i]
            assert abs(x - best) > 1e-3
            if x < best:
                n1 -= 1
                iters[i] += 1
            else:
                stopped[i] = True
                break
        if n1 < N[i] and n1 <= 1:
            n1 = 0
        out[i] = n1
    return out, iters, stopped, cs


def test_pruning_cases_worked_by_hand():
    # N_root = 37 (T = 36, sq = 6.0828), c_puct = 2, k = 8.  c* = child 0: best = 0.5 + (1/13) * 6.0828 * 2 * 0.4 = 0.8743
    N = [12, 2, 6, 12, 1, 3]
    W = [0.0, 2.0, -1.68, 0.0, -1.0, 3.0]
    P = [0.4, 0.01, 0.1, 0.2, 0.29, 0.04]
    #  1: m = min(2, floor(sqrt(8 * .01 * 36) = 1.69)) = 1; q = 0, u(1) = (1/2) * 12.166 * .01 = .061 < best -> 1 visit left, which goes too: 0
    #  2: m = min(6, floor(5.37)) = 5; q = .64; u(5) = (1/6) * 1.2166 = .2028: .8428 < best -> 5; u(4) = .2433: .8833 >= best: stops, 4 of m unused
    #  3: tied with c* at a later index, so it is pruned: m = min(12, floor(7.59)) = 7; q = .5, u(n) = 2.4331 / (n + 1): .7028, .7212, .7433, .7704,
    #     .8041, .8476 all < best -> 6; the 7th, u(5) = .4055: .9055 >= best: stops at 6
    #  4: m = min(1, floor(9.14)) = 1, capped by N_c; q = 1: stays
    #  5: m = min(3, floor(3.39)) = 3, capped by N_c; q = 0, u(2) = .1622, u(1) = .2433, u(0) = .4866, all < best: every visit goes
    want = [12, 0, 5, 6, 1, 0]
    hand, iters, stopped, cs = _hand(N, W, P, 37, 2.0, 8.0)
    assert hand == want and cs == 0
    assert iters == [0, 1, 1, 6, 0, 3] and stopped == [False, False, True, True, True, False]
    got, cstar, info = FR.prune(N, W, P, 37, 2.0, 8.0)
    assert got.tolist() == want and cstar == 0
    assert info["pruned_to_zero"] == 2 and info["stopped_at_bound"] == 2 and info["tied_with_best_later"] == 1 and info["m_capped_by_n"] == 2
    assert info["last_visit_taken"] == 1
    # K = 1: the only child is c*
    got, cstar, _ = FR.prune([5], [1.0], [1.0], 6, 2.0, 8.0)
    assert got.tolist() == [5] and cstar == 0
    # children without visits and a root with T = 0 lose nothing; the option's constant scales m_c only
    assert FR.prune([0, 3, 0], [0.0, 0.0, 0.0], [0.5, 0.3, 0.2], 4, 2.0, 8.0)[0].tolist() == [0, 3, 0]
    assert FR.prune([1, 1], [0.0, 0.0], [0.5, 0.5], 1, 2.0, 8.0)[0].tolist() == [1, 1]
    # k = 0.25: m = floor(3 * sqrt(P)) = 0, 0, 1, 1, 0 for children 1..5: child 3 loses one visit (.7028 < best), child 4 stays (q = 1)
    assert FR.prune(N, W, P, 37, 2.0, 0.25)[0].tolist() == [12, 2, 6, 11, 1, 3]


def test_forced_rule_by_hand():
    # n_p = 17, T = 16, k = 2: child c is forced while n_c < sqrt(2 * P_c * 16): P = .5 -> 4, P = .125 -> 2, P = .03125 -> 1
    N, K0, W = [9, 1, 1, 0], [0, 0, 0, 0], [0.0] * 4
    P = [0.5, 0.125, 0.03125, 0.34375]
    i, forced, info = FR.select_root(N, K0, W, P, None, 17, 2.0, 1.0, 2.0)
    assert (i, forced) == (1, True) and info["several_forced"] == 0           # child 1: 1 < 2; child 2: 1 < 1 is false; child 3 has no visit
    i, forced, _ = FR.select_root([9, 2, 1, 0], K0, W, P, None, 17, 2.0, 1.0, 2.0)
    assert (i, forced) == (3, False)                                        # nobody forced: PUCT takes the unvisited child with the large prior
    # in-flight counts count: n_p = 18, T = 17; one descent in flight through child 1 makes n_c = 2 < sqrt(2 * .125 * 17) = 2.06: forced; two make
    # n_c = 3, which is not, and child 2 is next: 1 < sqrt(2 * .03125 * 17) = 1.03
    i, forced, info = FR.select_root(N, [0, 1, 0, 0], W, P, None, 18, 2.0, 1.0, 2.0)
    assert (i, forced) == (1, True) and info["forced_in_flight"] == 1
    i, forced, info = FR.select_root(N, [0, 2, 0, 0], W, P, None, 18, 2.0, 1.0, 2.0)
    assert (i, forced) == (2, True) and info["forced_in_flight"] == 0
    # n_p = 1: T = 0 forces nothing
    assert FR.select_root([0, 0], [0, 0], [0.0, 0.0], [0.5, 0.5], None, 1, 2.0, 1.0, 2.0)[1] is False
    # proven WIN children are not forced while another child is open; when every child is WIN they are
    R = np.array([0, 1, 0, 0], np.int8)
    i, forced, info = FR.select_root(N, K0, W, P, R, 17, 2.0, 1.0, 2.0)
    assert forced is False and info["forced_win_skipped"] == 1
    i, forced, _ = FR.select_root(N, K0, W, P, np.ones(4, np.int8), 17, 2.0, 1.0, 2.0)
    assert (i, forced) == (1, True)


# ------------------------------------------------------------------------------------------------ scenarios and hook cases
_played = {}


def _play(name, L, solver):
    if (name, L, solver) not in _played:
        sc = next(s for s in FR.scenarios() if s.name == name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[(name, L, solver)] = (sc, FR.play(sc, L, solver))
    return _played[(name, L, solver)]


def _all_played():
    return [_play(sc.name, L, solver) for sc in FR.scenarios() for L, solver in FR.OPTIONS]


def test_the_tree_and_the_kept_subtree_hold_the_counted_visits():
    n_reused = 0
    for sc, games in _all_played():
        for g in games:
            assert g.error is None and len(g.searches) >= 1
            for ply, s in enumerate(g.searches):
                acts, vis = s.root_children()
                if g.forced_plies[ply]:
                    assert s.pruned is not None and (s.pruned <= vis).all() and s.pruned.sum() >= 1
                    assert s.pruned[int(np.argmax(vis))] == vis.max()                     # c* keeps its count
                if ply + 1 < len(g.searches) and g.starts[ply + 1] == "reused":
                    n_reused += 1
                    c = [int(a) for a in acts].index(g.chosen[ply])
                    assert g.searches[ply + 1].n_kept == int(vis[c])                      # the counted visits, not the pruned ones
    assert n_reused >= 10


def test_scenarios_and_hook_cases_reach_every_condition():
    hook, widths = collections.Counter(), set()
    for solver in (False, True):
        hc = FR.hook_cases(solver=solver)
        sel, frc, pruned, cst, cov = FR.hook_reference(hc)
        hook.update(cov)
        widths |= set(np.diff(hc.offsets).tolist())
        assert (hc.parent == 1).any() and (hc.P == 0.0).any() and (hc.P == 1.0).any() and (hc.K > 0).any()
        assert 0 < frc.sum() < len(frc) and (pruned <= hc.N).all() and (pruned < hc.N).any()
    assert set(FR.HOOK_K) <= widths and max(widths) == FR.MAX_MOVES
    assert hook["wide_case"] > 0 and hook["wide_pruned"] > 0 and hook["forced_win_skipped"] > 0
    played = _all_played()
    cov = FR.coverage(played, hook)
    print("coverage:", dict(cov))
    assert all(cov[k] >= 1 for k in FR.COVERAGE), dict(cov)
    games_alone = FR.coverage(played)                          # everything but K > 64 and the proven-WIN skip is reached by whole games as well
    assert all(games_alone[k] >= 1 for k in FR.COVERAGE if k not in ("wide_case", "forced_win_skipped")), dict(games_alone)
    # with and without leaf batching / the solver, each on its own
    for L, solver in FR.OPTIONS:
        c = FR.coverage([v for (_, l, sv), v in _played.items() if (l, sv) == (L, solver)])
        assert c["forced_selections"] > 0 and c["pruned_visits"] > 0 and c["forced_on_kept_root_at_begin"] > 0 and c["pruned_on_continued_ply"] > 0
        assert (c["forced_in_flight"] > 0) == (L > 1)
