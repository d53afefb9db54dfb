"""The combined restatement tests/composeref.py (leaf batching + solver + subtree reuse in one search) on the CPU: it reduces to each
single-option restatement bit for bit, its finished trees are fixpoints of the solver's rules, no descent stays in flight at a search
end, and the case sets tests/test_gpu_compose.py runs on the device reach every event they are there for."""
import collections
import warnings

import numpy as np
import pytest

import composeref as CR
import reuseref
import solver_cases as SC
import solverref
import vlref


def _same_tree(a, b, tag):
    for x, y in zip(a.tree(), b.tree()):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), tag


def _same_steps(a, b, tag):
    assert len(a.steps) == len(b.steps) and all(np.array_equal(x, y) for x, y in zip(a.steps, b.steps)), tag


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("L", [1, 2, 7])
def test_reduces_to_vlref_without_solver_and_reuse(L):
    for name, S, salt in SC.CASES[:5] + [("endgame_6_men", 64, 1)]:
        for learning in (False, True):
            kw = dict(learning=learning, L=L, lam=0.5, mode="dyadic", salt=salt)
            a, b = CR.search(SC.game(name), min(S, 96), **kw), vlref.search(SC.game(name), min(S, 96), **kw)
            tag = "%s L=%d learning=%d" % (name, L, learning)
            _same_tree(a, b, tag)
            _same_steps(a, b, tag)
            assert a.collisions == b.collisions and not a.R.any() and not a.complete.any(), tag


@pytest.mark.parametrize("name,S,salt", SC.CASES)
def test_reduces_to_solverref_at_L1(name, S, salt):
    for learning in (False, True):
        a = CR.search(SC.game(name), S, L=1, solver=True, learning=learning, mode="dyadic", salt=salt)
        b = solverref.search(SC.game(name), S, solver=True, learning=learning, mode="dyadic", salt=salt)
        tag = "%s S=%d learning=%d" % (name, S, learning)
        _same_tree(a, b, tag)
        _same_steps(a, b, tag)
        assert all(np.array_equal(x, y) for x, y in zip(a.tree_proven(), b.tree_proven())), tag
        for k in ("sims", "expansions", "terminal_hits", "sum_depth", "proven_stops", "proved", "skips", "root_proven_at"):
            assert getattr(a, k) == getattr(b, k), (tag, k)


def test_reduces_to_reuseref_at_L1_without_solver():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for sc in reuseref.scenarios():
            want = reuseref.play(sc)
            for bd, w in zip(sc.boards, want):
                g = CR.Game(bd.make(), sc.S, sc.edges_per_board, reuse=True, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt)
                for ply in range(sc.plies):
                    if g.live:
                        g.begin()
                        g.run()
                        if g.error is None:
                            g.play(bd.u(ply))
                tag = "%s %s" % (sc.name, bd.name)
                assert g.starts == w.starts and g.chosen == w.chosen and g.error == w.error and g.last_fallback == w.last_fallback, tag
                assert (g.simulations, g.expansions, g.terminal_hits) == (w.simulations, w.expansions, w.terminal_hits) or g.error, tag
                for a, b in zip(g.searches, w.searches):
                    _same_tree(a, b, tag)
                    _same_steps(a, b, tag)
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.begin_tree, b.begin_tree)), tag


# ------------------------------------------------------------------------------------------------ the GPU case sets, on the restatement
def test_solver_times_L_cases_are_fixpoints_and_reach_their_events():
    cov, widest = collections.Counter(), 0
    for (S, c960), items in CR.solver_items().items():
        for L in CR.L_VALUES:
            for learning in (False, True):
                for (name, _, _), r in zip(items, CR.solver_refs(S, c960, L, learning)):
                    tag = "%s S=%d L=%d learning=%d" % (name, S, L, learning)
                    SC.check_fixpoint(r, tag)                  # run() has asserted that no descent is in flight
                    assert r.sims == S and r.expansions + r.terminal_hits == S, tag
                    cov.update(r.cov)
                    if name == "moves_218" and L == 32:
                        widest = max(widest, int(r.n[0]))
    print("coverage:", dict(cov))
    assert all(cov[k] >= 1 for k in CR.SOLVER_COVERAGE), dict(cov)
    assert widest > 192                                         # the root's children span four 64-lane passes (218 legal moves, a few dropped for a zero prior)


_played = {}                                                # (L, solver) -> [Game] over all game cases


def _play_all(L, solver):
    if (L, solver) not in _played:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[(L, solver)] = [g for gc in CR.game_cases() for g in CR.play(gc, L, solver)]
    return _played[(L, solver)]


@pytest.mark.parametrize("L,solver", CR.GAME_OPTIONS)
def test_whole_game_cases_end_every_search_with_nothing_in_flight(L, solver):
    for g in _play_all(L, solver):
        assert len(g.starts) <= 60
        for s in g.searches:
            if s.error is None:
                assert not s.K[:s.n_edges].any()
                if solver:
                    SC.check_fixpoint(s, "L=%d" % L)


def test_whole_game_cases_reach_their_events():
    cov, fb = collections.Counter(), collections.Counter()
    for L, solver in CR.GAME_OPTIONS:
        if L > 1 or solver:                                     # L = 1 without the solver is subtree reuse alone: it proves nothing new
            for g in _play_all(L, solver):
                cov.update(g.cov)
                fb.update(g.fallbacks())
    print("coverage:", dict(cov), dict(fb))
    assert all(cov[k] >= 1 for k in CR.GAME_COVERAGE), dict(cov)
    # the three fresh-start conditions of sz_config.reuse_subtree: (1) never visited / a leaf, (2) too many nodes, (3) too many edges
    assert fb["unvisited"] >= 1 and fb["leaf"] >= 1 and fb["nodes"] >= 1 and fb["edges"] >= 1, dict(fb)


def test_setting_change_drops_the_kept_subtree_and_no_change_keeps_it():
    gc = CR.game_cases()[0]
    bd = gc.boards[0]
    g = CR.new_game(gc, bd, 1, False)
    plan = {2: (4, 1.0, False), 3: (4, 0.5, False), 4: (4, 0.5, True), 6: (1, 0.5, True), 7: (1, 0.5, True)}
    for ply in range(9):
        if ply in plan:
            g.set_options(*plan[ply])
        g.begin()
        g.run()
        g.play(bd.u(ply))
    assert [g.starts[p] for p in (2, 4, 6)] == ["dropped"] * 3 and g.starts[3] == "reused" and g.starts[7] == "reused", g.starts
    assert all(s.N[0] == 1 + gc.S for p, s in enumerate(g.searches) if g.starts[p] in ("new", "dropped"))
