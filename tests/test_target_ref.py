"""The restatement tests/targetref.py (visit targets, root noise at every search, quiet boards: subtree reuse as a self-play configuration)
on the CPU: with the options off it is composeref bit for bit, and hence reuseref and vlref; on a game without reuse a target is vlref's
search with S = t; after every search the root holds max(N_kept, 1 + t) visits and the new simulations add up to the goals; and the
scenarios tests/test_gpu_visit_targets.py runs on the device reach every condition they are there for."""
import warnings

import numpy as np
import pytest

import composeref as CR
import reuseref
import targetref as TR
import vlref


def _same_tree(a, b, tag):
    for x, y in zip(a.tree(), b.tree()):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), tag


def _same_steps(a, b, tag):
    assert len(a.steps) == len(b.steps) and all(np.array_equal(x, y) for x, y in zip(a.steps, b.steps)), tag


_played = {}


def _play(name, L, solver):
    if (name, L, solver) not in _played:
        sc = next(s for s in TR.scenarios() if s.name == name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[(name, L, solver)] = (sc, TR.play(sc, L, solver))
    return _played[(name, L, solver)]


def _all_played():
    return [_play(sc.name, L, solver) for sc in TR.scenarios() for L, solver in TR.OPTIONS]


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("L,solver", [(1, False), (4, True)])
def test_is_composeref_with_targets_off_and_no_gamma(L, solver):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for gc in CR.game_cases()[1:3]:
            gc = gc._replace(plies=min(gc.plies, 5), boards=gc.boards[:3])
            want = CR.play(gc, L, solver)
            for bd, w in zip(gc.boards, want):
                g = TR.Game(bd.make(), gc.S, gc.edges_per_board, reuse=True, L=L, lam=1.0, solver=solver, c=2.0, learning=gc.learning, mode=bd.mode, salt=bd.salt)
                for ply in range(gc.plies):
                    if g.live:
                        g.begin()
                        g.run()
                        if g.error is None:
                            g.play(bd.u(ply))
                tag = "%s %s L=%d solver=%d" % (gc.name, bd.name, L, solver)
                assert g.starts == w.starts and g.chosen == w.chosen and g.error == w.error, tag
                assert all(getattr(g, k) == getattr(w, k) for k in CR.Game.COUNTERS), tag
                assert g.goals == [gc.S] * len(g.goals), tag
                for a, b in zip(g.searches, w.searches):
                    _same_tree(a, b, tag)
                    _same_steps(a, b, tag)
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.begin_tree, b.begin_tree)), tag
                    assert all(np.array_equal(x, y) for x, y in zip(a.tree_proven(), b.tree_proven())), tag


def test_is_reuseref_with_targets_off_and_no_gamma():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for sc in reuseref.scenarios()[:2]:
            sc = sc._replace(plies=4)
            for bd, w in list(zip(sc.boards, reuseref.play(sc)))[:3]:
                g = TR.Game(bd.make(), sc.S, sc.edges_per_board, reuse=True, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt)
                for ply in range(sc.plies):
                    if g.live:
                        g.begin()
                        g.run()
                        g.play(bd.u(ply))
                tag = "%s %s" % (sc.name, bd.name)
                assert g.starts == w.starts and g.chosen == w.chosen, tag
                for a, b in zip(g.searches, w.searches):
                    _same_tree(a, b, tag)
                    _same_steps(a, b, tag)


@pytest.mark.parametrize("t", [0, 1, 2, 8, 33, 64])
def test_a_target_without_reuse_is_vlref_with_S_equal_t(t):
    """every search of a game without reuse starts from a fresh root: goal = t, exactly a budget of t"""
    sc = next(s for s in TR.scenarios() if s.name == "plain_targets")
    for L in (1, 4):
        for bd in sc.boards:
            for learning in (False, True):
                g = TR.Game(bd.make(), sc.S, None, reuse=False, L=L, lam=1.0, solver=False, c=2.0, learning=learning, mode=bd.mode, salt=bd.salt)
                for ply in range(3):
                    s = g.begin(t)
                    g.run()
                    w = vlref.search(g.game, t, c=2.0, learning=learning, L=L, lam=1.0, mode=bd.mode, salt=bd.salt)
                    tag = "%s t=%d L=%d ply %d" % (bd.name, t, L, ply)
                    assert g.goals[-1] == t and s.sims == t and int(s.N[0]) == 1 + t, tag
                    _same_tree(s, w, tag)
                    _same_steps(s, w, tag)
                    if t < 2:
                        break                                   # nothing to sample a move from (SZ_ERR_ZERO_VISITS)
                    g.play(bd.u(ply))


# ------------------------------------------------------------------------------------------------ the root mix
def test_gamma_sum_is_the_lane_strided_butterfly_order():
    g = TR.gammas(TR.scenarios()[0])[0, 0]
    for k in (1, 20, 64, 65, 130, 218):
        lanes = [np.float32(0)] * 64
        for c in range(k):
            lanes[c % 64] = np.float32(lanes[c % 64] + g[c])
        for off in (32, 16, 8, 4, 2, 1):
            lanes = [np.float32(lanes[i] + lanes[i ^ off]) for i in range(64)]
        assert TR.gamma_sum(g, k).tobytes() == lanes[0].tobytes(), k
    assert any(TR.gamma_sum(g, k) != np.float32(np.sum(g[:k].astype(np.float64))) for k in (65, 130, 218)), "the draws are not dyadic: the order matters"


def test_fresh_root_mix_is_root_only_and_quiet_leaves_priors_clean():
    sc = next(s for s in TR.scenarios() if s.name == "c960_noise")
    bd, gam = sc.boards[0], TR.gammas(sc)[0, 0]
    run = lambda gamma, quiet, learning=True: TR.Search(bd.make(), 64, c=2.0, learning=learning, mode=bd.mode, salt=bd.salt)
    clean, noisy, quiet = run(None, 0, False), run(gam, 0), run(gam, 1)
    clean.begin(16); noisy.begin(16, gam, False); quiet.begin(16, gam, True)
    for s in (clean, noisy, quiet):
        s.run()
    _same_tree(quiet, clean, "a quiet board under root noise has the priors of a search without learning")
    f, k = int(noisy.first[0]), int(noisy.n[0])
    first = TR.Search(bd.make(), 64, c=2.0, learning=False, mode=bd.mode, salt=bd.salt)
    first.begin(1)
    first.run()                                                 # one simulation: the root's expansion, clean priors
    assert noisy.P[f:f + k].tobytes() == TR.root_mix(first.P[f:f + k], gam).tobytes()
    assert abs(float(noisy.P[f:f + k].astype(np.float64).sum()) - 1.0) < 1e-5


# ------------------------------------------------------------------------------------------------ invariants over the GPU scenarios
@pytest.mark.parametrize("L,solver", TR.OPTIONS)
@pytest.mark.parametrize("name", [sc.name for sc in TR.scenarios()])
def test_root_visits_and_simulations_follow_the_goals(name, L, solver):
    sc, games = _play(name, L, solver)
    for bd, g in zip(sc.boards, games):
        assert g.error is None and len(g.starts) >= 1
        for ply, s in enumerate(g.searches):
            t, tag = bd.targets[ply], "%s %s ply %d (%s)" % (name, bd.name, ply, g.starts[ply])
            assert int(s.N[0]) == max(g.kept_visits[ply], 1 + t), tag
            assert s.sims == g.goals[ply] == (max(0, t + 1 - g.kept_visits[ply]) if g.starts[ply] == "reused" else t), tag
            assert (g.kept_visits[ply] == 1) == (g.starts[ply] != "reused") or g.starts[ply] == "reused", tag
            if g.starts[ply] == "reused" and g.goals[ply] == 0:
                assert not s.steps and all(x.tobytes() == y.tobytes() for x, y in zip(s.begin_tree, s.tree())), tag + ": done at begin, no network row"
        assert g.simulations == sum(g.goals)


def test_noise_mode_switch_drops_and_pointer_or_quiet_changes_keep():
    sc, games = _play("noise_switch", 1, False)
    for g in games:
        assert [g.starts[p] for p in (3, 6)] == ["dropped", "dropped"] and all(g.starts[p] == "reused" for p in (1, 2, 4, 5, 7)), g.starts
        assert g.goals[3] == sc.boards[games.index(g)].targets[3]      # a dropped board searches its whole target
    sc, games = _play("c960_noise", 1, False)                           # new draws and other quiet flags at every ply: nothing dropped
    assert not any("dropped" in g.starts for g in games)


def test_scenarios_reach_every_condition():
    cov = TR.coverage(_all_played())
    print("coverage:", dict(cov))
    assert all(cov[k] >= 1 for k in TR.COVERAGE), dict(cov)
    for L, solver in TR.OPTIONS:                                         # ... under each option combination on its own
        c = TR.coverage([_play(sc.name, L, solver) for sc in TR.scenarios()])
        assert all(c[k] >= 1 for k in TR.COVERAGE), (L, solver, dict(c))
