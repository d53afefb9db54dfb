"""CPU checks of the restatement of sz_play_moves (tests/playmovesref.py): its re-rooting is reuseref's where both apply, a two-ply
re-rooting is one re-rooting at the grandchild, play_move keeps the game the host mirror plays, and the scenario list that
tests/test_gpu_play_moves.py runs on the device meets its coverage conditions on the restatement alone."""
import warnings

import numpy as np
import pytest

import playmovesref as P
import reuseref as R


@pytest.fixture(scope="module")
def played():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return [(sc, P.play(sc)) for sc in P.scenarios()]


def _same_tree(x, y):
    return all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(x, y))


def _same_store(x, y):
    n = x.n_edges
    return n == y.n_edges and sorted(x.games) == sorted(y.games) and all(
        getattr(x, k)[:n].tobytes() == getattr(y, k)[:n].tobytes() for k in ("W", "N", "P", "first", "n", "action", "term", "tval")) and all(
        R.position_record(x.games[e]) == R.position_record(y.games[e]) for e in x.games)


def test_scenarios_meet_the_coverage_conditions_on_the_restatement(played):
    c = P.coverage(played)
    print("coverage:", {k: (dict(v) if hasattr(v, "items") else v) for k, v in c.items()})
    P.assert_coverage(c)
    assert c["begin_fallbacks"]["nodes"] >= 1, "a kept subtree refused at search begin"
    for sc, games in played:
        for a, b in games:
            assert a.error is None and b.error is None
            assert R.position_record(a.game) == R.position_record(b.game) and (a.over, a.result) == (b.over, b.result)
            for g in (a, b):
                for (start, rerooted, had_kept), s in zip(g.begins, g.searches):
                    assert s.continued == (start == "reused") and s.sims == sc.S and len(s.games) <= 2 * sc.S + 2
                    assert rerooted in ((1, 2) if start == "reused" else (0, 1, 2))


def test_keep_is_reuserefs_reroot_where_that_one_keeps():
    """one ply: where reuseref.Search.reroot answers "reused", keep() gives the same store; where it answers "unvisited" or "leaf", the same name"""
    n = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for sc in P.scenarios()[:2]:
            for bd in sc.boards[:3]:
                g = P.new_games(sc, bd)[0]
                g.begin()
                s = g.run()
                acts, _ = s.root_children()
                for a in acts:
                    after = g.game.copy()
                    after.push_action(int(a))
                    want, reason = s.reroot(int(a), after)
                    got, mine = s.keep(int(a), after)
                    if reason == "reused":
                        assert mine == "kept" and _same_store(got, want) and got.fits() is None
                        n += 1
                    elif reason in ("nodes", "edges"):
                        assert mine == "kept" and got.fits() == reason
                    else:
                        assert got is None and mine == reason
    assert n >= 20


def test_two_re_rootings_are_one_re_rooting_at_the_grandchild(played):
    """the consistency check: a side that re-roots twice (play, then play_move) starts its next search with the grandchild's depth-first
    slice of the tree its own search ended with, and ends it with the tree that a single search continued from those kept statistics
    reaches: a Search built from that slice alone, replayed"""
    n = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for sc, games in played:
            if sc.ponder:
                continue
            for sides in games:
                for g in sides:
                    for i in range(1, len(g.searches)):
                        start, rerooted, _ = g.begins[i]
                        if start != "reused" or rerooted != 2:
                            continue
                        prev, s = g.searches[i - 1], g.searches[i]
                        a1 = g.chosen[i - 1] if len(g.chosen) >= i else None
                        d, a, v, w, p = prev.tree()
                        root_after = g.roots[i]
                        # the two moves between the searches, read off the games
                        k1 = [j for j in range(1, len(d)) if d[j] == 0 and a[j] == a1]
                        if a1 is None or not k1:
                            continue
                        k1 = k1[0]
                        end1 = next((j for j in range(k1 + 1, len(d)) if d[j] <= 0), len(d))
                        cands = [j for j in range(k1 + 1, end1) if d[j] == 1]
                        hit = None
                        for j in cands:
                            mid = g.roots[i - 1].copy()
                            mid.push_action(int(a1))
                            mid.push_action(int(a[j]))
                            if R.position_record(mid) == R.position_record(root_after):
                                hit = j
                        assert hit is not None
                        end2 = next((j for j in range(hit + 1, end1) if d[j] <= 1), end1)
                        mid = g.roots[i - 1].copy()
                        mid.push_action(int(a1))
                        once, _ = prev.keep(int(a1), mid)
                        twice, how = once.keep(int(a[hit]), root_after)
                        assert how == "kept"
                        fd, fa, fv, fw, fp = twice.tree()
                        assert (int(fv[0]), fw[0].tobytes(), fp[0].tobytes()) == (int(v[hit]), w[hit].tobytes(), p[hit].tobytes())
                        assert _same_tree((fd[1:], fa[1:], fv[1:], fw[1:], fp[1:]),
                                          (d[hit + 1:end2] - 2, a[hit + 1:end2], v[hit + 1:end2], w[hit + 1:end2], p[hit + 1:end2]))
                        twice.run()                          # the single continued search from the same kept statistics
                        assert _same_tree(twice.tree(), s.tree()) and _same_tree(twice.begin_tree, s.begin_tree)
                        assert len(twice.steps) == len(s.steps) and all(np.array_equal(x, y) for x, y in zip(twice.steps, s.steps))
                        n += 1
    assert n >= 30


def test_play_move_refuses_illegal_moves_and_moves_no_counter():
    sc = P.scenarios()[0]
    g = P.new_games(sc, sc.boards[0])[0]
    legal = [int(a) for a in g.game.legal_action_indices()]
    before = R.position_record(g.game)
    assert g.play_move(-1) is None and R.position_record(g.game) == before
    assert g.play_move(legal[0]) == "no_tree" and R.position_record(g.game) != before
    assert (g.simulations, g.expansions, g.terminal_hits) == (0, 0, 0) and not g.searches
    bad = next(a for a in range(4672) if a not in g.game.legal_action_indices())
    here = R.position_record(g.game)
    assert g.play_move(bad) == "invalid" and g.error == "invalid" and R.position_record(g.game) == here
    assert g.play_move(int(g.game.legal_action_indices()[0])) is None and R.position_record(g.game) == here      # sticky


def test_reuse_off_keeps_nothing(played):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sc = P.scenarios()[0]
        for a, b in P.play(sc._replace(plies=4), reuse=False):
            assert all(s == "new" for s in a.starts + b.starts) and not any(x.continued for x in a.searches + b.searches)
