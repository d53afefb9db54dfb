"""CPU checks of the subtree-reuse restatement (tests/reuseref.py; sz_config.reuse_subtree, a NON-REFERENCE option): with the option off
it adds nothing to the reference's search, re-rooting keeps exactly the chosen child's subtree with the right positions, and the
scenario list that tests/test_gpu_subtree_reuse.py runs on the device meets its coverage conditions on the restatement alone."""
import warnings

import numpy as np
import pytest

import reuseref as R
import vlref


@pytest.fixture(scope="module")
def played():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # a policy that is 0 on every legal move: priors are NaN, as in the reference
        return [(sc, R.play(sc)) for sc in R.scenarios()]


def _same_tree(x, y):
    return all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(x, y))


def test_choose_is_numpys_choice():
    """the move choice against np.random.choice itself, driven by the uniform it would draw"""
    rng = np.random.RandomState(11)
    for _ in range(300):
        vis = rng.randint(0, 9, size=rng.randint(1, 40))
        if vis.sum() == 0:
            continue
        seed = int(rng.randint(1 << 30))
        u = np.random.RandomState(seed).random_sample()
        want = int(np.random.RandomState(seed).choice(len(vis), p=vis / vis.sum()))
        assert R.choose(vis, u) == want
    assert R.choose([0, 3, 7, 7, 1], -1.0) == 2 and R.choose([5, 0, 0], 1.0) == 2 and R.choose([5, 0, 0], 0.999) == 0


def test_reuse_off_is_a_fresh_reference_search_every_ply():
    """with reuse off a multi-ply game of the restatement is ply-by-ply vlref.search: same network inputs, same trees"""
    for sc in R.scenarios()[:3]:
        for bd in sc.boards[:3]:
            g = R.new_game(sc, bd, reuse=False)
            for ply in range(4):
                if not g.live:
                    break
                before = g.game.copy()
                g.begin()
                s = g.run()
                want = vlref.search(before, sc.S, c=2.0, learning=sc.learning, L=1, mode=bd.mode, salt=bd.salt)
                assert g.starts[-1] == "new" and not s.continued
                assert _same_tree(s.tree(), want.tree()), (sc.name, bd.name, ply)
                assert len(s.steps) == len(want.steps) and all(np.array_equal(a, b) for a, b in zip(s.steps, want.steps))
                assert (s.sims, s.expansions + s.terminal_hits) == (want.sims, want.sims)
                g.play(bd.u(ply))


def test_reroot_keeps_the_chosen_subtree_and_its_positions(played):
    """after reroot tree() is the depth-first slice of the previous tree below the chosen child, and the game of every kept edge is the
    position reached by replaying its actions from the new root"""
    n = 0
    for sc, games in played:
        for g in games:
            for ply in range(1, len(g.starts)):
                prev, s = g.searches[ply - 1], g.searches[ply]
                if g.starts[ply] != "reused":
                    assert not s.continued and s.kept_edges == 0
                    continue
                d, a, v, w, p = prev.tree()
                tops = [i for i in range(1, len(d)) if d[i] == 0]
                chosen = g.chosen[ply - 1]
                k0 = next(i for i in tops if a[i] == chosen)
                k1 = next((i for i in tops if i > k0), len(d))
                fresh = prev.reroot(chosen, g.roots[ply])[0]             # s itself has been searched on since: re-root once more
                fd, fa, fv, fw, fp = fresh.tree()
                assert (int(fv[0]), fw[0].tobytes(), fp[0].tobytes()) == (int(v[k0]), w[k0].tobytes(), p[k0].tobytes())
                assert _same_tree((fd[1:], fa[1:], fv[1:], fw[1:], fp[1:]), (d[k0 + 1:k1] - 1, a[k0 + 1:k1], v[k0 + 1:k1], w[k0 + 1:k1], p[k0 + 1:k1]))
                assert fresh.kept_edges == k1 - k0 == s.kept_edges and fresh.kept_nodes == s.kept_nodes == len(fresh.games) <= sc.S
                # positions: replay from the new root (the board's own game after the move)
                root = g.roots[ply]
                assert R.position_record(fresh.games[0]) == R.position_record(root)
                stack = [(0, root)]
                while stack:
                    e, pos = stack.pop()
                    assert R.position_record(fresh.games[e]) == R.position_record(pos)
                    assert np.array_equal(fresh.games[e].get_representation().numpy(), pos.get_representation().numpy())
                    v_, t_ = pos.get_value_and_terminated()
                    assert (int(fresh.term[e]), int(fresh.tval[e])) == (int(t_), int(v_) if t_ else 0) or e == 0
                    for j in range(int(fresh.n[e])):
                        c = int(fresh.first[e]) + j
                        if c in fresh.games:
                            child = pos.copy()
                            child.push_action(int(fresh.action[c]))
                            stack.append((c, child))
                n += 1
    assert n >= 100


def test_scenarios_meet_the_coverage_conditions_on_the_restatement(played):
    """the inputs of the GPU module were chosen so that the restatement reaches every branch and stays within the caps"""
    c = R.coverage(played)
    print("coverage:", {k: (dict(v) if hasattr(v, "items") else v) for k, v in c.items()})
    R.assert_coverage(c)
    for sc, games in played:
        for g, bd in zip(games, sc.boards):
            assert (g.error == "capacity") == sc.name.startswith("overflow"), (sc.name, bd.name)
            assert len(g.starts) == sc.plies or g.over or g.error, (sc.name, bd.name)
            for start, s in zip(g.starts, g.searches):
                assert s.continued == (start == "reused")
                if s.error is None:
                    assert s.sims == sc.S and s.n_edges <= s.e_cap and len(s.games) <= 2 * sc.S + 2
    by_name = {sc.name: games for sc, games in played}
    assert any("nodes" in g.starts for g in by_name["peaked"]) and any("edges" in g.starts for g in by_name["few_edges"])
    assert any("unvisited" in g.starts for g in by_name["last_child"])
    assert by_name["overflow_continued"][0].starts == ["new", "reused"]            # the search that overflows continues on a kept subtree
