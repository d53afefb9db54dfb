"""Proven-result propagation on the GPU (sz_set_solver, a NON-REFERENCE option): the HIP engine against the plain-Python restatement
tests/solverref.py, bit for bit (whole trees, proven labels, every network input, counters), sz_play on proven roots, budgets with
in-search shrinking, refusals, and one whole self-play game."""
import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
from hashmodel import HashModel, evaluate_packed, pack_planes
import reuseref
import solver_cases as SC
import solverref
import vlref
from solverref import UNKNOWN, WIN, DRAW, LOSS

pytestmark = pytest.mark.gpu


def _start(n):
    return sz.ChessTensor(chess960=True, scharnagl=n)


# what an engine fixes: (S, chess960) -> [(position, salt)]; the CPU case set plus the standard start and two Chess960 starts
def _groups():
    out = {}
    for name, S, salt in SC.CASES:
        out.setdefault((S, False), []).append((SC.game(name), salt))
    out[(64, False)].append((sz.ChessTensor(), 3))
    out[(200, False)].append((sz.ChessTensor(), 5))
    out[(64, True)] = [(_start(0), 4), (_start(959), 7)]
    assert all(len(v) <= 8 for v in out.values())
    return out


def _assert_tree(eng, b, r, tag):
    for x, y in zip(eng.debug_tree(b), r.tree()):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), tag
    pr, co = eng.debug_tree_proven(b)
    rp, rc = r.tree_proven()
    assert np.array_equal(pr, rp) and np.array_equal(co, rc), tag


def _engine_vs_ref(items, S, learning, c960):
    """one engine, board b = items[b]; every step: pending boards and network rows against the restatement; then trees, labels, counters"""
    refs = [solverref.search(ct, S, solver=True, learning=learning, mode="dyadic", salt=salt) for ct, salt in items]
    B = len(items)
    eng = SelfPlayEngine(None, {"C": 2, "num_searches": S, "solver": True}, B, chess960=c960, learning=learning)
    for b, (ct, _) in enumerate(items):
        eng.upload_game(b, ct)
    eng.begin()
    t = 0
    while True:
        torch.cuda.synchronize()
        pend = (eng.debug_pending()[4] & 2) != 0
        assert pend.tolist() == [t < len(r.steps) for r in refs], "step %d: boards waiting for the network" % t
        if not pend.any():
            break
        assert t < S
        planes = pack_planes(eng.planes.float().cpu().numpy())
        pol = np.zeros((B, N.SZ_ACTIONS), np.float32)
        val = np.zeros(B, np.float32)
        for b in np.nonzero(pend)[0]:
            want = refs[b].steps[t][0]
            assert np.array_equal(planes[b], want), "step %d board %d: network input differs" % (t, b)
            pol[b], val[b] = evaluate_packed(want, "dyadic", items[b][1])
        eng.step(torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda())
        t += 1
    st = eng.check_errors()
    assert st["boards_pending"] == 0 and st["boards_done"] == B
    for key, attr in (("simulations", "sims"), ("expansions", "expansions"), ("terminal_hits", "terminal_hits"), ("sum_depth", "sum_depth")):
        assert st[key] == sum(getattr(r, attr) for r in refs), key
    assert eng.solver_stats() == (sum(r.proven_stops for r in refs), sum(r.proved for r in refs))
    root, child = eng.root_proven()
    for b, r in enumerate(refs):
        tag = "board %d S=%d learning=%d" % (b, S, learning)
        _assert_tree(eng, b, r, tag)
        rr, rc = r.root_proven()
        assert int(root[b]) == rr and child[b, :len(rc)].tolist() == rc.tolist() and not child[b, len(rc):].any(), tag
    eng.close()
    return refs


# ------------------------------------------------------------------------------------------------ 1. engine == restatement
@pytest.mark.parametrize("learning", [False, True])
@pytest.mark.parametrize("S,c960", [(64, False), (200, False), (64, True)])
def test_trees_labels_inputs_and_counters_match_restatement(S, c960, learning):
    refs = _engine_vs_ref(_groups()[(S, c960)], S, learning, c960)
    if not c960:
        assert any(r.root_proven_at is not None for r in refs) and sum(r.proved for r in refs) > 0


# ------------------------------------------------------------------------------------------------ 2. off == never called
def test_solver_off_equals_no_call():
    items = [ct for its in _groups().values() for ct, _ in its if not ct.chess960][:8]
    trees = []
    for call in (False, True):
        eng = SelfPlayEngine(HashModel(salt=2), {"C": 2, "num_searches": 64}, len(items), learning=True)
        if call:
            N.check(N.lib().sz_set_solver(eng._e, 0, eng._stream()), "sz_set_solver")
        for b, ct in enumerate(items):
            eng.upload_game(b, ct)
        eng.search()
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(len(items))])
        assert all(not eng.debug_tree_proven(b)[0].any() and not eng.debug_tree_proven(b)[1].any() for b in range(len(items)))
        assert not eng.root_proven()[0].any() and eng.solver_stats() == (0, 0)
        eng.close()
    for b, ct in enumerate(items):
        for x, y in zip(trees[0][b], trees[1][b]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "board %d" % b
        for x, y in zip(trees[0][b], vlref.search(ct, 64, learning=True, L=1, mode="dyadic", salt=2).tree()):
            assert x.tobytes() == y.tobytes(), "board %d" % b


# ------------------------------------------------------------------------------------------------ 3. sz_play on proven roots
def test_play_on_proven_roots():
    names = ["mate_in_1", "forced_draw", "mated_in_2", "refuted_move"]
    games = [SC.game(n) for n in names]
    refs = [solverref.search(g, 200, solver=True, learning=False, mode="dyadic", salt=0) for g in games]
    assert [r.root_proven()[0] for r in refs] == [WIN, DRAW, LOSS, UNKNOWN]
    win = int(np.nonzero(refs[0].root_proven()[1] == LOSS)[0][0])
    # uniforms that sample another move than the proving one on the WIN root (non-negative), and arbitrary ones elsewhere
    u = [next(x for x in (0.05, 0.35, 0.65, 0.95) if reuseref.choose(refs[0].root_children()[1], x) != win), 0.5, 0.7, 0.3]
    for uniforms in (u, [-1.0] * 4):
        eng = SelfPlayEngine(HashModel(salt=0), {"C": 2, "num_searches": 200, "solver": True}, 4, learning=False)
        for b, g in enumerate(games):
            eng.upload_game(b, g)
        eng.search()
        eng.check_errors()
        assert eng.root_proven()[0].tolist() == [WIN, DRAW, LOSS, UNKNOWN]
        eng.play(uniforms)
        rec = eng.fetch_ply()
        eng.check_errors()
        for b, r in enumerate(refs):
            acts, vis = r.root_children()
            k = len(acts)
            assert int(rec["n_child"][b]) == k and rec["action"][b, :k].tolist() == acts.tolist() and rec["visits"][b, :k].tolist() == vis.tolist()
            plain = reuseref.choose(vis, uniforms[b])                 # the move the solver-off rule samples from the same visits
            want = win if b == 0 else plain
            assert r.choose(uniforms[b]) == want
            assert int(rec["chosen"][b]) == int(acts[want]), "board %d" % b
            g = games[b].copy()
            g.push_action(int(acts[want]))
            pos, ply = eng.debug_position(b)
            assert pos.tobytes() == reuseref.position_record(g), "board %d" % b
            assert bool(rec["game_over"][b]) == g.get_value_and_terminated()[1]
        assert rec["game_over"][0] == 1 and rec["result"][0] == 1     # Ra8#
        if uniforms[0] >= 0:
            assert int(rec["chosen"][0]) != int(refs[0].root_children()[0][reuseref.choose(refs[0].root_children()[1], uniforms[0])])
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. budgets and in-search shrinking
@pytest.mark.parametrize("max_shrinks", [3, 0])
def test_with_budgets_and_shrinking(max_shrinks):
    names = ["mate_in_1", "moves_218", "forced_draw", "mated_in_2", "refuted_move", "mate_in_1", "mated_in_2", "forced_draw"]
    budgets = [200, 64, 0, 120, 200, 1, 64, 17]
    games = [SC.game(n) for n in names]
    eng = SelfPlayEngine(HashModel(salt=0), {"C": 2, "num_searches": 200, "solver": True, "max_shrinks": max_shrinks}, 8, learning=False)
    for b, g in enumerate(games):
        eng.upload_game(b, g)
    eng.set_budgets(budgets)
    eng.search()
    st = eng.check_errors()
    refs = [solverref.search(g, s, solver=True, learning=False, mode="dyadic", salt=0) for g, s in zip(games, budgets)]
    assert refs[0].root_proven_at < 64 and refs[3].root_proven_at < 120      # roots proven long before their budgets were counted out
    assert st["simulations"] == sum(budgets) and st["boards_done"] == 8 and st["boards_pending"] == 0
    assert st["terminal_hits"] == sum(r.terminal_hits for r in refs) and st["sum_depth"] == sum(r.sum_depth for r in refs)
    assert eng.solver_stats() == (sum(r.proven_stops for r in refs), sum(r.proved for r in refs))
    for b, r in enumerate(refs):
        _assert_tree(eng, b, r, "board %d budget %d" % (b, budgets[b]))
        assert int(eng.debug_tree(b)[2][0]) == 1 + budgets[b]
    if max_shrinks:
        assert eng.last_rows < eng.last_steps * 8                 # the batch shrank as boards finished
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals():
    lib = N.lib()
    ct = SC.game("mated_in_2")
    want = solverref.search(ct, 64, solver=True, learning=False, mode="dyadic", salt=0)
    eng = SelfPlayEngine(HashModel(salt=0), {"C": 2, "num_searches": 64, "solver": True}, 1, learning=False)
    s = eng._stream()
    assert lib.sz_set_leaf_batching(eng._e, 2, 1.0, s) == N.SZ_ERR_INVALID       # L > 1 while the solver is on
    assert lib.sz_set_leaf_batching(eng._e, 1, 1.0, s) == N.SZ_OK
    eng.upload_game(0, ct)
    eng.begin()
    assert lib.sz_set_solver(eng._e, 0, s) == N.SZ_ERR_STATE                     # in the middle of a search
    assert lib.sz_set_solver(eng._e, 1, s) == N.SZ_ERR_STATE
    for _ in range(64):
        eng.step(*eng.evaluate(eng.planes))
    eng.check_errors()
    _assert_tree(eng, 0, want, "after refused calls")
    assert lib.sz_set_solver(eng._e, 0, s) == N.SZ_OK                            # between searches: off, and the plain search runs
    eng.upload_game(0, ct)
    eng.search()
    eng.check_errors()
    _assert_tree(eng, 0, solverref.search(ct, 64, solver=False, learning=False, mode="dyadic", salt=0), "switched off")
    eng.close()
    # the other order: leaf batching first
    vl = SelfPlayEngine(HashModel(salt=0), {"C": 2, "num_searches": 64, "leaves_per_step": 2}, 1, learning=False)
    assert lib.sz_set_solver(vl._e, 1, vl._stream()) == N.SZ_ERR_INVALID
    assert lib.sz_set_solver(vl._e, 0, vl._stream()) == N.SZ_OK
    vl.upload_game(0, ct)
    vl.search()
    vl.check_errors()
    for x, y in zip(vl.debug_tree(0), vlref.search(ct, 64, learning=False, L=2, lam=1.0, mode="dyadic", salt=0).tree()):
        assert x.tobytes() == y.tobytes()
    assert not vl.debug_tree_proven(0)[0].any()
    vl.close()
    reuse = SelfPlayEngine(None, {"C": 2, "num_searches": 8, "reuse_subtree": True}, 1, learning=False)
    assert lib.sz_set_solver(reuse._e, 1, reuse._stream()) == N.SZ_ERR_INVALID
    assert lib.sz_set_solver(reuse._e, 0, reuse._stream()) == N.SZ_OK
    reuse.close()
    for bad in ({"solver": 1}, {"solver": "yes"}, {"solver": True, "reuse_subtree": True}, {"solver": True, "leaves_per_step": 2}):
        with pytest.raises(ValueError):
            SelfPlayEngine(None, dict({"C": 2, "num_searches": 8}, **bad), 1)


# ------------------------------------------------------------------------------------------------ 6. a whole game
def test_whole_game_from_a_sparse_endgame():
    S, salt, max_plies = 64, 1, 60
    u = lambda ply: ((ply * 104729 + 12345) % 997) / 997.0
    game = SC.game("endgame_6_men")
    eng = SelfPlayEngine(HashModel(salt=salt), {"C": 2, "num_searches": S, "solver": True}, 1, learning=True)
    eng.upload_game(0, game)
    proven_roots = overrides = 0
    for ply in range(max_plies):
        r = solverref.search(game, S, solver=True, learning=True, mode="dyadic", salt=salt)
        eng.search()
        eng.check_errors()
        root = int(eng.root_proven()[0][0])
        eng.play([u(ply)])
        rec = eng.fetch_ply()
        eng.check_errors()
        acts, vis = r.root_children()
        k, c = len(acts), r.choose(u(ply))
        tag = "ply %d" % ply
        assert int(rec["n_child"][0]) == k and rec["action"][0, :k].tolist() == acts.tolist() and rec["visits"][0, :k].tolist() == vis.tolist(), tag
        assert int(rec["chosen"][0]) == int(acts[c]) and root == r.root_proven()[0], tag
        assert np.array_equal(rec["packed"][0], r.steps[0][0]) and bool(rec["colour"][0]) == bool(game.board.turn), tag
        proven_roots += 1 if r.root_proven()[0] else 0
        overrides += 1 if c != reuseref.choose(vis, u(ply)) else 0
        game.push_action(int(acts[c]))
        over = game.get_value_and_terminated()[1]
        assert bool(rec["game_over"][0]) == over, tag
        assert eng.debug_position(0)[0].tobytes() == reuseref.position_record(game), tag
        if over:
            assert int(rec["result"][0]) == {"1-0": 1, "0-1": -1}.get(game.board.result(), 0)
            break
    assert proven_roots >= 1
    eng.close()
