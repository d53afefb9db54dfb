"""Leaf batching, the solver and subtree reuse in ONE search on the GPU (sz_set_search_options / args["combine_options"], NON-REFERENCE
options): the HIP engine against the plain-Python restatement tests/composeref.py, bit for bit — whole trees, proven labels and `complete`
bits, every network input row of every step, the boards pending per step, step counts, counters, training records — plus budgets with
in-search shrinking, setting changes on a reuse engine, refusals and the Python surface.  tests/test_compose_ref.py proves on the CPU that
the case sets reach the events they are there for; the same counters are asserted here on the games the device was compared with."""
import collections
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
from hashmodel import HashModel, evaluate_packed, pack_planes
import composeref as CR
import solver_cases as SC
from solverref import UNKNOWN, WIN, DRAW, LOSS

pytestmark = pytest.mark.gpu

ST_PENDING, ST_ERROR = 2, 16
ALL = {"combine_options": True}


def _assert_tree(tag, eng, b, tree, proven):
    for x, y in zip(eng.debug_tree(b), tree):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: tree differs" % tag
    pr, co = eng.debug_tree_proven(b)
    assert np.array_equal(pr, proven[0]) and np.array_equal(co, proven[1]), "%s: proven labels / complete bits differ" % tag


def _options(eng, L, lam, solver):
    opt = N.sz_search_options(L, lam, int(solver))
    return N.lib().sz_set_search_options(eng._e, C.byref(opt), eng._stream())


def _steps(eng, searches, live, modes, tag, S):
    """the steps of one search on every live board b against searches[b]: boards pending, network rows, step count"""
    B, L = eng.B, eng.L
    t = 0
    while True:
        torch.cuda.synchronize()
        status = eng.debug_pending()[4]
        pend = (status & ST_PENDING) != 0
        want = [bool(live[b]) and t < len(s.steps) for b, s in enumerate(searches)]
        assert pend.tolist() == want, "%s step %d: boards waiting for the network %s, restatement %s" % (tag, t, pend.tolist(), want)
        if not pend.any():
            return t
        assert t < S
        planes = pack_planes(eng.planes.float().cpu().numpy())
        pol = np.zeros((B * L, N.SZ_ACTIONS), np.float32)
        val = np.zeros(B * L, np.float32)
        for b in np.nonzero(pend)[0]:
            rows = searches[b].steps[t]
            assert np.array_equal(planes[b * L:b * L + len(rows)], rows), "%s step %d board %d: network input rows differ" % (tag, t, b)
            for i in range(len(rows)):
                pol[b * L + i], val[b * L + i] = evaluate_packed(rows[i], *modes[b])
        eng.step(torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda())
        t += 1


# ------------------------------------------------------------------------------------------------ 1. solver x L
_solver_cov = collections.Counter()


@pytest.mark.parametrize("learning", [False, True])
@pytest.mark.parametrize("L", CR.L_VALUES)
@pytest.mark.parametrize("S,c960", [(64, False), (200, False), (64, True)])
def test_solver_with_leaf_batching_matches_restatement(S, c960, L, learning):
    items = CR.solver_items()[(S, c960)]
    refs = CR.solver_refs(S, c960, L, learning)
    B = len(items)
    eng = SelfPlayEngine(None, dict(ALL, C=2, num_searches=S, solver=True, leaves_per_step=L), B, chess960=c960, learning=learning)
    for b, (_, ct, _) in enumerate(items):
        eng.upload_game(b, ct)
    eng.begin()
    tag = "S=%d L=%d learning=%d" % (S, L, learning)
    t = _steps(eng, refs, [True] * B, [("dyadic", salt) for _, _, salt in items], tag, S)
    assert t == max(len(r.steps) for r in refs)
    st = eng.check_errors()
    assert st["boards_pending"] == 0 and st["boards_done"] == B
    for key, attr in (("simulations", "sims"), ("expansions", "expansions"), ("terminal_hits", "terminal_hits"), ("sum_depth", "sum_depth")):
        assert st[key] == sum(getattr(r, attr) for r in refs), key
    assert eng.solver_stats() == (sum(r.proven_stops for r in refs), sum(r.proved for r in refs))
    root, child = eng.root_proven()
    for b, r in enumerate(refs):
        _assert_tree("%s board %d (%s)" % (tag, b, items[b][0]), eng, b, r.tree(), r.tree_proven())
        rr, rc = r.root_proven()
        assert int(root[b]) == rr and child[b, :len(rc)].tolist() == rc.tolist() and not child[b, len(rc):].any(), tag
        _solver_cov.update(r.cov)
        if items[b][0] == "moves_218" and L == 32:
            _solver_cov["moves_218_at_L32"] += int(r.n[0]) > 192
    eng.close()


def test_solver_with_leaf_batching_coverage():
    """counted on the restatement, over the cases the device was compared with (all of them replayed when this test runs alone)"""
    if not _solver_cov:
        for (S, c960) in CR.solver_items():
            for L in CR.L_VALUES:
                for learning in (False, True):
                    for (name, _, _), r in zip(CR.solver_items()[(S, c960)], CR.solver_refs(S, c960, L, learning)):
                        _solver_cov.update(r.cov)
                        if name == "moves_218" and L == 32:
                            _solver_cov["moves_218_at_L32"] += int(r.n[0]) > 192
    print("coverage:", dict(_solver_cov))
    assert all(_solver_cov[k] >= 1 for k in CR.SOLVER_COVERAGE + ("moves_218_at_L32",)), dict(_solver_cov)


# ------------------------------------------------------------------------------------------------ 2. whole games with reuse
_game_cov, _game_fb = collections.Counter(), collections.Counter()


def _drive_games(gc, L, solver, plan=None, reuse=True, lam=1.0):
    """one reuse engine, board b = gc.boards[b], ply after ply in lock-step with the restatement; plan: {ply: (L, lam, solver)} setting
    changes made before that ply's search.  -> the restatement's games"""
    B = len(gc.boards)
    args = dict(ALL, C=2, num_searches=gc.S, solver=solver, leaves_per_step=L, virtual_loss=lam)
    if reuse:
        args["reuse_subtree"] = True
    eng = SelfPlayEngine(None, args, B, chess960=gc.c960, learning=gc.learning, edges_per_board=gc.edges_per_board)
    games = [CR.new_game(gc, bd, L, solver, reuse, lam) for bd in gc.boards]
    modes = [(bd.mode, bd.salt) for bd in gc.boards]
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(gc.plies):
            if plan and ply in plan:
                eng.set_search_options(*plan[ply])                 # sz_set_search_options; the Python side's row count follows
                for g in games:
                    g.set_options(*plan[ply])
            live = [g.live for g in games]
            if not any(live):
                break
            for g in games:
                if g.live:
                    g.begin()
                    g.run()
            tag = lambda b: "%s L=%d solver=%d board %d (%s) ply %d start=%s" % (gc.name, eng.L, eng.solver, b, gc.boards[b].name, ply, games[b].starts[-1])
            eng.begin()
            torch.cuda.synchronize()
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search begin", eng, b, g.search.begin_tree, g.search.begin_proven)
            _steps(eng, [g.search for g in games], live, modes, "%s ply %d" % (gc.name, ply), gc.S)
            status = eng.debug_pending()[4]
            st = eng.stats()
            assert [b for b in range(B) if status[b] & ST_ERROR] == [b for b, g in enumerate(games) if g.error], "%s ply %d: boards in error" % (gc.name, ply)
            if any(g.error for g in games):
                assert st["first_error"] == N.SZ_ERR_CAPACITY
            else:
                got = tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth"))
                assert got == tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits", "sum_depth")), "%s ply %d: counters" % (gc.name, ply)
                assert eng.solver_stats() == (sum(g.proven_stops for g in games), sum(g.proved for g in games)), "%s ply %d: solver counters" % (gc.name, ply)
            root = eng.root_proven()[0]
            for b, g in enumerate(games):
                if live[b] and not g.error:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search.tree(), g.search.tree_proven())
                    assert int(root[b]) == int(g.search.R[0]), tag(b)
            u = np.array([gc.boards[b].u(ply) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            rec = eng.fetch_ply()
            for b, g in enumerate(games):
                if not live[b] or g.error:
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tag(b)
                    continue
                want = g.play(u[b])
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r" % (tag(b), got)
                assert eng.debug_position(b)[0].tobytes() == CR.position_record(g.game), "%s: position record of the new root" % tag(b)
    eng.close()
    return games


@pytest.mark.parametrize("L,solver", CR.GAME_OPTIONS)
@pytest.mark.parametrize("name", [gc.name for gc in CR.game_cases()])
def test_whole_games_with_reuse_match_restatement(name, L, solver):
    gc = next(g for g in CR.game_cases() if g.name == name)
    games = _drive_games(gc, L, solver)
    assert all(s in ("new", "reused") + CR.FALLBACKS for g in games for s in g.starts)
    if L > 1 or solver:
        for g in games:
            _game_cov.update(g.cov)
            _game_fb.update(g.fallbacks())


def test_whole_games_coverage():
    if not _game_cov:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for gc in CR.game_cases():
                for L, solver in CR.GAME_OPTIONS[1:]:
                    for g in CR.play(gc, L, solver):
                        _game_cov.update(g.cov)
                        _game_fb.update(g.fallbacks())
    print("coverage:", dict(_game_cov), dict(_game_fb))
    assert all(_game_cov[k] >= 1 for k in CR.GAME_COVERAGE), dict(_game_cov)
    assert all(_game_fb[k] >= 1 for k in CR.FALLBACKS), dict(_game_fb)


# ------------------------------------------------------------------------------------------------ 3. budgets and in-search shrinking
@pytest.mark.parametrize("L", [2, 7])
@pytest.mark.parametrize("max_shrinks", [3, 0])
def test_budgets_and_shrinking_with_solver_and_leaf_batching(max_shrinks, L):
    names = ["mate_in_1", "moves_218", "forced_draw", "mated_in_2", "refuted_move", "mate_in_1", "mated_in_2", "forced_draw"]
    budgets = [200, 64, 0, 120, 200, 1, 64, 17]
    games = [SC.game(n) for n in names]
    eng = SelfPlayEngine(HashModel(salt=0), dict(ALL, C=2, num_searches=200, solver=True, leaves_per_step=L, max_shrinks=max_shrinks), 8, learning=False)
    for b, g in enumerate(games):
        eng.upload_game(b, g)
    eng.set_budgets(budgets)
    eng.search()
    st = eng.check_errors()
    refs = [CR.search(g, s, L=L, solver=True, learning=False, mode="dyadic", salt=0) for g, s in zip(games, budgets)]
    assert st["simulations"] == sum(budgets) and st["boards_done"] == 8 and st["boards_pending"] == 0
    assert st["terminal_hits"] == sum(r.terminal_hits for r in refs) and st["sum_depth"] == sum(r.sum_depth for r in refs)
    assert eng.solver_stats() == (sum(r.proven_stops for r in refs), sum(r.proved for r in refs))
    for b, r in enumerate(refs):
        _assert_tree("board %d budget %d" % (b, budgets[b]), eng, b, r.tree(), r.tree_proven())
        assert int(eng.debug_tree(b)[2][0]) == 1 + budgets[b]
    if max_shrinks:
        assert eng.last_rows < eng.last_steps * 8 * L             # the batch shrank as boards finished
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. setting changes
def test_setting_changes_on_a_reuse_engine_drop_the_kept_subtrees_and_no_change_keeps_them():
    gc = CR.game_cases()[0]._replace(plies=9)
    plan = {2: (4, 1.0, False), 3: (4, 0.5, False), 4: (4, 0.5, True), 6: (1, 0.5, True), 7: (1, 0.5, True)}
    games = _drive_games(gc, 1, False, plan=plan)
    for g in games:
        if len(g.starts) == 9:
            assert [g.starts[p] for p in (2, 4, 6)] == ["dropped"] * 3, g.starts
    assert any(g.starts[3] == "reused" for g in games) and any(g.starts[7] == "reused" for g in games)


def test_options_1_x_0_equal_never_called_and_old_setters_still_refuse():
    lib = N.lib()
    items = [ct for _, ct, _ in CR.solver_items()[(64, False)]]
    trees = []
    for call in (False, True):
        eng = SelfPlayEngine(HashModel(salt=2), {"C": 2, "num_searches": 64}, len(items), learning=True)
        if call:
            assert _options(eng, 1, 0.25, False) == N.SZ_OK
        for b, ct in enumerate(items):
            eng.upload_game(b, ct)
        eng.search()
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(len(items))])
        assert all(not eng.debug_tree_proven(b)[0].any() and not eng.debug_tree_proven(b)[1].any() for b in range(len(items)))
        eng.close()
    for b in range(len(items)):
        for x, y in zip(trees[0][b], trees[1][b]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "board %d" % b
    reuse = SelfPlayEngine(None, {"C": 2, "num_searches": 8, "reuse_subtree": True}, 1, learning=False)
    s = reuse._stream()
    for L, lam, solver in ((4, 1.0, True), (1, 1.0, False), (1, 1.0, True), (2, 0.5, False)):
        assert _options(reuse, L, lam, solver) == N.SZ_OK
        assert lib.sz_set_leaf_batching(reuse._e, 2, 1.0, s) == N.SZ_ERR_INVALID
        assert lib.sz_set_solver(reuse._e, 1, s) == N.SZ_ERR_INVALID
    for L, lam in ((0, 1.0), (257, 1.0), (2, -1.0), (2, float("nan")), (2, float("inf"))):
        assert _options(reuse, L, lam, True) == N.SZ_ERR_INVALID, (L, lam)
    assert lib.sz_set_search_options(reuse._e, None, s) == N.SZ_ERR_INVALID
    budgets = (C.c_int32 * 1)(4)
    assert lib.sz_set_search_budgets(reuse._e, budgets, s) == N.SZ_ERR_INVALID      # still refused on a reuse engine
    reuse.close()
    plain = SelfPlayEngine(None, {"C": 2, "num_searches": 8}, 1, learning=False)
    assert _options(plain, 2, 1.0, False) == N.SZ_OK
    assert lib.sz_set_solver(plain._e, 1, plain._stream()) == N.SZ_ERR_INVALID      # against the state now in force: L > 1
    assert _options(plain, 1, 1.0, True) == N.SZ_OK
    assert lib.sz_set_leaf_batching(plain._e, 2, 1.0, plain._stream()) == N.SZ_ERR_INVALID     # the solver is on
    plain.close()


def test_mid_search_calls_are_refused_and_change_nothing():
    ct = SC.game("mated_in_2")
    want = CR.search(ct, 64, L=4, solver=True, learning=False, mode="dyadic", salt=0)
    eng = SelfPlayEngine(HashModel(salt=0), dict(ALL, C=2, num_searches=64, solver=True, leaves_per_step=4), 1, learning=False)
    eng.upload_game(0, ct)
    eng.begin()
    for L, lam, solver in ((1, 1.0, False), (4, 1.0, True), (8, 0.5, True)):
        assert _options(eng, L, lam, solver) == N.SZ_ERR_STATE
    n = 0
    while eng.pending_boards():
        eng.step(*eng.evaluate(eng.planes))
        n += 1
    eng.check_errors()
    assert n == len(want.steps)
    _assert_tree("after refused calls", eng, 0, want.tree(), want.tree_proven())
    assert _options(eng, 1, 1.0, False) == N.SZ_OK                                # between searches
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. Python
def test_python_key_and_front_ends(monkeypatch):
    three = {"C": 2, "num_searches": 64, "solver": True, "leaves_per_step": 4, "reuse_subtree": True}
    with pytest.raises(ValueError):
        SelfPlayEngine(None, three, 1)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            SelfPlayEngine(None, dict(three, combine_options=bad), 1)
    with pytest.raises(ValueError):
        from sigma_zero_amd.sim import play_games
        play_games(HashModel(), dict(three, combine_options=True, playout_cap={"fast": 8, "p_full": 0.5}), 1)
    eng = SelfPlayEngine(HashModel(salt=1), dict(three, combine_options=True), 2, learning=False)
    eng.upload_game(0, SC.game("endgame_6_men"))
    eng.upload_game(1, SC.game("mate_in_1"))
    eng.search()
    assert eng.check_errors()["simulations"] == 128 and eng.pending_boards() == 0
    eng.close()
    # MCTS0.search on one position: the restatement's visit distribution
    ct = SC.game("mated_in_2")
    m = sz.MCTS0(game=ct, args=dict(three, combine_options=True, num_searches=200), model=HashModel())
    probs = m.search(ct.board, verbose=False, learning=False)
    acts, vis = CR.search(ct, 200, L=4, solver=True, learning=False, mode="dyadic", salt=0).root_children()
    want = {ct.move_from_index(int(x)): int(n) / int(vis.sum()) for x, n in zip(acts, vis)}
    assert list(probs.keys()) == list(want.keys()) and list(probs.values()) == list(want.values())
    # arena.play_match: two greedy games from a Chess960 start, both sides the hash model, against restatement games with all three options
    from sigma_zero_amd.arena import play_match
    plies, recs, fetch = 10, [], SelfPlayEngine.fetch_ply
    monkeypatch.setattr(SelfPlayEngine, "fetch_ply", lambda self: recs.append(fetch(self)) or recs[-1])
    out = play_match(HashModel(), HashModel(), dict(three, combine_options=True), 2, chess960=True, scharnagl=[518, 77], max_plies=plies,
                     planes_dtype=torch.float32)
    results = []
    for b, n in enumerate((518, 77)):
        g = CR.Game(sz.ChessTensor(chess960=True, scharnagl=n), 64, CR.worst_case(64), reuse=True, L=4, solver=True, c=2.0, learning=False, mode="dyadic", salt=0)
        for _ in range(plies):
            if g.live:
                g.begin()
                g.run()
                g.play(-1.0)
        results.append(g.result if g.over else 2)
        assert [int(r["chosen"][b]) for r in recs[:len(g.chosen)]] == g.chosen, "game %d: moves played" % b
        assert "reused" in g.starts
    assert out["results"] == results
