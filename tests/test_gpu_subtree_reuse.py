"""Subtree reuse on the GPU (sz_config.reuse_subtree / args["reuse_subtree"], a NON-REFERENCE option): k_play's in-place compaction and the
search that continues on the kept subtree, held to the plain-Python re-rooted search of tests/reuseref.py, ply after ply.

For every ply of every board of every scenario (reuseref.scenarios()), no tolerance anywhere:
  * after sz_search_begin and at the end of the search, sz_debug_tree equals the restatement's tree: depth, action, visits exactly, value
    sums as f64 bit patterns, priors as f32 bit patterns;
  * every network input the device writes equals the restatement's planes for that step, and the boards that wait for the network are
    the ones the restatement says (a misplaced position record of a kept node shows here: its children are made from a wrong parent);
  * sz_fetch_ply (packed root planes, child actions, visits, chosen action, colour, game over, result, active) equals the restatement's
    record, sz_debug_position of the new root equals the host mirror's 80-byte record;
  * sz_get_stats: simulations, expansions, terminal hits equal the restatement's counters (not in the two overflow scenarios, where the
    check is that SZ_ERR_CAPACITY is raised on exactly the boards, and at the step, where the restatement runs out of child slots).
Both sides are driven by the same uniforms; the device's choice is never read to steer the host.  The coverage conditions (every
fall-back, reuse on at least half of the pairs, a kept node wider than 64 children, a revisited kept terminal node, three reused plies in
a row) are counted on the restatement and asserted in test_coverage_conditions_counted_on_the_restatement; tests/test_reuse_ref.py proves
them on the CPU.  Sizes (found with the restatement, kept nodes / edges per reused ply): starts S = 64, 8 plies, 2-21 / 33-621;
positions S = 48, 6 plies, up to 48 / 425 (the 218-move position: spans of 201); peaked S = 32, 7 plies, 13-32 / 310-828 with "nodes"
13 times; few_edges S = 32 on 1350 child slots, "edges" 3 times and no overflow; last_child S = 12, "unvisited" twice; "leaf" 10 times.

Time (pytest --durations of one run of the whole GPU suite on MI355X): the slowest case here is [positions_learning1] with reuse off, 0.69 s
(with reuse: [classical_starts] 0.67 s; refill and compaction 0.42 s; the whole module 6 s), against the slowest pre-existing case of the same
run, test_gpu_round3.py::test_bench_plain_run_is_the_headline_and_full_adds_the_side_measurements, 25.5 s.  tests/test_reuse_ref.py on the CPU:
4.1 s for its slowest item (the scenarios played once), 8.4 s the module, against 14.2 s for the slowest pre-existing CPU case
(test_network_and_train.py::test_multi_rank_training_with_unequal_batch_counts_does_not_deadlock) of the same run.

Teeth (shown once, one run each, on scratch copies of the library with one line of k_play's compaction removed; not committed).  "old" is the
pre-existing test_gpu_train_and_precision.py::test_subtree_reuse_option_carries_the_chosen_subtree_exactly_and_default_is_off.
  A  `bp.npos[new_nid] = pz` removed (a kept node keeps another node's position record): old PASSES.  Here 8 of 15 fail:
     test_engine_with_reuse_matches_the_rerooted_host_search[c960_starts_learning] "c960_starts_learning board 5 (sp702) ply 1 start=reused
     step 17: network input differs from the restatement's"; [classical_starts] "board 0 (start/1) ply 1 start=reused step 0: network input
     differs ..."; likewise [positions_learning0] board 5 (en_passant_root), [positions_learning1] board 1 (pawn_endgame_e2), [peaked] board 0,
     [few_edges] board 0, [overflow_continued] board 0, all at ply 1 step 0; test_refill_and_compaction_with_reuse_give_identical_per_game_records
     "learning=0 game 1, two slots: moves played ... At index 5 diff: 119 != 48".  The reuse-off cases, overflow_fresh and last_child (kept
     subtrees of one node) pass, as they should.
  D  `bp.em[e_new].node = new_nid` removed (a stale node id in every kept edge): here the same 8 cases and [last_child] fail (progress line
     FFFFFF.FF.....F); the old test then died in the host code of sz_debug_tree (segmentation fault: the second compaction skips kept nodes whose
     stale id is past n_nodes, their `first` keeps pointing past n_edges and the dump follows it), so this run has no messages.
  B  `nmap[m2.node] = cursor + k` removed: [c960_starts_learning] failed, then sz_debug_tree's host walk of the corrupt store (spans shared by
     several parents) grew without bound in host memory until the run was ended; no GPU fault, no messages; not run again.
  C  the rewrite of `em[e_new].first` removed: NOT run.  It leaves every kept edge pointing at its old span, the same shared-span store that B
     produced, so the same host walk was to be expected; D was run in its place.
sz_debug_tree trusts the store it dumps; on a corrupt one it can crash or exhaust the host.  That is a weakness of the test hook, seen with
B and D only, and is left as it is here.
"""
import warnings

import numpy as np
import pytest
import torch

from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
from hashmodel import HashModel, evaluate_packed, pack_planes
import reuseref as R

pytestmark = pytest.mark.gpu

ST_PENDING, ST_ERROR = 2, 16
NAMES = ["c960_starts_learning", "classical_starts", "positions_learning0", "positions_learning1", "peaked", "few_edges", "overflow_fresh",
         "overflow_continued", "last_child"]
_played = {}                                                # scenario name -> (Scenario, [Game]) of the runs with reuse on


def _scenario(name):
    return next(sc for sc in R.scenarios() if sc.name == name)


def _assert_tree(tag, got, want):
    d, a, v, w, p = got
    rd, ra, rv, rw, rp = want
    assert np.array_equal(d, rd) and np.array_equal(a, ra), "%s: tree shape (depth, action) differs" % tag
    assert np.array_equal(v, rv), "%s: visits differ at DFS rows %s" % (tag, np.nonzero(v != rv)[0][:8].tolist())
    assert w.tobytes() == rw.tobytes(), "%s: value sums differ (f64 bits)" % tag
    assert p.tobytes() == rp.tobytes(), "%s: priors differ (f32 bits)" % tag


def drive(sc, reuse=True):
    """one engine, board b = sc.boards[b], through sc.plies plies in lock-step with the restatement; -> the restatement's games"""
    B = len(sc.boards)
    args = {"C": 2, "num_searches": sc.S}
    if reuse:
        args["reuse_subtree"] = True
    eng = SelfPlayEngine(None, args, B, chess960=sc.c960, learning=sc.learning, edges_per_board=sc.edges_per_board)
    games = [R.new_game(sc, bd, reuse) for bd in sc.boards]
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    compared = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # NaN priors (a policy that is 0 on every legal move), as in the reference
        for ply in range(sc.plies):
            live = [g.live for g in games]
            for g in games:
                if g.live:
                    g.begin()
                    g.run()
            tag = lambda b: "%s board %d (%s) ply %d start=%s" % (sc.name, b, sc.boards[b].name, ply, games[b].starts[-1])
            eng.begin()
            torch.cuda.synchronize()
            for b, g in enumerate(games):
                d = eng.debug_tree(b)
                if not live[b]:
                    assert len(d[0]) == 0, "%s: a board whose game ended searches" % tag(b)
                    continue
                _assert_tree(tag(b) + " at search begin", d, g.search.begin_tree)
            t = 0
            while True:
                torch.cuda.synchronize()
                status = eng.debug_pending()[4]
                pend = (status & ST_PENDING) != 0
                want = [live[b] and t < len(g.search.steps) for b, g in enumerate(games)]
                assert pend.tolist() == want, "%s step %d: boards waiting for the network %s, restatement %s" % (sc.name, t, pend.tolist(), want)
                if not pend.any():
                    break
                assert t < sc.S
                planes = pack_planes(eng.planes.float().cpu().numpy())
                pol = np.zeros((B, N.SZ_ACTIONS), np.float32)
                val = np.zeros(B, np.float32)
                for b in np.nonzero(pend)[0]:
                    assert np.array_equal(planes[b], games[b].search.steps[t][0]), "%s step %d: network input differs from the restatement's" % (tag(b), t)
                    pol[b], val[b] = evaluate_packed(planes[b], sc.boards[b].mode, sc.boards[b].salt)
                eng.step(torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda())
                t += 1
            torch.cuda.synchronize()
            status = eng.debug_pending()[4]
            st = eng.stats()
            errors = [b for b, g in enumerate(games) if live[b] and g.error]
            assert [b for b in range(B) if status[b] & ST_ERROR] == [b for b, g in enumerate(games) if g.error], "%s ply %d: boards in error" % (sc.name, ply)
            if any(g.error for g in games):
                assert st["first_error"] == N.SZ_ERR_CAPACITY and all(g.error == "capacity" for g in games if g.error)
            else:
                got = (st["simulations"], st["expansions"], st["terminal_hits"])
                assert got == tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits")), "%s ply %d: counters" % (sc.name, ply)
            for b, g in enumerate(games):
                if live[b] and not g.error:
                    _assert_tree(tag(b) + " at search end", eng.debug_tree(b), g.search.tree())
            u = np.array([sc.boards[b].u(ply) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            rec = eng.fetch_ply()
            for b, g in enumerate(games):
                if not live[b] or b in errors:
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tag(b)
                    compared += live[b]
                    continue
                want = g.play(u[b])
                assert rec["active"][b] == 1
                assert np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r" % (tag(b), got)
                pos, gply = eng.debug_position(b)
                assert pos.tobytes() == R.position_record(g.game) and gply == g.game.board.ply, "%s: position record of the new root" % tag(b)
                compared += 1
    assert eng.stats()["boards_error"] == sum(1 for g in games if g.error)
    eng.close()
    assert compared == sum(len(g.starts) for g in games), "every (board, ply) pair is compared"
    return games


@pytest.mark.parametrize("name", NAMES)
def test_engine_with_reuse_matches_the_rerooted_host_search(name):
    """scenarios 1-5: trees at search begin and end, every network input, training records, position records and counters, every ply"""
    sc = _scenario(name)
    games = drive(sc, reuse=True)
    _played[name] = (sc, games)
    if name.startswith("overflow"):
        assert [g.error for g in games] == ["capacity"]
    else:
        assert not any(g.error for g in games)
        assert any(len(g.starts) == sc.plies for g in games)


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("c960", "classical", "positions"))])
def test_reuse_off_on_the_same_inputs_is_the_fresh_search(name):
    """scenario 7: without the option every ply starts from a bare root and equals the reference's search (tests/test_reuse_ref.py: the
    restatement with reuse off is vlref.search ply by ply)"""
    games = drive(_scenario(name), reuse=False)
    assert all(s == "new" for g in games for s in g.starts)


def test_coverage_conditions_counted_on_the_restatement():
    """counted by the restatement, on the games the device was compared with in this run (a scenario that was deselected is replayed on
    the restatement alone: the games are the same, they do not depend on the device)"""
    assert NAMES == [sc.name for sc in R.scenarios()]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        played = [_played.get(sc.name) or (sc, R.play(sc)) for sc in R.scenarios()]
    c = R.coverage(played)
    print("coverage:", {k: (dict(v) if hasattr(v, "items") else v) for k, v in c.items()})
    R.assert_coverage(c)


def test_refill_and_compaction_with_reuse_give_identical_per_game_records():
    """scenario 6: six games on two slots with sz_compact and refill against one slot per game, both with reuse, and against the restatement
    game by game: a refilled slot starts its game from a bare root, never from the previous game's subtree"""
    from sigma_zero_amd.sim import play_games
    S, n_games = 16, 6
    args = {"C": 2, "num_searches": S, "reuse_subtree": True}
    sch = [31, 32, 500, 640, 77, 903]
    caps = [5, 9, 4, 7, 6, 8]
    uni = lambda g, ply: ((g * 7919 + ply * 104729 + 17) % 1000003) / 1000003.0 if (g + ply) % 3 else -1.0
    runs = [play_games(HashModel(), args, n_games, c960=True, scharnagl=sch, uniforms=uni, learning=learning, max_plies=caps, **kw)
            for learning in (False, True) for kw in (dict(n_boards=2, compact=True), dict(compact=False))]
    import sigma_zero_amd as sz
    n_reused = 0
    for k, learning in enumerate((False, True)):
        packed, plain = runs[2 * k], runs[2 * k + 1]
        for g in range(n_games):
            ref = R.Game(sz.ChessTensor(chess960=True, scharnagl=sch[g]), S, R.worst_case(S), reuse=True, c=2.0, learning=learning, mode="dyadic", salt=0)
            recs = []
            for ply in range(caps[g]):
                if not ref.live:
                    break
                ref.begin()
                ref.run()
                recs.append(ref.play(uni(g, ply)))
            n_reused += sum(s == "reused" for s in ref.starts)
            assert ref.starts[0] == "new"
            for name, run in (("two slots", packed), ("one slot per game", plain)):
                tag = "learning=%d game %d, %s" % (learning, g, name)
                got = run[g]
                assert got["chosen_actions"] == ref.chosen, "%s: moves played" % tag
                assert len(got["packed_states"]) == len(recs) and all(np.array_equal(x, r["packed"]) for x, r in zip(got["packed_states"], recs)), "%s: states" % tag
                for x, r in zip(got["actions"], recs):
                    vis = r["visits"][:r["n_child"]].astype(np.int64)
                    assert list(x.values()) == (vis / int(vis.sum())).tolist(), "%s: visit distribution" % tag
                assert got["colours"] == [bool(r["colour"]) for r in recs]
                assert got["result"] == ({1: "1-0", -1: "0-1", 0: "1/2-1/2"}[ref.result] if ref.over else None)
    assert n_reused >= n_games * 2
