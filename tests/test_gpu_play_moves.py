"""sz_play_moves on the GPU (SelfPlayEngine.play_moves): a GIVEN move played on the device, with the re-rooting that goes with it on a
reuse_subtree engine, held to the host restatement of tests/playmovesref.py ply after ply, and arena.play_options_match built on it.

Lock-step (test_engines_match_the_restatement): per scenario two engines, sides A and B, hold the same boards.  Each searches only when its
side is to move (with `ponder` also on the other side's time) and takes the other's move through play_moves; scripted moves reach both
through play_moves.  No tolerance anywhere.  For every ply of every board:
  * sz_debug_tree after sz_search_begin and at the end of every search equals the restatement's tree: depth, action and visits exactly, value
    sums as f64 bit patterns, priors as f32 bit patterns;
  * every network input equals the restatement's planes for that step; the boards that wait for the network are the restatement's;
  * sz_debug_position after every play_moves (and every play) equals the host mirror's 80 bytes, on both engines; as every ring slot is
    written once, by the ply that reaches it, this compares the ring entry by entry;
  * sz_fetch_ply after play_moves: active 0, chosen, game_over and result as the restatement says; after play: the record of reuseref;
  * sz_get_stats' simulations, expansions and terminal hits equal the restatement's: a given move moves no counter.
Both sides are driven by the restatement's moves; the device's own choices are compared and never steer the host.

Sizes (found with the restatement on the CPU, kept nodes / edges of the continued searches): alternate_c960 S = 64, 8 plies, 6 boards,
1-3 / 18-69; alternate_peaked S = 32, 8 plies, 4 boards, 9-32 / 257-778, "nodes" twice at search begin; alternate_sampled S = 32, 6 plies,
1 / 30-32; positions S = 48, 6 plies, 8 boards; ponder S = 24, 6 plies, 6 boards, 1-8 / 18-175 (38 play_moves on a finished search, 20 of
them keep a subtree); wide S = 32, 4 plies, the 218-move position under four networks, 3-22 / 374-1718 (grandchild spans up to 199);
scripted S = 16, 5 plies.  Fall-backs over all scenarios: no_tree 32, dropped_move 5, unvisited 61, leaf 10, over 5; a two-ply re-rooting
is followed by a continued search on 59 of 104 plies where it could be; three in a row occur.

The other cases: the record against sz_play's on rule_endings' positions (a draw by the 75-move rule and a mate among the games); the
refusals (illegal, out of range, a legal move expansion dropped, sticky errors, byte-identical neighbours, a board in mid-search, -1); visit
targets after a two-ply re-rooting; L = 4, the solver and both on composeref's endgame and Chess960 games, composed from
composeref.Search.reroot applied twice (none of the three option cases was dropped); the match against itself and against a slow path
by upload_game.  That last comparison runs 6 plies, within which no game ends: the two paths agree on the dictionary (plies, results,
no finished pair), while B's continued searches are free to choose other moves than the slow path's fresh ones.

Time (pytest --durations, one run of this module on MI355X): slowest case [alternate_c960] 1.10 s, reuse off 0.81 s, every other case
under 0.45 s, the module 9.0 s for 26 cases.  tests/test_play_moves_ref.py on the CPU: 13 s.

Teeth (shown once, one run each, on scratch copies of the library with one change; not committed):
  A  `bp.npos[new_nid] = pz` removed from wave_keep_subtree, the compaction k_play and k_play_moves share (a kept node keeps another node's
     position record; the edge store stays consistent, so sz_debug_tree walks a sound store).  9 of 26 fail: test_engines_match_the_restatement
     [alternate_c960] "side A board 2 (sp518) ply 2 start=reused step 0: network input differs from the restatement's", likewise
     [alternate_peaked] side A board 0 (sp5) ply 2, [positions] side A board 4 (en_passant_root) ply 2, [wide] side A board 0 (moves_218/0) ply 2,
     all at step 0, and [ponder] side B board 3 (sp959) ply 1 step 11; test_play_moves_writes_the_record_sz_play_writes[True] (engine X
     plays from misplaced positions a move that is illegal on the board: Y's legality test flags it, "invalid argument or illegal move");
     test_two_ply_rerooting_under_leaf_batching_and_the_solver[c960-4-False], [c960-1-True], [c960-4-True] "round 1 step 0 board 1: network
     input rows differ" (the peaked board).  [alternate_sampled], [scripted] and the [endgame-*] option cases keep subtrees of one or two
     nodes and pass, as do the reuse-off cases.
  B  the test of the action's bit in wave_movegen's mask skipped (`legal = 1` for every action below SZ_ACTIONS; the range check kept,
     so nothing is decoded from an index past the 73 planes).  1 of 23 fails (run before the [c960-*] cases existed):
     test_refusals_are_per_board_sticky_and_leave_the_neighbours_alone "assert [False, True, ...] == [True, True, ...]": the illegal
     in-range action on board 0 is played instead of flagged; the out-of-range one on board 1 is still refused.  Every other case gives
     legal moves only and passes.
Neither removal makes sz_debug_tree walk a corrupt store (tests/test_gpu_subtree_reuse.py explains why that matters), so both were run.
"""
import warnings

import numpy as np
import pytest
import torch

from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
from hashmodel import HashModel, evaluate_packed, pack_planes
import playmovesref as P
import reuseref as R

pytestmark = pytest.mark.gpu

ST_PENDING, ST_ERROR = 2, 16
NAMES = ["alternate_c960", "alternate_peaked", "alternate_sampled", "positions", "ponder", "wide", "scripted"]
_played = {}


def _scenario(name):
    return next(sc for sc in P.scenarios() if sc.name == name)


def _assert_tree(tag, got, want):
    d, a, v, w, p = got
    rd, ra, rv, rw, rp = want
    assert np.array_equal(d, rd) and np.array_equal(a, ra), "%s: tree shape (depth, action) differs" % tag
    assert np.array_equal(v, rv), "%s: visits differ at DFS rows %s" % (tag, np.nonzero(v != rv)[0][:8].tolist())
    assert w.tobytes() == rw.tobytes(), "%s: value sums differ (f64 bits)" % tag
    assert p.tobytes() == rp.tobytes(), "%s: priors differ (f32 bits)" % tag


def _engine(S, B, c960, learning, edges, reuse, **more):
    args = {"C": 2, "num_searches": S}
    if reuse:
        args["reuse_subtree"] = True
    args.update(more)
    return SelfPlayEngine(None, args, B, chess960=c960, learning=learning, edges_per_board=edges)


def _search(eng, games, searched, boards, salts, tag):
    """one search of `eng` in lock-step with the restatement's finished searches (games[b].search where searched[b])"""
    B = len(games)
    eng.begin()
    torch.cuda.synchronize()
    for b, g in enumerate(games):
        d = eng.debug_tree(b)
        if not searched[b]:
            assert len(d[0]) == 0, "%s: a board that does not search has a tree" % tag(b)
            continue
        _assert_tree(tag(b) + " at search begin", d, g.search.begin_tree)
    t = 0
    while True:
        torch.cuda.synchronize()
        pend = (eng.debug_pending()[4] & ST_PENDING) != 0
        want = [bool(searched[b]) and t < len(g.search.steps) for b, g in enumerate(games)]
        assert pend.tolist() == want, "%s step %d: boards waiting for the network %s, restatement %s" % (tag(0), t, pend.tolist(), want)
        if not pend.any():
            break
        assert t < eng.S
        planes = pack_planes(eng.planes.float().cpu().numpy())
        pol = np.zeros((B, N.SZ_ACTIONS), np.float32)
        val = np.zeros(B, np.float32)
        for b in np.nonzero(pend)[0]:
            assert np.array_equal(planes[b], games[b].search.steps[t][0]), "%s step %d: network input differs from the restatement's" % (tag(b), t)
            pol[b], val[b] = evaluate_packed(planes[b], boards[b].mode, salts[b])
        eng.step(torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda())
        t += 1
    torch.cuda.synchronize()
    for b, g in enumerate(games):
        if searched[b]:
            _assert_tree(tag(b) + " at search end", eng.debug_tree(b), g.search.tree())


def _assert_positions(eng, games, tag):
    for b, g in enumerate(games):
        pos, gply = eng.debug_position(b)
        assert pos.tobytes() == R.position_record(g.game) and gply == g.game.board.ply, "%s: position record" % tag(b)


def _assert_counters(eng, games, tag):
    st = eng.stats()
    got = (st["simulations"], st["expansions"], st["terminal_hits"])
    assert got == tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits")), "%s: counters %r" % (tag, got)
    assert st["boards_error"] == 0


def drive(sc, reuse=True):
    """two engines (sides A and B), board b = sc.boards[b], through sc.plies plies in lock-step with the restatement -> [(Game A, Game B)]"""
    B = len(sc.boards)
    engs = [_engine(sc.S, B, sc.c960, sc.learning, sc.edges_per_board, reuse) for _ in range(2)]
    games = [P.new_games(sc, bd, reuse) for bd in sc.boards]
    salts = [[bd.salt for bd in sc.boards], [bd.salt + sc.salt_b for bd in sc.boards]]
    for b, sides in enumerate(games):
        for k in range(2):
            engs[k].upload_game(b, sides[k].game)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(sc.plies):
            live = [sides[0].live for sides in games]
            steps = [P.ply_of(sc, bd, ply, sides) for sides, bd in zip(games, sc.boards)]       # the restatement first: it steers both engines
            m = P.side_to_move(ply)
            action = np.array([a for _, _, a, _ in steps], np.int32)
            how = [h for _, _, _, h in steps]
            for k in ([m, 1 - m] if sc.ponder else [m]):
                side = [sides[k] for sides in games]
                tag = lambda b, k=k: "%s side %s board %d (%s) ply %d start=%s" % (sc.name, "AB"[k], b, sc.boards[b].name, ply, side[b].starts[-1] if side[b].starts else None)
                _search(engs[k], side, [s[1][k] for s in steps], sc.boards, salts[k], tag)
            mover, other = engs[m], engs[1 - m]
            mside, oside = [sides[m] for sides in games], [sides[1 - m] for sides in games]
            tagm = lambda b: "%s board %d (%s) ply %d mover %s" % (sc.name, b, sc.boards[b].name, ply, "AB"[m])
            given = np.array([a if h == "given" else -1 for a, h in zip(action, how)], np.int32)
            if (given >= 0).any():                               # scripted moves: the mover takes them on its finished search, before play() moves the rest
                mover.play_moves(given)
                rec = mover.fetch_ply()
                for b in np.nonzero(given >= 0)[0]:
                    assert rec["active"][b] == 0 and rec["chosen"][b] == given[b], "%s: record of a given move" % tagm(b)
                    assert (int(rec["game_over"][b]), int(rec["result"][b])) == (int(mside[b].over), mside[b].result), "%s: game over / result" % tagm(b)
            u = np.array([sc.boards[b].u(ply) if how[b] == "play" else 0.0 for b in range(B)], np.float64)
            mover.play(u)
            rec = mover.fetch_ply()
            for b in range(B):
                if how[b] != "play":
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tagm(b)
                    continue
                assert rec["active"][b] == 1 and int(rec["chosen"][b]) == int(action[b]), "%s: chosen %d, restatement %d" % (tagm(b), rec["chosen"][b], action[b])
                assert (int(rec["game_over"][b]), int(rec["result"][b])) == (int(mside[b].over), mside[b].result), "%s: game over / result" % tagm(b)
            _assert_positions(mover, mside, tagm)
            other.play_moves(action)                             # -1 for the boards whose game had ended
            rec = other.fetch_ply()
            tago = lambda b: "%s board %d (%s) ply %d receiver %s move %s" % (sc.name, b, sc.boards[b].name, ply, "AB"[1 - m], oside[b].moves[-1][1:] if oside[b].moves else None)
            for b in range(B):
                if action[b] < 0:
                    continue
                assert rec["active"][b] == 0 and int(rec["chosen"][b]) == int(action[b]), "%s: record of a given move" % tago(b)
                assert (int(rec["game_over"][b]), int(rec["result"][b])) == (int(oside[b].over), oside[b].result), "%s: game over / result" % tago(b)
            _assert_positions(other, oside, tago)
            for k in range(2):
                _assert_counters(engs[k], [sides[k] for sides in games], "%s ply %d side %s" % (sc.name, ply, "AB"[k]))
                assert not (engs[k].debug_pending()[4] & ST_ERROR).any()
            assert [sides[0].live for sides in games] == [sides[1].live for sides in games]
            del live
    for e in engs:
        e.close()
    return games


@pytest.mark.parametrize("name", NAMES)
def test_engines_match_the_restatement(name):
    """reuse on: the re-rooted trees at every search begin and end, network inputs, positions, records and counters, every ply, both sides"""
    sc = _scenario(name)
    games = drive(sc, reuse=True)
    _played[name] = (sc, games)
    assert not any(g.error for sides in games for g in sides)


@pytest.mark.parametrize("name", ["alternate_c960", "positions", "ponder", "scripted"])
def test_reuse_off_every_search_is_fresh(name):
    """reuse off: play_moves moves the game and keeps nothing; every search starts from a bare root"""
    games = drive(_scenario(name), reuse=False)
    assert all(not s.continued for sides in games for g in sides for s in g.searches)


def test_coverage_conditions_counted_on_the_restatement():
    """counted by the restatement on the games the device was compared with in this run (a deselected scenario is replayed on the
    restatement alone: the games do not depend on the device)"""
    assert NAMES == [sc.name for sc in P.scenarios()]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        played = [_played.get(sc.name) or (sc, P.play(sc)) for sc in P.scenarios()]
    c = P.coverage(played)
    print("coverage:", {k: (dict(v) if hasattr(v, "items") else v) for k, v in c.items()})
    P.assert_coverage(c)


# ------------------------------------------------------------------------------------------------ the same record as sz_play
def _ending_boards():
    import sigma_zero_amd as sz
    import rule_endings as RE
    from test_gpu_parity import FENS
    case = lambda name: RE.build(next(c for c in RE.CASES if c[0] == name))[0]
    return [("clock_149", case("clock_149")),                       # every move is a draw by the 75-move rule
            ("fivefold_next_move", case("fivefold_next_move")), ("kb_v_k_by_capture", case("kb_v_k_by_capture")),
            ("ring_wrap_260_plies", case("ring_wrap_260_plies")), ("window_84_plies", case("window_84_plies")),
            ("kqk", sz.ChessTensor(fen=FENS[4])), ("back_rank_mate", sz.ChessTensor(fen=FENS[6])), ("moves_218", sz.ChessTensor(fen=FENS[10])),
            ("start", sz.ChessTensor())]


@pytest.mark.parametrize("reuse", [False, True])
def test_play_moves_writes_the_record_sz_play_writes(reuse):
    """engine X searches and plays greedily; engine Y, from the same upload, gets X's chosen move through play_moves and never searches.
    Position record and ply agree after every ply, with each other and with the host mirror playing the same moves (every ring slot is
    written once, so this is the ring entry by entry); game_over and result agree, a mate and a draw by rule among them."""
    boards = _ending_boards()
    B, S = len(boards), 48
    X, Y = _engine(S, B, False, False, R.worst_case(S), reuse), _engine(S, B, False, False, R.worst_case(S), reuse)
    mirror = [g.copy() for _, g in boards]
    for b, g in enumerate(mirror):
        X.upload_game(b, g)
        Y.upload_game(b, g)
    X.model = HashModel()
    ended = {}
    for ply in range(4):
        X.search()
        X.check_errors()
        X.play(np.full(B, -1.0))
        rx = X.fetch_ply()
        moved = rx["active"].astype(bool)
        Y.play_moves(np.where(moved, rx["chosen"], -1))
        ry = Y.fetch_ply()
        Y.check_errors()
        for b in np.nonzero(moved)[0]:
            name = boards[b][0]
            mirror[b].push_action(int(rx["chosen"][b]))
            v, t = mirror[b].get_value_and_terminated()
            want = (int(t), 0 if not (t and v) else (-1 if mirror[b].board.turn else 1))
            assert (int(rx["game_over"][b]), int(rx["result"][b])) == want == (int(ry["game_over"][b]), int(ry["result"][b])), "%s ply %d" % (name, ply)
            assert ry["active"][b] == 0 and ry["chosen"][b] == rx["chosen"][b]
            (px, lx), (py, ly) = X.debug_position(b), Y.debug_position(b)
            assert px.tobytes() == py.tobytes() == R.position_record(mirror[b]) and lx == ly == mirror[b].board.ply, "%s ply %d: position record" % (name, ply)
            if want[0]:
                ended[name] = want[1]
    X.close()
    Y.close()
    assert ended.get("clock_149") == 0, "the draw by the 75-move rule: %r" % ended
    assert any(r != 0 for r in ended.values()), "a mating move: %r" % ended


# ------------------------------------------------------------------------------------------------ refusals
def _refusal_run(bad):
    """six Chess960 starts on a reuse engine: search, then play_moves.  bad=True: board 0 gets an illegal action, board 1 one out of range,
    board 2 a legal move expansion dropped; bad=False: those three get -1.  Boards 3-5 get their most visited move either way.  Then a second
    search.  -> what the neighbours (and board 2) look like"""
    import sigma_zero_amd as sz
    S = 16
    sch = P.dropped_starts(want=3, salt=0) + [5, 77, 400]
    sch = [sch[2], sch[1], sch[0]] + sch[3:]
    B = len(sch)
    eng = _engine(S, B, True, False, R.worst_case(S), True)
    eng.model = HashModel()
    eng.new_games(sch)
    games = [P.Game(sz.ChessTensor(chess960=True, scharnagl=n), S, R.worst_case(S), reuse=True, c=2.0, learning=False, mode="dyadic", salt=0) for n in sch]
    for g in games:
        g.begin()
        g.run()
    eng.search()
    legal = [[int(a) for a in g.game.legal_action_indices()] for g in games]
    best = [int(g.search.root_children()[0][np.argmax(g.search.root_children()[1])]) for g in games]
    acts = np.array(best, np.int32)
    acts[:3] = -1
    if bad:
        acts[0] = next(a for a in range(N.SZ_ACTIONS) if a not in legal[0])
        acts[1] = N.SZ_ACTIONS
        acts[2] = P.pick("dropped", games[2])
    eng.play_moves(acts)
    rec = eng.fetch_ply()
    out = dict(eng=eng, games=games, acts=acts, rec=rec, best=best)
    return out


def test_refusals_are_per_board_sticky_and_leave_the_neighbours_alone():
    bad, good = _refusal_run(True), _refusal_run(False)
    eng, games, acts = bad["eng"], bad["games"], bad["acts"]
    status = eng.debug_pending()[4]
    st = eng.stats()
    assert [bool(s & ST_ERROR) for s in status] == [True, True, False, False, False, False]
    assert st["boards_error"] == 2 and st["first_error"] == N.SZ_ERR_INVALID
    for b in (0, 1):                                                # nothing else on the board changed: position and ply of the start
        pos, ply = eng.debug_position(b)
        assert pos.tobytes() == R.position_record(games[b].game) and ply == 0
        assert games[b].play_move(int(acts[b]) if acts[b] < N.SZ_ACTIONS else 10 ** 6) == "invalid"
    # the dropped move is legal: it is played, and nothing is kept
    assert games[2].play_move(int(acts[2])) == "dropped_move"
    pos, ply = eng.debug_position(2)
    assert pos.tobytes() == R.position_record(games[2].game) and ply == 1 and bad["rec"]["chosen"][2] == acts[2] and not bad["rec"]["active"][2]
    for b in (3, 4, 5):
        assert games[b].play_move(int(acts[b])) in ("kept", "unvisited")
    # sticky: a legal move on a board in error changes nothing
    again = np.full(len(games), -1, np.int32)
    again[0], again[1] = bad["best"][0], bad["best"][1]
    eng.play_moves(again)
    for b in (0, 1):
        assert eng.debug_position(b)[1] == 0
    assert eng.stats()["first_error"] == N.SZ_ERR_INVALID and eng.stats()["boards_error"] == 2
    # the next search: board 2 from a bare root, the neighbours as in the run without the bad boards, byte for byte
    for e in (eng, good["eng"]):
        e.begin()
    torch.cuda.synchronize()
    for g in games[2:]:
        g.begin()
    assert games[2].starts[-1] == "dropped_move"
    _assert_tree("board 2 after a dropped move", eng.debug_tree(2), (np.array([-1], np.int32), np.array([-1], np.int32), np.array([1], np.int32),
                                                                     np.zeros(1, np.float64), np.zeros(1, np.float32)))
    for b in (3, 4, 5):
        x, y = eng.debug_tree(b), good["eng"].debug_tree(b)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y)), "board %d: tree differs from the run without the bad boards" % b
        assert eng.debug_position(b)[0].tobytes() == good["eng"].debug_position(b)[0].tobytes()
        for key in ("chosen", "game_over", "result", "active"):    # what play_moves writes; no sz_play has filled the rest
            assert np.array_equal(bad["rec"][key][b], good["rec"][key][b]), "board %d: record field %s" % (b, key)
        games[b].run()
        if games[b].starts[-1] == "reused":
            _assert_tree("board %d continues on the kept subtree" % b, x, games[b].search.begin_tree)
    # -1 left boards 0-2 of the good run alone: their finished search is still there to be played
    geng = good["eng"]
    assert not (geng.debug_pending()[4] & ST_ERROR).any()
    eng.close()
    geng.close()


def test_minus_one_keeps_the_record_and_the_kept_subtree():
    """a board with -1 keeps rec_active and the subtree sz_play kept: the next search continues on it as if play_moves had not been called"""
    S, sch = 32, [5, 77, 400, 811]
    engs = [_engine(S, 4, True, False, R.worst_case(S), True) for _ in range(2)]
    trees = []
    for k, e in enumerate(engs):
        e.model = HashModel(mode="peaked")
        e.new_games(sch)
        e.search()
        e.play(np.full(4, -1.0))
        if k == 0:
            e.play_moves(np.full(4, -1, np.int32))
        rec = e.fetch_ply()
        assert rec["active"].tolist() == [1, 1, 1, 1]
        e.begin()
        torch.cuda.synchronize()
        trees.append([e.debug_tree(b) for b in range(4)])
        e.close()
    assert all(len(t[0]) > 1 for t in trees[0]), "the kept subtrees are continued on"
    for x, y in zip(*trees):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


def test_a_board_in_mid_search_is_flagged():
    eng = _engine(8, 2, True, False, R.worst_case(8), True)
    eng.new_games([1, 2])
    eng.begin()
    import sigma_zero_amd as sz
    eng.play_moves(np.array([sz.ChessTensor(chess960=True, scharnagl=1).legal_action_indices()[0], -1], np.int32))
    st = eng.stats()
    status = eng.debug_pending()[4]
    assert st["boards_error"] == 1 and st["first_error"] == N.SZ_ERR_STATE and (status[0] & ST_ERROR) and not (status[1] & ST_ERROR)
    assert eng.debug_position(0)[1] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ with the other options
def test_visit_targets_count_the_grandchild_visits():
    """visit targets: after a two-ply re-rooting the goal of the continued search is max(0, t + 1 - N_kept)"""
    import sigma_zero_amd as sz
    S, sch, t = 32, [5, 77, 400, 811], np.array([32, 20, 8, 2], np.int32)
    A = _engine(S, 4, True, False, R.worst_case(S), True, visit_targets=True)
    A.model = HashModel(mode="peaked")
    A.new_games(sch)
    games = [P.Game(sz.ChessTensor(chess960=True, scharnagl=n), S, R.worst_case(S), reuse=True, c=2.0, learning=False, mode="peaked", salt=0) for n in sch]
    A.search()
    A.play(np.full(4, -1.0))
    reply = []
    for g in games:
        g.begin()
        g.run()
        g.play(-1.0)
        acts, vis = g.kept.root_children()                       # the reply the kept subtree has thought about most
        reply.append(int(acts[np.argmax(vis)]))
        assert g.play_move(reply[-1]) == "kept" and g.rerooted == 2
    A.play_moves(np.array(reply, np.int32))
    A.set_visit_targets(t)
    A.begin()
    goals = A.search_goals()
    kept = np.array([int(g.kept.N[0]) for g in games])
    assert goals.tolist() == np.maximum(0, t + 1 - kept).tolist(), "goals %s, kept root visits %s" % (goals.tolist(), kept.tolist())
    assert (goals == 0).any() and (goals > 0).any()
    for b, g in enumerate(games):
        d = A.debug_tree(b)
        assert int(d[2][0]) == kept[b]
    A.close()


@pytest.mark.parametrize("L,solver", [(4, False), (1, True), (4, True)])
@pytest.mark.parametrize("case", ["endgame", "c960"])
def test_two_ply_rerooting_under_leaf_batching_and_the_solver(case, L, solver):
    """L = 4, the solver, and both: composeref's endgame games and its Chess960 games (a peaked evaluator among them: large kept subtrees), where after every play() the board is given the reply its kept subtree has
    visited most (composeref.Search.reroot applied a second time, to the kept tree).  At the begin and the end of the next search the
    device's tree equals the restatement's (sz_debug_tree), and so do the proven labels and `complete` bits of the kept grandchild subtree
    (sz_debug_tree_proven); every network row of the continued search equals the restatement's."""
    import composeref as CR
    from test_gpu_compose import _assert_tree as assert_tree_proven, _steps, ALL
    gc = next(g for g in CR.game_cases() if g.name == case)
    B = len(gc.boards)
    args = dict(ALL, C=2, num_searches=gc.S, solver=solver, leaves_per_step=L, reuse_subtree=True)
    eng = SelfPlayEngine(None, args, B, chess960=gc.c960, learning=gc.learning, edges_per_board=gc.edges_per_board)
    games = [CR.new_game(gc, bd, L, solver) for bd in gc.boards]
    modes = [(bd.mode, bd.salt) for bd in gc.boards]
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    two_ply = labelled = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for rnd in range(4):
            live = [g.live for g in games]
            for g in games:
                if g.live:
                    g.begin()
                    g.run()
            tag = lambda b: "L=%d solver=%d board %d round %d start=%s" % (L, solver, b, rnd, games[b].starts[-1])
            eng.begin()
            torch.cuda.synchronize()
            for b, g in enumerate(games):
                if live[b]:
                    assert_tree_proven(tag(b) + " at search begin", eng, b, g.search.begin_tree, g.search.begin_proven)
                    if rnd and g.starts[-1] == "reused":
                        two_ply += 1
                        labelled += bool(g.search.begin_proven[0].any() or g.search.begin_proven[1].any())
            _steps(eng, [g.search for g in games], live, modes, "round %d" % rnd, gc.S)
            for b, g in enumerate(games):
                if live[b]:
                    assert_tree_proven(tag(b) + " at search end", eng, b, g.search.tree(), g.search.tree_proven())
            u = np.array([gc.boards[b].u(rnd) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            reply = np.full(B, -1, np.int32)
            for b, g in enumerate(games):
                if not live[b]:
                    continue
                g.play(u[b])
                if g.over or g.next is None or g.next[1] != "reused":
                    continue                                        # -1: the board is left alone (a one-ply re-rooting, or none)
                acts, vis = g.next[0].root_children()
                reply[b] = int(acts[np.argmax(vis)])
                g.game.push_action(int(reply[b]))
                v, t = g.game.get_value_and_terminated()
                g.over = bool(t)
                g.result = 0 if not (t and v) else (-1 if g.game.board.turn else 1)
                g.next = None if g.over else g.next[0].reroot(int(reply[b]), g.game)
            eng.play_moves(reply)
            rec = eng.fetch_ply()
            for b, g in enumerate(games):
                if live[b]:
                    assert eng.debug_position(b)[0].tobytes() == CR.position_record(g.game), "%s: position record" % tag(b)
                    if reply[b] >= 0:
                        assert (int(rec["chosen"][b]), int(rec["game_over"][b]), int(rec["result"][b]), int(rec["active"][b])) == (int(reply[b]), int(g.over), g.result, 0)
    eng.check_errors()
    eng.close()
    assert two_ply >= 3, "continued searches after a two-ply re-rooting: %d" % two_ply
    if solver and case == "endgame":
        assert labelled >= 1, "a kept grandchild subtree that carries proven labels or complete bits"


# ------------------------------------------------------------------------------------------------ the match
def test_match_of_a_configuration_against_itself_is_even_pair_by_pair():
    """args_a == args_b, greedy, 4 pairs.  So that the games end within a few plies, both configurations adjudicate a draw after their third
    search (args["endings"] with draw_value 1: every search qualifies), which also runs the path of an ending (chosen -1, game over) that
    ends a game for both engines.  The games of a pair are the same game, A scores exactly 0.5, only 1-1 pairs, identical final positions."""
    from sigma_zero_amd.arena import play_options_match
    args = {"C": 2, "num_searches": 16, "endings": {"draw_value": 1.0, "draw_patience": 3}}
    timing = {}
    out = play_options_match(HashModel(), args, dict(args), 4, chess960=True, scharnagl=[5, 77, 400, 811], max_plies=12, check_positions=True, timing=timing)
    assert out["unfinished"] == 0 and out["results"] == [0] * 8 and out["draws"] == 8
    assert out["score"] == 0.5 and out["pentanomial"] == [0, 0, 4, 0, 0] and out["elo"] == 0.0
    assert out["plies"] == [out["plies"][0]] * 8 and 4 <= out["plies"][0] <= 6, out["plies"]
    a, b = timing["final_positions"]
    assert a == b, "both engines end with identical positions"
    for i in range(4):                                              # the games of a pair are the same game
        assert a[2 * i] == a[2 * i + 1]
    assert len(set(a)) == 4, "different starts give different games"


def test_match_with_reuse_on_one_side_equals_the_slow_path_by_upload():
    """args_b adds reuse_subtree; the slow path moves the other side by upload_game (which drops B's kept subtree at every opponent move)"""
    from sigma_zero_amd.arena import play_options_match, match_stats
    import sigma_zero_amd as sz
    args_a = {"C": 2, "num_searches": 16}
    args_b = dict(args_a, reuse_subtree=True)
    sch, n, max_plies = [5, 77, 400, 811], 8, 6
    fast = play_options_match(HashModel(), args_a, args_b, 4, chess960=True, scharnagl=sch, max_plies=max_plies, check_positions=True)
    engs = [SelfPlayEngine(HashModel(), a, n, chess960=True, learning=False, edges_per_board=R.worst_case(16)) for a in (args_a, args_b)]
    mirror = [sz.ChessTensor(chess960=True, scharnagl=sch[g // 2]) for g in range(n)]
    for e in engs:
        e.new_games(np.repeat(sch, 2))
    a_is_white = np.arange(n) % 2 == 0
    results, plies = np.full(n, 2, np.int8), np.zeros(n, np.int64)
    for _ in range(max_plies):
        live = results == 2
        to_move = [live & (a_is_white == (plies % 2 == 0)), live & (a_is_white != (plies % 2 == 0))]
        recs = []
        for k, e in enumerate(engs):
            e.set_active(to_move[k])
            e.compact()
            e.search()
            e.check_errors()
            e.play(np.full(n, -1.0))
            recs.append(e.fetch_ply())
        for k, e in enumerate(engs):
            for g in np.nonzero(to_move[k])[0]:
                mirror[g].push_action(int(recs[k]["chosen"][g]))
                engs[1 - k].upload_game(int(g), mirror[g])
                if recs[k]["game_over"][g]:
                    results[g] = recs[k]["result"][g]
                plies[g] += 1
    for e in engs:
        e.close()
    results_a = np.where(results == 2, 2, np.where(a_is_white, results, -results)).astype(np.int8)
    slow = match_stats(results_a)
    slow.update(results=results.tolist(), results_a=results_a.tolist(), plies=plies.tolist())
    assert fast == slow
