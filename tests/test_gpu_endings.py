"""Resignation and adjudicated game endings on the GPU (sz_set_endings / sz_fetch_endings / sz_ending_stats / sz_debug_endings,
args["endings"], a NON-REFERENCE option): the HIP engine against the plain-Python restatement tests/endingref.py, bit for bit and ply after
ply — whole trees at search begin and end, every network input row of every step, step counts, the counters, the training records, what
sz_fetch_endings and sz_ending_stats say, the position after sz_play (the unchanged root where a game was ended) — plus the device's
decision function on seeded cases, off is off, a new game resets the state, the setter rules and play_games end to end.
tests/test_ending_ref.py proves on the CPU that the scenarios and hook cases reach the conditions they are there for.
m is compared by its bits (so -0.0 is not 0.0), except that any NaN equals any NaN: the payload of 0 / 0 is not part of the rule."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
from hashmodel import HashModel
import endingref as ER
import forcedref as FR
from endingref import DRAW_ADJ, NONE, PROVEN, RESIGN, options
from hashmodel import evaluate_packed, pack_planes

pytestmark = pytest.mark.gpu

ST_PENDING = 2
REUSE = {"combine_options": True, "reuse_subtree": True, "C": 2, "num_searches": 64}
PLAIN = {"combine_options": True, "C": 2, "num_searches": 64}


def _assert_tree(tag, eng, b, tree, proven):
    for x, y in zip(eng.debug_tree(b), tree):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: tree differs" % tag
    pr, co = eng.debug_tree_proven(b)
    assert np.array_equal(pr, proven[0]) and np.array_equal(co, proven[1]), "%s: proven labels / complete bits differ" % tag


def _steps(eng, searches, live, modes, tag, S):
    """the steps of one search on every live board b against searches[b]: boards pending, every network input row, step count"""
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


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def _same_value(a, b):
    a, b = np.float64(a), np.float64(b)
    return bool(np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. whole games against the restatement
def _drive(sc, L, solver):
    B = len(sc.boards)
    eng = SelfPlayEngine(None, dict(REUSE if sc.reuse else PLAIN, num_searches=sc.S, solver=solver, leaves_per_step=L), B, chess960=sc.c960,
                         learning=sc.learning, edges_per_board=sc.edges_per_board or 0)
    games = [ER.new_game(sc, bd, L, solver) for bd in sc.boards]
    modes = [(bd.mode, bd.salt) for bd in sc.boards]
    gam = ER.gammas(sc)
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    holdout = [bd.holdout for bd in sc.boards]
    n_plies = n_steps = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(sc.plies):
            live = [g.live for g in games]
            if not any(live):
                break
            n_plies += 1
            numbers = [bd.targets[ply] if live[b] else 0 for b, bd in enumerate(sc.boards)]
            if sc.reuse:
                eng.set_visit_targets(numbers)
            else:
                eng.set_budgets(numbers)
            eng.set_search_root_noise(torch.from_numpy(gam[ply]) if sc.noise[ply] else None, [bd.quiet[ply] for bd in sc.boards])
            eng.set_forced_playouts(sc.k[ply], [bd.forced[ply] for bd in sc.boards])
            eng.set_endings(sc.endings[ply], holdout)
            for b, (g, bd) in enumerate(zip(games, sc.boards)):
                if live[b]:
                    ER.begin_ply(sc, g, bd, b, ply, gam)
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s L=%d solver=%d board %d (%s) ply %d start=%s goal=%d" % (sc.name, L, solver, b, sc.boards[b].name, ply, games[b].starts[-1], games[b].goals[-1])
            eng.begin()
            goals = eng.search_goals()
            assert goals.tolist() == [g.goals[-1] if live[b] else 0 for b, g in enumerate(games)], "%s ply %d: goals %s" % (sc.name, ply, goals.tolist())
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search begin", eng, b, g.search.begin_tree, g.search.begin_proven)
            n_steps += _steps(eng, [g.search for g in games], live, modes, "%s ply %d" % (sc.name, ply), sc.S)
            st = eng.check_errors()
            got = tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth"))
            assert got == tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits", "sum_depth")), "%s ply %d: sz_stats" % (sc.name, ply)
            assert st["boards_pending"] == 0 and st["boards_done"] == sum(live)
            assert eng.solver_stats() == (sum(g.proven_stops for g in games), sum(g.proved for g in games)), "%s ply %d: solver counters" % (sc.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search.tree(), g.search.tree_proven())
            u = np.array([sc.boards[b].u(ply) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            rec, ends = eng.fetch_ply(), eng.fetch_endings()
            for b, g in enumerate(games):
                if not live[b]:
                    assert not rec["active"][b] and ends["kind"][b] == NONE and math.isnan(ends["mover_value"][b]), "%s: a board that did not play" % tag(b)
                    continue
                root = FR.position_record(g.game)
                want = g.play(u[b])
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r, restatement %r" % (tag(b), got, want)
                assert int(ends["kind"][b]) == g.last[0] and _same_value(ends["mover_value"][b], g.last[1]), \
                    "%s: sz_fetch_endings kind %d m %r, restatement %r" % (tag(b), ends["kind"][b], ends["mover_value"][b], g.last)
                pos = eng.debug_position(b)[0].tobytes()
                assert pos == FR.position_record(g.game), "%s: position record after sz_play" % tag(b)
                if g.last[0] != NONE:
                    assert pos == root and want["chosen"] == -1 and want["game_over"] == 1, "%s: an ended game keeps its root" % tag(b)
            for b, g in enumerate(games):                       # the sticky marks, live or not
                want_mark = tuple(g.state[3:])
                assert (int(ends["would_ply"][b]), int(ends["would_kind"][b]), int(ends["would_colour"][b])) == want_mark, "%s: holdout mark" % tag(b)
            assert eng.ending_stats() == tuple(sum(g.ended[i] for g in games) for i in range(4)), "%s ply %d: sz_ending_stats" % (sc.name, ply)
            assert eng.forced_stats() == (sum(g.forced_selections for g in games), sum(g.pruned_visits for g in games)), "%s ply %d: sz_forced_stats" % (sc.name, ply)
    es = eng.ending_stats()
    eng.close()
    sims = sum(g.simulations for g in games)
    print("%s L=%d solver=%d: %d plies, %d network steps, %d simulations, %d board searches compared; resignations, draws, proven, marks = %s"
          % (sc.name, L, solver, n_plies, n_steps, sims, sum(len(g.searches) for g in games), es))
    assert n_plies >= 2 and n_steps >= 16 and sims >= 2 * sc.S and st["simulations"] == sims
    for bd, g in zip(sc.boards, games):
        assert ER.role_reached(bd, g, solver), "%s: board %s did not do what it is there for" % (sc.name, bd.name)
    return games, es


@pytest.mark.parametrize("L,solver", ER.OPTIONS)
@pytest.mark.parametrize("name", [sc.name for sc in ER.scenarios()])
def test_whole_games_match_restatement(name, L, solver):
    sc = next(s for s in ER.scenarios() if s.name == name)
    games, es = _drive(sc, L, solver)
    if name == "c960_endings":                                  # a resigning, a draw-adjudicated, a marked holdout and an untouched board, on kept subtrees
        assert es[0] > 0 and es[1] > 0 and es[3] > 0 and es[2] == 0
        assert all(s == "reused" for g in games for s in g.starts[1:])
    elif name == "budgets_endings":
        assert es[0] > 0 and es[3] > 0 and all(s == "new" for g in games for s in g.starts)
    elif name == "proven_endings":                              # WIN (a holdout board), LOSS and DRAW roots; without the solver `proven` is ignored
        assert es == ((0, 0, 3, 0) if solver else (0, 0, 0, 0))
    else:                                                       # proven off: the WIN root's move is played as always; on for ply 1: the kept WIN root ends
        assert es == ((0, 0, 1, 0) if solver else (0, 0, 0, 0))


# ------------------------------------------------------------------------------------------------ 2. the device's decision on seeded cases
def test_device_decision_on_seeded_cases():
    hc = ER.hook_cases()
    n = len(hc.R)
    widths = np.diff(hc.offsets)
    assert n >= 2000 and set(ER.HOOK_K) <= set(widths.tolist())
    assert hc.opts.dtype.itemsize == C.sizeof(N.sz_ending_options) == 28
    kind, m, state, cov = ER.hook_reference(hc)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ins = [dev(x) for x in (hc.offsets, hc.N, hc.W, hc.R, hc.colour, hc.ply, hc.holdout, hc.state, hc.opts)]
    kind_d = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    m_d = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    state_d = torch.full((n, 6), -7, dtype=torch.int32, device="cuda")
    rc = N.lib().sz_debug_endings(*[ptr(t) for t in ins], ptr(kind_d), ptr(m_d), ptr(state_d), n, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == N.SZ_OK
    torch.cuda.synchronize()
    got_kind, got_m, got_state = kind_d.cpu().numpy(), m_d.cpu().numpy(), state_d.cpu().numpy()
    print("hook cases: %d cases, %d children; %s" % (n, len(hc.N), dict(cov)))
    same_m = (np.isnan(got_m) & np.isnan(m)) | (got_m.view(np.uint64) == m.view(np.uint64))
    bad = np.nonzero((got_kind != kind) | ~same_m | (got_state != state).any(axis=1))[0]
    assert not len(bad), "case %d (K = %d): kind %d m %r state %s, restatement %d %r %s" % (
        bad[0], widths[bad[0]], got_kind[bad[0]], got_m[bad[0]], got_state[bad[0]].tolist(), kind[bad[0]], m[bad[0]], state[bad[0]].tolist())
    assert all(cov[k] > 0 for k in ER.HOOK_COVERAGE), dict(cov)
    assert N.lib().sz_debug_endings(None, *[ptr(t) for t in ins[1:]], ptr(kind_d), ptr(m_d), ptr(state_d), n, None) == N.SZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 3. off is off
ARGS = dict(REUSE, num_searches=32, visit_targets=True, root_dirichlet_alpha=0.3)
STARTS = [0, 17, 518]
ALWAYS = options(resign_value=1.0, resign_patience=1, draw_value=1.0, draw_patience=1)      # m <= 1 always: every board resigns at once


def _three_plies(eng, draws, u=(-1.0, 0.3, 0.7), plies=3, before=None):
    """plies with HashModel evaluations and fixed Gamma draws -> per ply (trees at the end of the search, record, positions, endings)"""
    out = []
    for ply in range(plies):
        if before is not None:
            before(ply)
        eng.next_gamma = torch.from_numpy(draws[ply]).cuda()
        eng.search()
        eng.check_errors()
        trees = [eng.debug_tree(b) for b in range(eng.B)]
        eng.play(list(u))
        out.append((trees, eng.fetch_ply(), [eng.debug_position(b)[0].tobytes() for b in range(eng.B)], eng.fetch_endings()))
    return out


def test_off_is_off():
    draws = np.random.default_rng(5).standard_gamma(0.3, size=(3, 3, N.SZ_MAX_MOVES)).astype(np.float32)
    runs = []
    for how in ("never", "on_then_null", "all_rules_off"):
        eng = SelfPlayEngine(HashModel(salt=2), ARGS, 3, chess960=True, learning=True)
        if how == "on_then_null":
            eng.set_endings(ALWAYS, [0, 1, 0])
            eng.set_endings(None)
        if how == "all_rules_off":
            eng.set_endings(options())
        eng.new_games(STARTS)
        runs.append((_three_plies(eng, draws), eng.ending_stats()))
        eng.close()
    (a, sa), (b, sb), (c, sc) = runs
    assert sa == sb == sc == (0, 0, 0, 0)
    for ply in range(3):
        for other in (b, c):
            assert _same(a[ply][0], other[ply][0]), "ply %d: trees" % ply
            assert all(a[ply][1][k].tobytes() == other[ply][1][k].tobytes() for k in a[ply][1]), "ply %d: records" % ply
            assert a[ply][2] == other[ply][2], "ply %d: positions" % ply
        for run in (a, b, c):
            e = run[ply][3]
            assert not e["kind"].any() and (e["would_ply"] == -1).all() and not e["would_kind"].any()
        assert np.isnan(a[ply][3]["mover_value"]).all() and np.isnan(b[ply][3]["mover_value"]).all()      # off: nothing is computed
        assert np.isfinite(c[ply][3]["mover_value"]).all()                                                  # on with every rule off: m is reported
    # ... and the option does something on the same inputs
    eng = SelfPlayEngine(HashModel(salt=2), ARGS, 3, chess960=True, learning=True)
    eng.set_endings(ALWAYS, [0, 1, 0])
    eng.new_games(STARTS)
    (trees, rec, pos, e), = _three_plies(eng, draws, plies=1)
    assert e["kind"].tolist() == [RESIGN, NONE, RESIGN] and e["would_ply"].tolist() == [-1, 0, -1] and e["would_kind"].tolist() == [0, RESIGN, 0]
    assert rec["chosen"][0] == -1 and rec["chosen"][2] == -1 and rec["chosen"][1] == a[0][1]["chosen"][1]
    assert rec["game_over"].tolist() == [1, 0, 1] and rec["result"].tolist() == [-1, 0, -1]                # white to move resigned
    assert _same(trees, a[0][0]) and np.array_equal(rec["visits"], a[0][1]["visits"]) and pos[1] == a[0][2][1]
    assert eng.ending_stats() == (2, 0, 0, 1)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. a new game resets the state
def test_a_new_game_resets_the_state():
    two = {"resign_value": 1.0, "resign_patience": 2}             # m <= 1 always: each colour resigns at its second search
    eng = SelfPlayEngine(HashModel(salt=2), dict(PLAIN, num_searches=32, endings=two), 3, chess960=True, learning=True)
    eng.new_games(STARTS)
    kinds = []

    def ply():
        eng.search()
        eng.check_errors()
        eng.play([-1.0, -1.0, -1.0])
        kinds.append(eng.fetch_endings()["kind"].tolist())
        return eng.fetch_ply()

    ply(), ply()                                                # both colours of every board are one search short of resigning
    assert kinds == [[0, 0, 0], [0, 0, 0]]
    eng.new_games([959, -1, -1], [1, 0, 0])                     # board 0: refilled
    eng.upload_game(1, sz.ChessTensor(chess960=True, scharnagl=100))        # board 1: filled from the host
    rec = ply()
    assert kinds[-1] == [NONE, NONE, RESIGN], "the neighbour that was not refilled resigns, the two new games do not"
    assert rec["game_over"].tolist() == [0, 0, 1] and rec["chosen"][2] == -1 and rec["result"][2] == -1 and rec["colour"][2] == 1
    ply()                                                       # black's first search of the two new games
    rec = ply()                                                 # white's second: now they resign, at their own ply 2
    assert kinds[-2:] == [[NONE, NONE, NONE], [RESIGN, RESIGN, NONE]] and rec["active"].tolist() == [1, 1, 0]
    assert eng.ending_stats() == (3, 0, 0, 0)
    eng.set_active([1, 1, 1])                                   # sz_set_active does not reset anything: nothing to observe but no error
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. setter rules
def test_setter_rules():
    lib = N.lib()
    O = lambda **kw: N.sz_ending_options(*[options(**kw)[k] for k in ER.KEYS])
    eng = SelfPlayEngine(HashModel(salt=2), ARGS, 3, chess960=True, learning=True)
    s = eng._stream()
    nan, inf = float("nan"), float("inf")
    bad = [dict(resign_value=1.5), dict(resign_value=-1.5), dict(draw_value=-0.25), dict(draw_value=1.5),
           dict(resign_patience=-1), dict(resign_patience=65536), dict(draw_patience=-1), dict(draw_patience=65536), dict(resign_min_ply=-1), dict(draw_min_ply=-1)]
    for kw in bad:
        assert lib.sz_set_endings(eng._e, C.byref(O(**kw)), None, s) == N.SZ_ERR_INVALID, kw
    for field in ("resign_value", "draw_value"):
        for v in (nan, inf, -inf):
            o = O()
            setattr(o, field, v)
            assert lib.sz_set_endings(eng._e, C.byref(o), None, s) == N.SZ_ERR_INVALID, (field, v)
    assert lib.sz_set_endings(None, C.byref(O()), None, s) == N.SZ_ERR_INVALID
    assert lib.sz_ending_stats(eng._e, None, s) == N.SZ_ERR_INVALID and lib.sz_fetch_endings(None, None, None, None, None, None, s) == N.SZ_ERR_INVALID
    assert lib.sz_set_endings(eng._e, C.byref(O(resign_value=-1.0, resign_patience=65535, draw_value=1.0, draw_patience=65535)), None, s) == N.SZ_OK
    assert eng.ending_stats() == (0, 0, 0, 0) and eng.fetch_endings()["would_ply"].tolist() == [-1, -1, -1]
    with pytest.raises(ValueError):
        eng.set_endings(options(), [1])                          # one flag for three boards
    eng.close()

    # during a search: refused and nothing changes; a call that changes `holdout` only keeps the subtrees and the streaks
    draws = np.random.default_rng(6).standard_gamma(0.3, size=(5, 3, N.SZ_MAX_MOVES)).astype(np.float32)
    three = options(resign_value=1.0, resign_patience=3)        # m <= 1 always: white's third search, at ply 4, resigns
    runs = []
    for meddle in (False, True):
        eng = SelfPlayEngine(HashModel(salt=2), ARGS, 3, chess960=True, learning=True)
        eng.set_endings(three, [0, 0, 0])
        eng.new_games(STARTS)
        s = eng._stream()
        out = []
        for ply in range(5):
            if meddle and ply >= 1:
                eng.set_endings(three, [0, 1, 0])               # the same options, a new holdout array, before every ply
            eng.next_gamma = torch.from_numpy(draws[ply]).cuda()
            eng.begin()
            goals = eng.search_goals().tolist()
            if meddle and ply == 2:                             # mid-search: SZ_ERR_STATE, for new options and for off alike
                assert eng.pending_boards() > 0
                assert lib.sz_set_endings(eng._e, C.byref(O(**ALWAYS)), None, s) == N.SZ_ERR_STATE
                assert lib.sz_set_endings(eng._e, None, None, s) == N.SZ_ERR_STATE
            for _ in range(32):
                eng.step(*eng.evaluate(eng.planes))
            assert eng.check_errors()["boards_pending"] == 0
            trees = [eng.debug_tree(b) for b in range(3)]
            eng.play([-1.0, 0.3, 0.7])
            out.append((trees, eng.fetch_ply(), eng.fetch_endings(), goals))
        runs.append((out, eng.ending_stats()))
        eng.close()
    (a, sa), (b, sb) = runs
    for ply in range(5):
        assert a[ply][3] == b[ply][3] and _same(a[ply][0], b[ply][0]), "ply %d: trees (a kept subtree was dropped, or the refused call changed something)" % ply
        assert a[ply][2]["kind"].tolist() == ([RESIGN] * 3 if ply == 4 else [NONE] * 3), "ply %d" % ply
        assert b[ply][2]["kind"].tolist() == ([RESIGN, NONE, RESIGN] if ply == 4 else [NONE] * 3), "ply %d: the streaks survive the holdout-only calls" % ply
        for k in ("packed", "action", "visits", "n_child", "colour"):
            assert a[ply][1][k].tobytes() == b[ply][1][k].tobytes(), "ply %d: records" % ply
    assert all(min(a[ply][3]) < 32 for ply in range(1, 5)), "the plies after the first continue on kept subtrees: %r" % [x[3] for x in a]
    assert sa == (3, 0, 0, 0) and sb == (2, 0, 0, 1)
    assert b[4][2]["would_ply"].tolist() == [-1, 4, -1] and b[4][1]["chosen"][1] >= 0 and b[4][1]["game_over"][1] == 0


# ------------------------------------------------------------------------------------------------ 6. play_games end to end
def test_play_games_end_to_end():
    from sigma_zero_amd.sim import play_games, ending_report
    KIND = {RESIGN: "resign", DRAW_ADJ: "draw_adjudicated", PROVEN: "proven"}
    endings = {"resign_value": -0.1, "resign_patience": 1, "resign_min_ply": 1, "holdout": 0.5}
    args = {"C": 2, "num_searches": 32, "endings": endings}
    starts, caps, held, salt = [0, 959, 518, 400, 77], [6, 4, 5, 6, 3], [False, False, True, False, False], 4
    stats = {}
    got = play_games(HashModel(salt=salt), args, 5, c960=True, scharnagl=starts, uniforms=lambda g, ply: -1.0, holdout=lambda g: held[g],
                     max_plies=caps, learning=True, n_boards=2, stats=stats)
    opts = options(**{k: v for k, v in endings.items() if k != "holdout"})
    want_stats = [0, 0, 0, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for g, (n, cap) in enumerate(zip(starts, caps)):
            ref = ER.Game(sz.ChessTensor(chess960=True, scharnagl=n), 32, None, reuse=False, c=2.0, learning=True, mode="dyadic", salt=salt)
            ref.set_endings(opts, held[g])                      # a refilled slot starts clean: the restatement's game starts from FRESH
            recs = []
            while ref.live and len(ref.chosen) < cap:
                ref.begin()
                ref.run()
                recs.append(ref.play(-1.0))
            want_stats = [a + b for a, b in zip(want_stats, ref.ended)]
            term = KIND[ref.termination] if ref.termination is not None else ("rules" if ref.over else "max_plies")
            mark = None if ref.state.would_ply < 0 else {"kind": KIND[ref.state.would_kind], "ply": ref.state.would_ply, "colour": ref.state.would_colour}
            tag = "game %d (start %d)" % (g, n)
            assert (got[g]["termination"], got[g]["would_end"], got[g]["holdout"]) == (term, mark, held[g]), "%s: %r %r, restatement %r %r" % (
                tag, got[g]["termination"], got[g]["would_end"], term, mark)
            assert got[g]["chosen_actions"] == ref.chosen and len(got[g]["chosen_actions"]) == len(recs) - (ref.termination is not None), tag
            assert got[g]["sample_plies"] == list(range(len(recs))) and len(got[g]["states"]) == len(recs), "%s: the ending ply is a sample" % tag
            result = {1: "1-0", -1: "0-1", 0: "1/2-1/2"}[ref.result] if ref.over else None
            reward = {"1-0": 1, "0-1": -1}.get(result, 0)
            assert got[g]["result"] == result and got[g]["rewards"] == [reward if p % 2 == 0 else -reward for p in got[g]["sample_plies"]], tag
            last = recs[-1]["visits"][:recs[-1]["n_child"]].astype(np.int64)
            assert list(got[g]["actions"][-1].values()) == (last / int(last.sum())).tolist(), tag
    terms = [g["termination"] for g in got]
    print("play_games:", terms, [g["would_end"] for g in got], {k: stats[k] for k in ("plies", "resigned", "adjudicated_draws", "adjudicated_proven", "holdout_games", "holdout_marks")})
    assert terms.count("resign") >= 2 and terms.count("max_plies") >= 2 and got[2]["would_end"] is not None and got[2]["termination"] == "max_plies"
    assert [stats[k] for k in ("resigned", "adjudicated_draws", "adjudicated_proven", "holdout_marks")] == want_stats and stats["holdout_games"] == 1
    r = ending_report(got)
    assert r["games"] == 5 and r["resigned"] == stats["resigned"] == terms.count("resign") and r["holdout_games"] == 1 and r["holdout_marks"] == stats["holdout_marks"] == 1
    assert r["resigned"] + r["adjudicated_draws"] + r["adjudicated_proven"] + r["rules"] + r["max_plies"] == 5
    assert r["resign_marks"] == 1 and r["resign_false_positives"] == 1        # the marked game was cut at max_plies: the marked colour did not lose
    off = {}
    plain = play_games(HashModel(salt=salt), {"C": 2, "num_searches": 32}, 1, c960=True, scharnagl=[0], uniforms=lambda g, ply: -1.0, max_plies=2, learning=True, stats=off)
    assert plain[0]["termination"] == "max_plies" and plain[0]["would_end"] is None and off["resigned"] == 0 and off["holdout_games"] == 0
    with pytest.raises(ValueError):
        play_games(HashModel(salt=salt), {"C": 2, "num_searches": 32}, 1, holdout=lambda g: True)
