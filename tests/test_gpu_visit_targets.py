"""Subtree reuse as a self-play configuration on the GPU (sz_set_visit_targets / sz_search_goals / sz_set_search_root_noise,
args["visit_targets"], NON-REFERENCE options): the HIP engine against the plain-Python restatement tests/targetref.py, bit for bit and ply
after ply — whole trees with their priors at search begin and end, the goals, every network input row of every step, step counts,
counters, training records, the position after sz_play — plus in-search shrinking planned from the goals, the setter rules and the Python
surface.  tests/test_target_ref.py proves on the CPU that the scenarios reach the conditions they are there for; the same counters are
asserted here on the games the device was compared with."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine, search_segments
from hashmodel import HashModel, evaluate_packed, pack_planes
import targetref as TR

pytestmark = pytest.mark.gpu

ST_PENDING, ST_ERROR = 2, 16
REUSE = {"combine_options": True, "reuse_subtree": True, "C": 2, "num_searches": 64}


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


# ------------------------------------------------------------------------------------------------ 1. whole games against the restatement
_played = []


def _drive(sc, L, solver):
    B = len(sc.boards)
    eng = SelfPlayEngine(None, dict(REUSE, num_searches=sc.S, solver=solver, leaves_per_step=L), B, chess960=sc.c960, learning=sc.learning,
                         edges_per_board=sc.edges_per_board)
    games = [TR.new_game(sc, bd, L, solver) for bd in sc.boards]
    modes = [(bd.mode, bd.salt) for bd in sc.boards]
    gam = TR.gammas(sc)
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    n_plies = n_steps = 0                                       # what was actually driven and compared (asserted below: no vacuous pass)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(sc.plies):
            live = [g.live for g in games]
            if not any(live):
                break
            n_plies += 1
            eng.set_visit_targets([bd.targets[ply] if live[b] else 0 for b, bd in enumerate(sc.boards)])
            eng.set_search_root_noise(torch.from_numpy(gam[ply]) if sc.noise[ply] else None, [bd.quiet[ply] for bd in sc.boards])
            for b, (g, bd) in enumerate(zip(games, sc.boards)):
                if live[b]:
                    TR.begin_ply(sc, g, bd, b, ply, gam)
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s L=%d solver=%d board %d (%s) ply %d start=%s goal=%d" % (sc.name, L, solver, b, sc.boards[b].name, ply, games[b].starts[-1], games[b].goals[-1])
            eng.begin()
            goals = eng.search_goals()                                  # synchronises
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
            rec = eng.fetch_ply()
            for b, g in enumerate(games):
                if not live[b]:
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tag(b)
                    continue
                want = g.play(u[b])
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r" % (tag(b), got)
                assert eng.debug_position(b)[0].tobytes() == TR.position_record(g.game), "%s: position record of the new root" % tag(b)
    eng.close()
    sims = sum(g.simulations for g in games)
    print("%s L=%d solver=%d: %d plies, %d network steps, %d simulations, %d board searches compared" % (sc.name, L, solver, n_plies, n_steps, sims, sum(len(g.searches) for g in games)))
    assert n_plies >= 3 and n_steps >= 16 and sims >= 3 * sc.S and st["simulations"] == sims
    return games


@pytest.mark.parametrize("L,solver", TR.OPTIONS)
@pytest.mark.parametrize("name", [sc.name for sc in TR.scenarios()])
def test_whole_games_match_restatement(name, L, solver):
    sc = next(s for s in TR.scenarios() if s.name == name)
    games = _drive(sc, L, solver)
    for bd, g in zip(sc.boards, games):
        for ply, s in enumerate(g.searches):
            assert int(s.N[0]) == max(g.kept_visits[ply], 1 + bd.targets[ply])
    _played.append((sc, games))


def test_whole_games_coverage():
    """counted on the restatement, over the games the device was compared with (all of them replayed when this test runs alone)"""
    played = _played
    if not played:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            played = [(sc, TR.play(sc, L, solver)) for sc in TR.scenarios() for L, solver in TR.OPTIONS]
    cov = TR.coverage(played)
    print("coverage:", dict(cov))
    assert all(cov[k] >= 1 for k in TR.COVERAGE), dict(cov)


# ------------------------------------------------------------------------------------------------ 2. in-search shrinking planned from the goals
def _expected_rows(goals, L, max_shrinks, n_rows):
    """network rows of SelfPlayEngine.search at L = 1: per segment of search_segments(goals) the boards whose goal reaches into it"""
    segs, need, lo, rows = search_segments(goals, L, max_shrinks, 64), np.asarray(goals), 0, 0
    for n in segs:
        rows += n * (int((need > lo).sum()) if max_shrinks > 0 else n_rows)
        lo += n
    return rows


def test_shrinking_follows_the_goals_and_does_not_change_results():
    starts = [0, 17, 518, 959, 333, 702, 77, 5]
    second = [8, 64, 8, 16, 64, 2, 32, 8]                              # ply 1's targets after a full ply 0; greedy play keeps the largest subtree
    trees, rows = {}, {}
    for max_shrinks in (3, 0):
        eng = SelfPlayEngine(HashModel(salt=0), dict(REUSE, visit_targets=True, max_shrinks=max_shrinks), 8, chess960=True, learning=False)
        games = [TR.Game(sz.ChessTensor(chess960=True, scharnagl=n), 64, TR.worst_case(64), reuse=True, c=2.0, learning=False, mode="dyadic", salt=0) for n in starts]
        for b, g in enumerate(games):
            eng.upload_game(b, g.game)
        for ply, targets in enumerate(([64] * 8, second)):
            eng.set_visit_targets(targets)
            eng.search()
            eng.check_errors()
            for g, t in zip(games, targets):
                g.begin(t)
                g.run()
            goals = [g.goals[-1] for g in games]
            assert eng.last_goals.tolist() == goals
            assert eng.last_rows == _expected_rows(goals, 1, max_shrinks, 8), "network rows: %d, goals %s" % (eng.last_rows, goals)
            assert eng.last_steps == max(goals)
            for b, g in enumerate(games):
                _assert_tree("max_shrinks=%d ply %d board %d" % (max_shrinks, ply, b), eng, b, g.search.tree(), g.search.tree_proven())
            if ply == 0:
                eng.play([-1.0] * 8)
                for g in games:
                    g.play(-1.0)
        assert min(goals) == 0 and len(set(goals)) >= 4, goals        # a board done at begin, several distinct segment ends
        trees[max_shrinks], rows[max_shrinks] = [eng.debug_tree(b) for b in range(8)], eng.last_rows
        eng.close()
    assert rows[3] < rows[0] == 8 * max(goals)                      # planned from the goals a board with goal 0 never takes a row; unplanned every board every step
    for b in range(8):
        for x, y in zip(trees[3][b], trees[0][b]):
            assert x.tobytes() == y.tobytes(), "board %d: results depend on the shrinking" % b


def test_all_boards_done_at_begin_make_no_network_call():
    eng = SelfPlayEngine(HashModel(salt=0), dict(REUSE, visit_targets=True), 2, chess960=True, learning=False)
    eng.new_games([0, 17])
    eng.search()
    before = eng.check_errors()["simulations"]
    kept = [int(eng.root_children()[1][b].max()) for b in range(2)]       # greedy: the most visited child is the next root
    eng.play([-1.0, -1.0])
    eng.set_visit_targets([min(kept) - 1] * 2)
    eng.search()
    st = eng.check_errors()
    assert eng.last_goals.tolist() == [0, 0] and eng.last_steps == 0 and eng.last_rows == 0 and st["simulations"] == before and st["boards_done"] == 2
    eng.play([0.5, 0.5])                                                 # sampled from the kept visit counts
    rec = eng.fetch_ply()
    assert rec["active"].tolist() == [1, 1] and [int(rec["visits"][b].sum()) for b in range(2)] == [k - 1 for k in kept]
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. setter rules
def _trees(eng, n):
    return [eng.debug_tree(b) for b in range(n)]


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def test_without_reuse_the_new_setters_equal_the_old_ones():
    starts, t = [0, 17, 518, 959], [64, 1, 0, 23]
    g = torch.Generator(device="cuda").manual_seed(7)
    gamma = torch._standard_gamma(torch.full((4, N.SZ_MAX_MOVES), 0.3, device="cuda"), generator=g)
    out = []
    for new in (False, True):
        eng = SelfPlayEngine(HashModel(salt=3), {"C": 2, "num_searches": 64}, 4, chess960=True, learning=True)
        eng.new_games(starts)
        if new:
            eng.set_visit_targets(t)
            eng.set_search_root_noise(gamma)
        else:
            eng.set_budgets(t)
            eng.set_root_noise(gamma)
        eng.search()
        st = eng.check_errors()
        out.append((_trees(eng, 4), st, eng.search_goals().tolist()))
        eng.close()
    assert _same(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert out[0][2] == out[1][2] == t                                   # sz_search_goals reads budgets as well
    assert [int(tr[2][0]) for tr in out[1][0]] == [1 + x for x in t]


def test_targets_and_budgets_exclude_each_other_the_later_call_wins():
    eng = SelfPlayEngine(HashModel(salt=1), {"C": 2, "num_searches": 32}, 2, learning=False)
    root_visits = lambda: [int(eng.debug_tree(b)[2][0]) for b in range(2)]
    for call, want in ((lambda: eng.set_budgets([5, 9]), [6, 10]), (lambda: eng.set_visit_targets([20, 3]), [21, 4]), (lambda: eng.set_budgets([7, 7]), [8, 8]),
                       (lambda: eng.set_visit_targets([11, 12]), [12, 13]), (lambda: eng.set_visit_targets(None), [33, 33]),
                       (lambda: (eng.set_visit_targets([4, 4]), eng.set_budgets(None)), [33, 33])):
        call()
        eng.new_games()
        eng.search()
        eng.check_errors()
        assert root_visits() == want
        assert eng.search_goals().tolist() == [w - 1 for w in want]
    eng.close()


def test_range_and_state_errors_and_old_setters_still_refuse_on_a_reuse_engine():
    lib = N.lib()
    arr = lambda *v: (C.c_int32 * len(v))(*v)
    for reuse in (False, True):
        eng = SelfPlayEngine(HashModel(salt=0), dict(REUSE, num_searches=16) if reuse else {"C": 2, "num_searches": 16}, 2, learning=True)
        s = eng._stream()
        for bad in ((-1, 4), (4, 17)):
            assert lib.sz_set_visit_targets(eng._e, arr(*bad), s) == N.SZ_ERR_INVALID
        assert lib.sz_set_visit_targets(eng._e, arr(0, 16), s) == N.SZ_OK
        assert lib.sz_search_goals(eng._e, None, s) == N.SZ_ERR_INVALID
        gamma = torch.ones(2, N.SZ_MAX_MOVES, device="cuda")
        eng.new_games()
        eng.set_visit_targets([16, 16])
        eng.begin()
        assert lib.sz_set_visit_targets(eng._e, arr(3, 3), s) == N.SZ_ERR_STATE              # during a search: refused, nothing changes
        assert lib.sz_set_visit_targets(eng._e, None, s) == N.SZ_ERR_STATE
        assert lib.sz_set_search_root_noise(eng._e, C.c_void_p(gamma.data_ptr()), None, s) == N.SZ_ERR_STATE
        for _ in range(16):
            eng.step(*eng.evaluate(eng.planes))
        st = eng.check_errors()
        assert st["boards_done"] == 2 and [int(eng.debug_tree(b)[2][0]) for b in range(2)] == [17, 17]
        if reuse:
            assert lib.sz_set_search_budgets(eng._e, arr(4, 4), s) == N.SZ_ERR_INVALID        # the old refusals stand
            assert lib.sz_set_root_noise(eng._e, C.c_void_p(gamma.data_ptr())) == N.SZ_ERR_STATE
            assert lib.sz_set_search_root_noise(eng._e, C.c_void_p(gamma.data_ptr()), None, s) == N.SZ_OK
            assert lib.sz_set_root_noise(eng._e, None) == N.SZ_ERR_STATE                       # this mode is left through its own setter
            assert lib.sz_set_search_root_noise(eng._e, None, None, s) == N.SZ_OK
            assert lib.sz_set_root_noise(eng._e, None) == N.SZ_OK
        else:
            assert lib.sz_set_search_budgets(eng._e, arr(4, 4), s) == N.SZ_OK
            assert lib.sz_set_root_noise(eng._e, C.c_void_p(gamma.data_ptr())) == N.SZ_OK
        eng.close()


# ------------------------------------------------------------------------------------------------ 4. Python surface
KEYS = {"C": 2, "num_searches": 32, "reuse_subtree": True, "visit_targets": True, "playout_cap": {"fast": 6, "p_full": 0.4},
        "root_dirichlet_alpha": 0.3, "quiet_fast_plies": True}


def test_play_games_records_do_not_depend_on_the_slots():
    from sigma_zero_amd.sim import play_games
    n_games = 6
    draws = np.random.default_rng(11).standard_gamma(0.3, size=(n_games, 16, N.SZ_MAX_MOVES)).astype(np.float32)
    kw = dict(c960=True, scharnagl=[0, 17, 518, 959, 333, 702], uniforms=lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0,
              full_search=lambda g, ply: (g + ply) % 3 == 0, root_gamma=lambda g, ply: draws[g, ply], max_plies=[5, 7, 4, 8, 6, 5], learning=True)
    runs, stats = [], []
    for n_boards in (2, 6):
        stats.append({})
        runs.append(play_games(HashModel(salt=4), KEYS, n_games, n_boards=n_boards, stats=stats[-1], **kw))
    for g, (a, b) in enumerate(zip(*runs)):
        assert a["chosen_actions"] == b["chosen_actions"] and len(a["chosen_actions"]) == kw["max_plies"][g], "game %d: moves played" % g
        assert a["sample_plies"] == b["sample_plies"] == [p for p in range(kw["max_plies"][g]) if (g + p) % 3 == 0], "game %d" % g
        assert a["actions"] == b["actions"] and a["colours"] == b["colours"] and a["rewards"] == b["rewards"], "game %d: samples" % g
        assert all(np.array_equal(x, y) for x, y in zip(a["packed_states"], b["packed_states"])), "game %d" % g
    print("play_games:", [(st["plies"], st["sims"], st["nn_rows"], st["full_plies"], st["fast_plies"], st["searches_without_network"]) for st in stats])
    for st in stats:
        assert st["full_plies"] + st["fast_plies"] == sum(kw["max_plies"]) and st["full_plies"] > 0 and st["fast_plies"] > 0
        assert st["sims"] == stats[0]["sims"] and st["fast_plies"] == stats[0]["fast_plies"] and st["full_plies"] == stats[0]["full_plies"]
        assert 0 < st["sims"] < 32 * st["full_plies"] + 6 * st["fast_plies"]                   # kept visits counted: fewer new simulations than the targets
        assert st["nn_rows"] > 0 and "searches_without_network" in st


def test_old_key_combinations_raise_as_before():
    from sigma_zero_amd.sim import play_games, playout_cap_of
    old = {k: v for k, v in KEYS.items() if k not in ("visit_targets", "quiet_fast_plies")}
    with pytest.raises(ValueError):
        playout_cap_of(old)
    with pytest.raises(ValueError):
        play_games(HashModel(), old, 1)
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {k: v for k, v in old.items() if k != "playout_cap"}, 1)
    assert playout_cap_of(KEYS) == (6, 0.4)
    for missing in ("visit_targets", "playout_cap", "root_dirichlet_alpha"):
        with pytest.raises(ValueError):
            SelfPlayEngine(None, {k: v for k, v in KEYS.items() if k != missing}, 1)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            SelfPlayEngine(None, dict(KEYS, visit_targets=bad), 1)
    eng = SelfPlayEngine(None, KEYS, 2)
    assert eng.targets.tolist() == [32, 32]                              # without a per-ply call every board's target is num_searches
    eng.close()
