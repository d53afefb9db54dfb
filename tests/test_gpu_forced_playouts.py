"""Forced playouts and policy-target pruning on the GPU (sz_set_forced_playouts / sz_forced_stats / sz_debug_forced,
args["forced_playouts"], a NON-REFERENCE option): the HIP engine against the plain-Python restatement tests/forcedref.py, bit for bit and
ply after ply — whole trees at search begin and end with the counted visits, every network input row of every step, step counts, the
counters, the training records with the pruned visits, the position after sz_play — plus the device's selection and pruning functions on
seeded cases, off is off, the setter rules and the Python surface.  tests/test_forced_ref.py proves on the CPU that the scenarios and hook
cases reach the conditions they are there for; the same counters are asserted here on the games the device was compared with."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine, forced_playout_options_of
from hashmodel import HashModel, evaluate_packed, pack_planes
import forcedref as FR

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


# ------------------------------------------------------------------------------------------------ 1. whole games against the restatement
_played = []


def _drive(sc, L, solver):
    B = len(sc.boards)
    eng = SelfPlayEngine(None, dict(REUSE if sc.reuse else PLAIN, num_searches=sc.S, solver=solver, leaves_per_step=L), B, chess960=sc.c960,
                         learning=sc.learning, edges_per_board=sc.edges_per_board or 0)
    games = [FR.new_game(sc, bd, L, solver) for bd in sc.boards]
    modes = [(bd.mode, bd.salt) for bd in sc.boards]
    gam = FR.gammas(sc)
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
            numbers = [bd.targets[ply] if live[b] else 0 for b, bd in enumerate(sc.boards)]
            if sc.reuse:
                eng.set_visit_targets(numbers)
            else:
                eng.set_budgets(numbers)
            eng.set_search_root_noise(torch.from_numpy(gam[ply]) if sc.noise[ply] else None, [bd.quiet[ply] for bd in sc.boards])
            eng.set_forced_playouts(sc.k[ply], [bd.forced[ply] for bd in sc.boards])
            for b, (g, bd) in enumerate(zip(games, sc.boards)):
                if live[b]:
                    FR.begin_ply(sc, g, bd, b, ply, gam)
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s L=%d solver=%d board %d (%s) ply %d start=%s goal=%d k=%g" % (
                sc.name, L, solver, b, sc.boards[b].name, ply, games[b].starts[-1], games[b].goals[-1], games[b].forced_plies[-1])
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
            assert eng.forced_stats()[0] == sum(g.forced_selections for g in games), "%s ply %d: forced selections" % (sc.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search.tree(), g.search.tree_proven())
            u = np.array([sc.boards[b].u(ply) if live[b] else 0.0 for b in range(B)], np.float64)
            counted = eng.root_children()[1]                            # before sz_play: the counted visits
            eng.play(u)
            rec = eng.fetch_ply()
            for b, g in enumerate(games):
                if not live[b]:
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tag(b)
                    continue
                vis = g.search.root_children()[1]
                assert counted[b, :len(vis)].tolist() == vis.tolist(), "%s: sz_root_children shows the counted visits" % tag(b)
                want = g.play(u[b])
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, pruned visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r" % (tag(b), got)
                assert eng.debug_position(b)[0].tobytes() == FR.position_record(g.game), "%s: position record of the new root" % tag(b)
            assert eng.forced_stats() == (sum(g.forced_selections for g in games), sum(g.pruned_visits for g in games)), "%s ply %d: sz_forced_stats" % (sc.name, ply)
    fs = eng.forced_stats()
    eng.close()
    sims = sum(g.simulations for g in games)
    print("%s L=%d solver=%d: %d plies, %d network steps, %d simulations, %d board searches compared, %d forced selections, %d visits pruned"
          % (sc.name, L, solver, n_plies, n_steps, sims, sum(len(g.searches) for g in games), fs[0], fs[1]))
    assert n_plies >= 3 and n_steps >= 16 and sims >= 3 * sc.S and st["simulations"] == sims
    assert fs[0] > 0 and fs[1] > 0
    return games


@pytest.mark.parametrize("L,solver", FR.OPTIONS)
@pytest.mark.parametrize("name", [sc.name for sc in FR.scenarios()])
def test_whole_games_match_restatement(name, L, solver):
    sc = next(s for s in FR.scenarios() if s.name == name)
    games = _drive(sc, L, solver)
    if sc.reuse:                                                # k and `boards` change between plies: the kept subtrees are not dropped
        g = games[0]
        changes = [p for p in range(1, len(g.starts)) if sc.k[p] != sc.k[p - 1]]
        assert changes and all(g.starts[p] == "reused" for p in changes), g.starts
    else:
        assert all(s == "new" for g in games for s in g.starts)
    _played.append((sc, games))


def test_whole_games_coverage():
    """counted on the restatement, over the games the device was compared with (all of them replayed when this test runs alone)"""
    played = _played
    if not played:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            played = [(sc, FR.play(sc, L, solver)) for sc in FR.scenarios() for L, solver in FR.OPTIONS]
    cov = FR.coverage(played)
    print("coverage:", dict(cov))
    assert all(cov[k] >= 1 for k in FR.COVERAGE if k not in ("wide_case", "forced_win_skipped")), dict(cov)      # those two: the hook cases below


# ------------------------------------------------------------------------------------------------ 2. the device functions on seeded cases
def _debug_forced(hc):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    n, total = len(hc.parent), len(hc.N)
    ins = [dev(x) for x in (hc.offsets, hc.N, hc.K, hc.W, hc.P)]
    R = None if hc.R is None else dev(hc.R)
    tail = [dev(x) for x in (hc.parent, hc.c, hc.fk)]
    outs = [torch.full((m,), -7, dtype=torch.int32, device="cuda") for m in (n, n, total, n)]
    rc = N.lib().sz_debug_forced(*[ptr(t) for t in ins], None if R is None else ptr(R), *[ptr(t) for t in tail], C.c_float(hc.lam),
                                 *[ptr(t) for t in outs], n, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == N.SZ_OK
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize("solver", [False, True])
def test_device_selection_and_pruning_on_seeded_cases(solver):
    hc = FR.hook_cases(solver=solver)
    widths = np.diff(hc.offsets)
    assert len(widths) >= 2000 and set(FR.HOOK_K) <= set(widths.tolist())
    sel, frc, pruned, cst, cov = FR.hook_reference(hc)
    got = _debug_forced(hc)
    print("hook cases solver=%d: %d cases, %d children, %d decided by a forced child, %d visits pruned; %s"
          % (solver, len(widths), len(hc.N), int(frc.sum()), int((hc.N - pruned).sum()), dict(cov)))
    bad = np.nonzero((got[0] != sel) | (got[1] != frc) | (got[3] != cst))[0]
    assert not len(bad), "case %d (K = %d): selected %d forced %d c* %d, restatement %d %d %d" % (
        bad[0], widths[bad[0]], got[0][bad[0]], got[1][bad[0]], got[3][bad[0]], sel[bad[0]], frc[bad[0]], cst[bad[0]])
    assert np.array_equal(got[2], pruned), "pruned counts differ at flat child %d" % int(np.nonzero(got[2] != pruned)[0][0])
    assert cov["wide_case"] > 0 and cov["wide_pruned"] > 0 and cov["several_forced"] > 0 and cov["forced_in_flight"] > 0 and cov["tied_with_best_later"] > 0
    assert cov["forced_win_skipped"] > 0 if solver else cov["forced_win_skipped"] == 0


# ------------------------------------------------------------------------------------------------ 3. off is off, setter rules
ARGS = dict(REUSE, num_searches=32, visit_targets=True, root_dirichlet_alpha=0.3)
STARTS = [0, 17, 518]


def _three_plies(eng, draws, between=None):
    """three plies with HashModel evaluations and fixed Gamma draws -> (trees at the end of every search, records)"""
    eng.new_games(STARTS)
    trees, recs = [], []
    for ply in range(3):
        if between is not None:
            between(ply)
        eng.next_gamma = torch.from_numpy(draws[ply]).cuda()
        eng.search()
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(eng.B)])
        eng.play([-1.0, 0.3, 0.7])
        recs.append(eng.fetch_ply())
    return trees, recs


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def test_switched_on_and_off_again_equals_never_switched_on():
    draws = np.random.default_rng(5).standard_gamma(0.3, size=(3, 3, N.SZ_MAX_MOVES)).astype(np.float32)
    out = []
    for touch in (False, True, "forced"):
        eng = SelfPlayEngine(HashModel(salt=2), ARGS, 3, chess960=True, learning=True)
        if touch:
            eng.set_forced_playouts(2.0, [1, 0, 1])
            if touch is True:
                eng.set_forced_playouts(0)
        out.append(_three_plies(eng, draws) + (eng.forced_stats(),))
        eng.close()
    (t0, r0, f0), (t1, r1, f1), (t2, r2, f2) = out
    assert f0 == f1 == (0, 0) and f2[0] > 0 and f2[1] > 0
    for ply in range(3):
        assert _same(t0[ply], t1[ply]), "ply %d: trees" % ply
        assert all(r0[ply][k].tobytes() == r1[ply][k].tobytes() for k in r0[ply]), "ply %d: records" % ply
    # ... and the option does something on the same inputs: board 1, whose bit is off, is untouched on the first ply; boards 0 and 2 are not both
    assert _same([t0[0][1]], [t2[0][1]]) and not (_same([t0[0][0]], [t2[0][0]]) and _same([t0[0][2]], [t2[0][2]]))
    assert np.array_equal(r0[0]["visits"][1], r2[0]["visits"][1])


def test_setter_rules():
    lib = N.lib()
    draws = np.random.default_rng(6).standard_gamma(0.3, size=(3, 3, N.SZ_MAX_MOVES)).astype(np.float32)
    mask = lambda *v: (C.c_uint8 * len(v))(*v)
    results = []
    for meddle in (False, True):
        eng = SelfPlayEngine(HashModel(salt=2), dict(ARGS, forced_playouts=2.0), 3, chess960=True, learning=True)
        s = eng._stream()
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert lib.sz_set_forced_playouts(eng._e, C.c_float(bad), None, s) == N.SZ_ERR_INVALID
        assert lib.sz_forced_stats(eng._e, None, s) == N.SZ_ERR_INVALID
        eng.new_games(STARTS)
        eng.next_gamma = torch.from_numpy(draws[0]).cuda()
        eng.begin()
        if meddle:                                                   # during a search: refused, nothing changes
            assert lib.sz_set_forced_playouts(eng._e, C.c_float(0.0), None, s) == N.SZ_ERR_STATE
            assert lib.sz_set_forced_playouts(eng._e, C.c_float(64.0), mask(0, 0, 1), s) == N.SZ_ERR_STATE
        for _ in range(32):
            eng.step(*eng.evaluate(eng.planes))
        assert eng.check_errors()["boards_done"] == 3
        trees = [eng.debug_tree(b) for b in range(3)]
        if meddle:                                                   # between the search and its sz_play: accepted, and that sz_play is not changed
            assert lib.sz_set_forced_playouts(eng._e, C.c_float(0.0), None, s) == N.SZ_OK
        eng.play([-1.0, 0.3, 0.7])
        results.append((trees, eng.fetch_ply(), eng.forced_stats()))
        eng.close()
    (ta, ra, fa), (tb, rb, fb) = results
    assert _same(ta, tb) and fa == fb and fa[0] > 0 and fa[1] > 0
    assert all(ra[k].tobytes() == rb[k].tobytes() for k in ra)
    # without `learning`: refused, by the library and by the Python surface; switching off is always accepted
    eng = SelfPlayEngine(HashModel(salt=2), dict(REUSE, num_searches=8), 2, learning=False)
    assert lib.sz_set_forced_playouts(eng._e, C.c_float(2.0), None, eng._stream()) == N.SZ_ERR_INVALID
    assert lib.sz_set_forced_playouts(eng._e, C.c_float(0.0), None, eng._stream()) == N.SZ_OK
    with pytest.raises(ValueError):
        eng.set_forced_playouts(2.0, [1])                            # one flag for two boards
    eng.close()
    with pytest.raises(ValueError):
        SelfPlayEngine(None, dict(REUSE, forced_playouts=2.0), 1, learning=False)


# ------------------------------------------------------------------------------------------------ 4. Python surface
def test_forced_playout_options_of_validates():
    assert forced_playout_options_of({}) is None and forced_playout_options_of({"forced_playouts": 2}) == 2.0
    assert forced_playout_options_of({"forced_playouts": np.float32(0.5)}) == 0.5
    for bad in (True, False, float("nan"), float("inf"), -1.0, 0, 0.0, "2", [2.0]):
        with pytest.raises(ValueError):
            forced_playout_options_of({"forced_playouts": bad})


KEYS = {"C": 2, "num_searches": 32, "reuse_subtree": True, "visit_targets": True, "playout_cap": {"fast": 6, "p_full": 0.4},
        "root_dirichlet_alpha": 0.3, "forced_playouts": 2.0}


def test_play_games_forces_and_prunes_the_full_plies_only():
    from sigma_zero_amd.sim import play_games
    starts, max_plies, salt = [0, 17, 518], [4, 5, 4], 4
    draws = np.random.default_rng(12).standard_gamma(0.3, size=(3, 8, N.SZ_MAX_MOVES)).astype(np.float32)
    u = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    full = lambda g, ply: (g + ply) % 2 == 0
    stats = {}
    got = play_games(HashModel(salt=salt), KEYS, 3, c960=True, scharnagl=starts, uniforms=u, full_search=full, root_gamma=lambda g, ply: draws[g, ply],
                     max_plies=max_plies, learning=True, stats=stats)
    want_forced = want_pruned = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for g, (n, plies) in enumerate(zip(starts, max_plies)):
            ref = FR.Game(sz.ChessTensor(chess960=True, scharnagl=n), 32, FR.worst_case(32), reuse=True, c=2.0, learning=True, mode="dyadic", salt=salt)
            fractions = []
            for ply in range(plies):
                ref.set_root_noise(True)
                ref.begin(32 if full(g, ply) else 6, draws[g, ply], False, 2.0 if full(g, ply) else 0.0)
                ref.run()
                rec = ref.play(u(g, ply))
                if full(g, ply):
                    vis = rec["visits"][:rec["n_child"]].astype(np.int64)
                    fractions.append((vis / int(vis.sum())).tolist())
            want_forced, want_pruned = want_forced + ref.forced_selections, want_pruned + ref.pruned_visits
            assert got[g]["chosen_actions"] == ref.chosen, "game %d: moves played" % g
            assert got[g]["sample_plies"] == [p for p in range(plies) if full(g, p)], "game %d: only full-search plies are recorded" % g
            assert [list(a.values()) for a in got[g]["actions"]] == fractions, "game %d: the targets are the pruned visit fractions" % g
    print("play_games:", {k: stats[k] for k in ("plies", "sims", "full_plies", "fast_plies", "forced_selections", "pruned_visits")})
    assert (stats["forced_selections"], stats["pruned_visits"]) == (want_forced, want_pruned) and want_forced > 0 and want_pruned > 0
    off = {}
    play_games(HashModel(salt=salt), {k: v for k, v in KEYS.items() if k != "forced_playouts"}, 1, c960=True, scharnagl=[0], uniforms=u, full_search=full,
               root_gamma=lambda g, ply: draws[g, ply], max_plies=2, learning=True, stats=off)
    assert off["forced_selections"] == 0 and off["pruned_visits"] == 0
    with pytest.raises(ValueError):
        play_games(HashModel(salt=salt), KEYS, 1, learning=False)
