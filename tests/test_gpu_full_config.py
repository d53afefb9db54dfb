"""Every self-play option at once on the GPU (leaf batching, the solver, subtree reuse with visit targets and root noise, quiet fast plies,
forced playouts, first-play urgency and the ending rules: k_search_step<.., ForcedOpts, FpuOpts> and k_play<.., ForcedOpts, EndOpts> in one
engine), NON-REFERENCE options all of them.  a. the HIP engine against the combined restatement tests/fullref.py, bit for bit and ply after
ply, on endingref's role scenarios under FPU; b. sim.play_games with everything on and fewer board slots than games against per-game
restatements: a refilled slot starts clean in every option's per-slot state at once; c. the shipped networks under that configuration:
a game's records do not depend on the slot schedule.  tests/test_full_ref.py proves on the CPU that the scenarios reach the conditions they
are there for, and that the play_games configuration sees a refill that keeps the streaks or the kept subtree of the game before it."""
import math
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
from hashmodel import HashModel, evaluate_packed, pack_planes
import fullref as FU
from fullref import NONE

pytestmark = pytest.mark.gpu

ST_PENDING = 2


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


def _same_value(a, b):
    a, b = np.float64(a), np.float64(b)
    return bool(np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ a. the engine against the restatement
_played = {}


def _drive(sc, L, solver):
    B = len(sc.boards)
    args = {"combine_options": True, "C": 2, "num_searches": sc.S, "solver": solver, "leaves_per_step": L, "fpu": FU.fpu_args(FU.FPU)}
    if sc.reuse:
        args["reuse_subtree"] = True
    eng = SelfPlayEngine(None, args, B, chess960=sc.c960, learning=sc.learning, edges_per_board=sc.edges_per_board or 0)
    games = [FU.new_game(sc, bd, L, solver) for bd in sc.boards]
    modes = [(bd.mode, bd.salt) for bd in sc.boards]
    gam = FU.gammas(sc)
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
                    FU.begin_ply(sc, g, bd, b, ply, gam)
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
            assert eng.forced_stats()[0] == sum(g.forced_selections for g in games), "%s ply %d: forced selections" % (sc.name, ply)
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
                root = FU.position_record(g.game)
                want = g.play(u[b])
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r, restatement %r" % (tag(b), got, want)
                assert int(ends["kind"][b]) == g.last[0] and _same_value(ends["mover_value"][b], g.last[1]), \
                    "%s: sz_fetch_endings kind %d m %r, restatement %r" % (tag(b), ends["kind"][b], ends["mover_value"][b], g.last)
                pos = eng.debug_position(b)[0].tobytes()
                assert pos == FU.position_record(g.game), "%s: position record after sz_play" % tag(b)
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
    assert all(fp is not None for g in games for fp in g.fpu_plies)
    for bd, g in zip(sc.boards, games):
        assert FU.role_reached(bd, g, solver), "%s: board %s did not do what it is there for" % (sc.name, bd.name)
    _played[(sc.name, L, solver)] = games
    return games


@pytest.mark.parametrize("L,solver", FU.RUNS)
@pytest.mark.parametrize("name", [sc.name for sc in FU.scenarios()])
def test_whole_games_match_restatement(name, L, solver):
    sc = next(s for s in FU.scenarios() if s.name == name)
    games = _drive(sc, L, solver)
    if sc.reuse:                                                # the reuse engine: every ply after the first continues on a kept subtree
        assert all(s == "reused" for g in games for s in g.starts[1:])
    else:                                                       # the budgets engine
        assert all(s == "new" for g in games for s in g.starts)


@pytest.mark.parametrize("L,solver", FU.RUNS)
def test_whole_games_coverage(L, solver):
    """the conditions the combination is there for, counted on the games the device was compared with (driven here when this test runs alone)"""
    games = []
    for sc in FU.scenarios():
        games += _played.get((sc.name, L, solver)) or _drive(sc, L, solver)
    cov = FU.coverage(games)
    print("coverage L=%d solver=%d:" % (L, solver), {k: cov[k] for k in FU.COVERAGE + FU.SOLVER_COVERAGE})
    FU.assert_coverage(cov, solver)
    assert cov["forced_selections"] > 0 and cov["pruned_visits"] > 0


# ------------------------------------------------------------------------------------------------ b. play_games, everything on
_restated = {}


def _restate(L, solver):
    if (L, solver) not in _restated:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _restated[(L, solver)] = FU.restate(FU.play_config(), L, solver, n_slots=3)
    return _restated[(L, solver)]


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("n_boards", [8, 3])
@pytest.mark.parametrize("L,solver", FU.OPTIONS)
def test_play_games_with_everything_on_matches_per_game_restatements(L, solver, n_boards, compact):
    from sigma_zero_amd.sim import play_games, ending_report
    cfg = FU.play_config()
    want, want_stats, ref_games, refills = _restate(L, solver)
    stats = {}
    got = play_games(HashModel(mode=cfg.mode, salt=cfg.salt), FU.args_of(cfg, L, solver), len(cfg.starts), c960=True, scharnagl=cfg.starts, uniforms=cfg.uniforms,
                     full_search=cfg.full_search, root_gamma=cfg.root_gamma, holdout=cfg.holdout, max_plies=cfg.caps, learning=True, n_boards=n_boards,
                     compact=compact, stats=stats)
    assert len(got) == len(want) == 8
    for g, (a, w) in enumerate(zip(got, want)):
        a = FU.record_of(a)
        for k in FU.RECORD_KEYS:
            assert a[k] == w[k], "game %d (start %d) L=%d solver=%d n_boards=%d compact=%d: %s %r, restatement %r" % (
                g, cfg.starts[g], L, solver, n_boards, compact, k, a[k] if k != "packed_states" else "...", w[k] if k != "packed_states" else "...")
        assert len(got[g]["states"]) == len(w["sample_plies"])
    print("play_games L=%d solver=%d n_boards=%d compact=%d:" % (L, solver, n_boards, compact), [g["termination"] for g in got], {k: stats[k] for k in FU.STAT_KEYS})
    assert {k: stats[k] for k in FU.STAT_KEYS} == want_stats
    # what the device's own games reached (tests/test_full_ref.py asserts the same of the restatement): no vacuous pass
    terms = [g["termination"] for g in got]
    assert terms.count("resign") >= 1 and terms.count("draw_adjudicated") >= 1 and terms.count("max_plies") >= 1 and stats["holdout_marks"] >= 1
    assert stats["forced_selections"] > 0 and stats["pruned_visits"] > 0 and stats["full_plies"] > 0 and stats["fast_plies"] > 0
    assert stats["sims"] < stats["full_plies"] * cfg.S + stats["fast_plies"] * cfg.fast, "kept roots counted towards the targets"
    if n_boards == 3:                                           # the refills of the restatement's schedule happened here
        assert any(got[before]["termination"] in ("resign", "draw_adjudicated", "proven") for _, before, _ in refills)
        assert any(got[before]["holdout"] for _, before, _ in refills)
    r = ending_report(got)
    assert r["games"] == 8 and r["holdout_games"] == stats["holdout_games"] == 2 and r["holdout_marks"] == stats["holdout_marks"]
    assert (r["resigned"], r["adjudicated_draws"], r["adjudicated_proven"]) == (stats["resigned"], stats["adjudicated_draws"], stats["adjudicated_proven"])
    assert r["resigned"] + r["adjudicated_draws"] + r["adjudicated_proven"] + r["rules"] + r["max_plies"] == 8
    assert r["resign_marks"] + r["draw_marks"] == r["holdout_marks"]


# ------------------------------------------------------------------------------------------------ c. the shipped networks
@pytest.mark.parametrize("kind", ["fp16", "split"])
def test_shipped_networks_records_do_not_depend_on_the_slot_schedule(kind):
    """the real-f32 counterpart of test_refill_and_compaction_give_identical_per_game_records under the full configuration: in-search batch
    shrinking from per-board goals, leaf gathers that end early, pruning and the ending rules add paths on which a slot schedule could reach a
    record.  draw_value 1.0 qualifies every search: every game that is not a holdout game is adjudicated at its third search, whatever the
    network says, so 12 games on 5 slots are certain to be refilled 7 times"""
    from sigma_zero_amd.fastnet import FastPolicyNet, SplitPolicyNet
    from sigma_zero_amd.sim import play_games
    torch.manual_seed(0)
    net = sz.policyNN({}).cuda().eval()
    fast = FastPolicyNet(net, operands="fp16") if kind == "fp16" else SplitPolicyNet(net)
    cfg = FU.play_config()
    n_games, held = 12, [g in (3, 7) for g in range(12)]
    args = FU.args_of(cfg, 4, True, endings={"draw_value": 1.0, "draw_patience": 3})
    args["num_searches"] = 24
    starts = [(3 * g + 5) % 960 for g in range(n_games)]
    caps = [5 if held[g] else 6 for g in range(n_games)]
    draws = np.random.default_rng(13).standard_gamma(0.3, size=(n_games, 6, N.SZ_MAX_MOVES)).astype(np.float32)

    def run(n_boards, compact):
        st, events = {}, []                                     # play_games asks holdout(g) when game g starts and uniforms(g, ply) when it moves

        def uniforms(g, ply):
            events.append("move")
            return cfg.uniforms(g, ply)

        def holdout(g):
            events.append("start")
            return held[g]

        games = play_games(fast, args, n_games, c960=True, scharnagl=starts, uniforms=uniforms, full_search=cfg.full_search,
                           root_gamma=lambda g, ply: draws[g, ply], holdout=holdout, max_plies=caps, learning=True, planes_dtype="bits128",
                           n_boards=n_boards, compact=compact, stats=st)
        st["refills"] = events[events.index("move"):].count("start")       # games started on a slot another game had played on
        return [FU.record_of(g) for g in games], st

    runs = [run(n_boards, compact) for n_boards in (12, 5) for compact in (True, False)]
    base, st0 = runs[0]
    for records, st in runs[1:]:
        for g, (a, b) in enumerate(zip(base, records)):
            for k in FU.RECORD_KEYS:
                assert a[k] == b[k], "%s game %d: %s differs between slot schedules" % (kind, g, k)
        assert {k: st[k] for k in FU.STAT_KEYS} == {k: st0[k] for k in FU.STAT_KEYS}
    print(kind, [r["termination"] for r in base], {k: st0[k] for k in FU.STAT_KEYS}, [st["searches_without_network"] for _, st in runs])
    for g, r in enumerate(base):
        if held[g]:                                             # played out to its cap, marked where the rule would have ended it
            assert r["termination"] == "max_plies" and len(r["chosen_actions"]) == 5 and r["would_end"] == {"kind": "draw_adjudicated", "ply": 2, "colour": 1}
        else:                                                   # two moves, then the third search ends the game
            assert r["termination"] == "draw_adjudicated" and len(r["chosen_actions"]) == 2 and r["would_end"] is None and r["result"] == "1/2-1/2"
    assert [st["refills"] for _, st in runs] == [0, 0, 7, 7], "12 games on 5 slots: 7 refills"
    assert all(st["plies"] > runs[0][1]["plies"] == 5 for _, st in runs[2:])       # ... which took lock-step plies the 12-slot runs did not need
    assert st0["adjudicated_draws"] == 10 and st0["holdout_marks"] == 2 and st0["holdout_games"] == 2
    kept_counted = st0["sims"] < st0["full_plies"] * 24 + st0["fast_plies"] * cfg.fast
    assert kept_counted or any(st["searches_without_network"] > 0 for _, st in runs), "a kept root counted towards its target"
    assert st0["pruned_visits"] > 0 and st0["forced_selections"] > 0
