"""The combined restatement tests/fullref.py (every self-play option in one board) on the CPU: with first-play urgency off it is endingref on
endingref's scenarios, with the ending rules off it is fpuref on fpuref's; under FPU every board of the role scenarios still does what its
role says and the conditions the combination is there for are reached; the play_games configuration of tests/test_gpu_full_config.py reaches
what it is there for, and sees a refilled slot that inherits the streaks or the kept subtree of the game before it; and the trainer's flags
yield that configuration (train_rl.selfplay_args_of)."""
import math
import warnings

import pytest

import endingref as ER
import fpuref as FP
import fullref as FU


def _trees_equal(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _same_games(tag, got, want):
    """two lists of restatement games: trees of every search (at begin and end), network input rows, moves, starts, goals, pruning, ending state"""
    n = 0
    for b, (g, w) in enumerate(zip(got, want)):
        t = "%s board %d" % (tag, b)
        assert g.chosen == w.chosen and g.starts == w.starts and g.goals == w.goals and g.error == w.error, t
        assert (g.forced_selections, g.pruned_visits) == (w.forced_selections, w.pruned_visits), t
        assert all(getattr(g, k) == getattr(w, k) for k in FU.Game.COUNTERS), t
        assert len(g.searches) == len(w.searches), t
        for a, s in zip(g.searches, w.searches):
            assert type(a) is type(s), t
            assert _trees_equal(a.tree(), s.tree()) and _trees_equal(a.begin_tree, s.begin_tree) and _trees_equal(a.tree_proven(), s.tree_proven()), t
            assert len(a.steps) == len(s.steps) and all((x == y).all() for x, y in zip(a.steps, s.steps)), t
        n += len(g.searches)
    return n


# ------------------------------------------------------------------------------------------------ degenerate cases
@pytest.mark.parametrize("L,solver", FU.OPTIONS)
def test_is_endingref_with_fpu_off(L, solver):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        n = 0
        for sc in ER.scenarios():
            got, want = FU.play(sc, L, solver, fpu=None), ER.play(sc, L, solver)
            n += _same_games("%s L=%d solver=%d" % (sc.name, L, solver), got, want)
            for g, w in zip(got, want):
                assert g.state == w.state and g.ended == w.ended and g.termination == w.termination and g.fpu_plies == [None] * len(g.searches)
                assert len(g.values) == len(w.values) and all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(g.values, w.values))
                assert not any(type(s) is FP.Search for s in g.searches)
        assert n >= 30


@pytest.mark.parametrize("L,solver", FU.OPTIONS)
def test_is_fpuref_with_the_endings_off(L, solver):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        n = 0
        for sc in FP.scenarios():
            want = FP.play(sc, L, solver, True)
            got = [FU.Game(bd.make(), sc.S, FP.worst_case(sc.S), reuse=True, L=L, lam=1.0, solver=solver, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt,
                           fpu=sc.fpu) for bd in sc.boards]
            gam = FP.gammas(sc) if sc.extras is not None else None
            for ply in range(sc.plies):
                for b, (g, bd) in enumerate(zip(got, sc.boards)):
                    if g.live:
                        g.set_endings(None)
                        FP.begin_ply(sc, g, b, ply, gam)
                        g.run()
                        g.play(bd.u(ply))
                        assert g.last[0] == FU.NONE and math.isnan(g.last[1]) and g.state == ER.FRESH
            n += _same_games("%s L=%d solver=%d" % (sc.name, L, solver), got, want)
            for g, w in zip(got, want):
                assert g.fpu_plies == w.fpu_plies and g.ended == [0, 0, 0, 0] and g.termination is None and g.cov == w.cov
        assert n >= 40


# ------------------------------------------------------------------------------------------------ role scenarios under FPU
_played = {}


def _play(name, L, solver):
    if (name, L, solver) not in _played:
        sc = next(s for s in FU.scenarios() if s.name == name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[(name, L, solver)] = (sc, FU.play(sc, L, solver))
    return _played[(name, L, solver)]


@pytest.mark.parametrize("L,solver", FU.RUNS)
def test_every_board_reaches_its_role_under_fpu(L, solver):
    games_all = []
    for sc in FU.scenarios():
        _, games = _play(sc.name, L, solver)
        for bd, g in zip(sc.boards, games):
            tag = "%s L=%d solver=%d %s: %r %r %r" % (sc.name, L, solver, bd.name, g.termination, g.ended, g.values)
            assert g.error is None and FU.role_reached(bd, g, solver), tag
            assert all(fp == FP.checked(FU.FPU) for fp in g.fpu_plies) and all(type(s) is FP.Search for s in g.searches), tag
            if g.termination is not None:                       # the game ended instead of a move: one record more than moves, nothing kept
                assert g.over and g.next is None and len(g.searches) == len(g.chosen) + 1, tag
        games_all += games
    cov = FU.coverage(games_all)
    print("coverage L=%d solver=%d:" % (L, solver), {k: cov[k] for k in FU.COVERAGE + FU.SOLVER_COVERAGE})
    FU.assert_coverage(cov, solver)
    assert (cov["ended_proven"] > 0) == solver and cov["forced_selections"] > 0 and cov["pruned_visits"] > 0


# ------------------------------------------------------------------------------------------------ the play_games configuration
_restated = {}


def _restate(L, solver, **kw):
    key = (L, solver) + tuple(sorted(kw.items()))
    if key not in _restated:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _restated[key] = FU.restate(FU.play_config(), L, solver, **kw)
    return _restated[key]


@pytest.mark.parametrize("L,solver", FU.OPTIONS)
def test_play_config_reaches_what_it_is_there_for(L, solver):
    cfg = FU.play_config()
    records, stats, games, refills = _restate(L, solver, n_slots=3)
    terms = [r["termination"] for r in records]
    print("L=%d solver=%d:" % (L, solver), terms, [r["would_end"] for r in records], stats, refills)
    assert len(cfg.starts) == 8 and all(3 <= c <= 6 for c in cfg.caps) and sum(cfg.held) == 2
    assert terms.count("resign") >= 1 and terms.count("draw_adjudicated") >= 1 and terms.count("max_plies") >= 1
    assert stats["holdout_marks"] >= 1 and any(r["would_end"] is not None and r["holdout"] for r in records)
    assert stats["full_plies"] > 0 and stats["fast_plies"] > 0
    quiet_fast = sum(s.quiet and s.target == cfg.fast and not getattr(s, "forced_k", 0.0) for g in games for s in g.searches)
    assert quiet_fast == stats["fast_plies"] >= 1                # quiet_fast_plies: every fast ply is quiet and not forced
    assert all(not s.quiet and s.target == cfg.S and s.forced_k == cfg.forced_k for g in games for s in g.searches if s.target != cfg.fast)
    assert any(st == "reused" for g in games for st in g.starts)
    assert stats["forced_selections"] > 0 and stats["pruned_visits"] > 0
    cov = FU.coverage(games)
    assert cov["clamp_low"] > 0 and cov["forced_overruled_fpu"] > 0 and cov["ended_on_continued_ply"] > 0, dict(cov)
    assert stats["sims"] == sum(sum(g.goals) for g in games) and any(goal < s.target for g in games for goal, s in zip(g.goals, g.searches))
    # the 3-slot schedule: a refill on a slot whose last game a rule ended, and one on a slot whose last game was a holdout game
    assert len(refills) == 5 and sorted(g for _, _, g in refills) == [3, 4, 5, 6, 7]
    assert any(games[before].termination is not None for _, before, _ in refills), refills
    assert any(cfg.held[before] for _, before, _ in refills), refills
    assert any(games[before].state != ER.FRESH and games[before].next is None for _, before, _ in refills)
    assert any(games[before].next is not None for _, before, _ in refills)
    # without a carried state a game's record does not depend on the slots
    alone = _restate(L, solver)
    assert alone[0] == records and alone[1] == stats and alone[3] == []


@pytest.mark.parametrize("L,solver", FU.OPTIONS)
@pytest.mark.parametrize("carry", ["endings", "subtree"])
def test_a_refill_that_keeps_the_last_games_state_changes_a_record(carry, L, solver):
    """teeth: the configuration sees a slot that starts its next game with the streaks, or with the kept subtree, of the game before it"""
    records = _restate(L, solver, n_slots=3)[0]
    faulty = _restate(L, solver, n_slots=3, carry=carry)[0]
    changed = [g for g, (a, b) in enumerate(zip(records, faulty)) if a != b]
    print("carry=%s L=%d solver=%d: games whose record changes: %s" % (carry, L, solver, changed), [faulty[g].get("broken") for g in changed])
    assert changed and all(g >= 3 for g in changed), changed      # the first three games start on empty slots


# ------------------------------------------------------------------------------------------------ the trainer's flags
FULL_FLAGS = ["--searches", "32", "--visit-targets", "--leaves-per-step", "4", "--solver", "--playout-cap-fast", "8", "--root-dirichlet-alpha", "0.3",
              "--quiet-fast-plies", "--forced-playouts", "2", "--resign-value", "-0.05", "--resign-patience", "2", "--resign-min-ply", "1",
              "--draw-value", "0.13", "--draw-patience", "2", "--draw-min-ply", "0", "--adjudicate-proven", "--ending-holdout", "0.25"]


def _args(flags):
    from sigma_zero_amd import train_rl
    return train_rl.selfplay_args_of(train_rl.flag_parser().parse_args(flags))


def _check(args):
    from sigma_zero_amd.selfplay import search_options_of, visit_target_options_of, forced_playout_options_of, ending_options_of
    from sigma_zero_amd.sim import playout_cap_of
    return search_options_of(args), visit_target_options_of(args), forced_playout_options_of(args), ending_options_of(args), playout_cap_of(args)


def test_the_trainers_full_flag_set_is_the_play_games_configuration():
    args = _args(FULL_FLAGS)
    search, vt, forced, end, pcap = _check(args)
    assert search == (4, 1.0, True, True) and vt == (True, True) and forced == 2.0 and pcap == (8, 0.25)
    assert end["proven"] is True and end["holdout"] == 0.25 and (end["resign_patience"], end["draw_patience"], end["resign_min_ply"]) == (2, 2, 1)
    want = FU.args_of(FU.play_config(), 4, True)
    assert want["fpu"] is not None and _check(want)[:4] == (search, vt, forced, end)
    assert set(args) - {"max_plies"} == set(want) - {"fpu"}, "main has no flag for args['fpu']; max_plies is run_cycle's"
    differs = {k for k in set(args) & set(want) if args[k] != want[k]}
    assert differs == {"playout_cap"} and args["playout_cap"]["fast"] == want["playout_cap"]["fast"], differs      # p_full: the tests decide per ply themselves
    assert set(args["endings"]) == set(want["endings"])
    # the second pair of the tests: no leaf batching, no solver
    plain = _args([f for f in FULL_FLAGS if f not in ("--leaves-per-step", "4", "--solver", "--adjudicate-proven")])
    want = FU.args_of(FU.play_config(), 1, False)
    assert set(plain) - {"max_plies"} == set(want) - {"fpu", "combine_options"}       # the trainer asks to combine only where there is something to
    assert _check(plain)[0] == (1, 1.0, False, False) and _check(want)[0] == (1, 1.0, False, True) and _check(plain)[1:4] == _check(want)[1:4]
    assert _check(plain)[3]["proven"] is False
    # no flag, no option
    assert _args([]) == {"C": 2, "num_searches": 100, "max_plies": 100000} and _check(_args([])) == ((1, 1.0, False, False), (False, False), None, None, None)


@pytest.mark.parametrize("flags", [
    ["--leaves-per-step", "4", "--solver"],                                      # each pair of leaf batching, solver, reuse needs combine_options,
    ["--quiet-fast-plies", "--playout-cap-fast", "8", "--root-dirichlet-alpha", "0.3"],      # which --visit-targets brings; quiet fast plies need it too
    ["--visit-targets", "--quiet-fast-plies", "--root-dirichlet-alpha", "0.3"],  # ... and a playout cap
    ["--adjudicate-proven"],                                                     # only the solver proves a root
    ["--resign-patience", "2"],                                                  # a patience needs its value
    ["--draw-patience", "2", "--draw-value", "-0.1"],
    ["--resign-patience", "2", "--resign-value", "-0.05", "--ending-holdout", "1.5"],
    ["--playout-cap-fast", "200"],                                               # above --searches
    ["--forced-playouts", "-1"],
])
def test_refused_flag_combinations_raise(flags):
    with pytest.raises(ValueError):
        _check(_args(flags))
