"""The restatement tests/endingref.py (resignation and adjudicated game endings) on the CPU: the rule on cases worked by hand; with the
option off it is forcedref on forcedref's own scenarios; the scenarios and hook cases tests/test_gpu_endings.py runs on the device reach
every condition they are there for, every board does what its role says; and the validation of args["endings"]."""
import collections
import math
import warnings

import numpy as np
import pytest

import endingref as ER
import forcedref as FR
from endingref import DRAW_ADJ, FRESH, NONE, PROVEN, RESIGN, State, decide, options
from solverref import DRAW, LOSS, WIN


# ------------------------------------------------------------------------------------------------ the rule by hand
def test_threshold_hit_exactly_fires():
    o = options(resign_value=-0.25, resign_patience=1, draw_value=0.125, draw_patience=1)
    # c* = child 1 (N = 8): m = -(2 / 8) = -0.25, exactly the resign threshold
    kind, m, st, marked = decide([3, 8, 8], [9.0, 2.0, -8.0], 0, 1, 0, FRESH, o, False)
    assert (kind, m, st, marked) == (RESIGN, -0.25, State(0, 1, 0, -1, 0, 0), False)
    # one ulp above it does not: W = 2 - 2^-51 -> m = -0.25 + 2^-54
    assert decide([3, 8, 8], [9.0, math.nextafter(2.0, 0.0), -8.0], 0, 1, 0, FRESH, o, False)[0] == NONE
    # |m| = 0.125 exactly, from either side, fires the draw rule (resign does not: 0.125 and -0.125 > -0.25)
    for w in (1.0, -1.0):
        kind, m, st, _ = decide([8], [w], 0, 0, 0, FRESH, o, False)
        assert (kind, m, st) == (DRAW_ADJ, -w / 8.0, State(0, 0, 1, -1, 0, 0))
    assert decide([8], [math.nextafter(1.0, 2.0)], 0, 0, 0, FRESH, o, False)[0] == NONE
    # the threshold is the f32 the struct holds: 0.1f > 0.1, so m = 0.1 (f64) fires and m = f64(0.1f) fires, the next f64 above it does not
    o = options(resign_value=0.1, resign_patience=1)
    t = float(np.float32(0.1))
    assert t > 0.1 and decide([1], [-t], 0, 1, 0, FRESH, o, False)[0] == RESIGN
    assert decide([1], [-math.nextafter(t, 1.0)], 0, 1, 0, FRESH, o, False)[0] == NONE


def test_one_good_search_resets_a_streak_and_the_colours_count_apart():
    o = options(resign_value=-0.5, resign_patience=3)
    bad, good = ([4], [3.0]), ([4], [0.0])                      # m = -0.75, m = -0.0
    st = FRESH
    for ply, (colour, pos, want) in enumerate([(1, bad, (0, 1)), (0, bad, (1, 1)), (1, bad, (1, 2)), (0, good, (0, 2)), (1, good, (0, 0)),
                                              (0, bad, (1, 0)), (1, bad, (1, 1)), (0, bad, (2, 1)), (1, bad, (2, 2))]):
        kind, _, st, _ = decide(*pos, 0, colour, ply, st, o, False)
        assert kind == NONE and (st.rs0, st.rs1) == want, ply
    assert decide(*bad, 0, 0, 9, st, o, False)[0] == RESIGN     # black's third in a row; white's streak of 2 is untouched
    assert decide(*bad, 0, 0, 9, st, o, False)[2][:2] == (3, 2)
    # the draw streak is shared by both colours and reset by one decisive-looking search
    o = options(draw_value=0.25, draw_patience=3)
    level = ([4], [0.5])
    st = decide(*level, 0, 1, 0, FRESH, o, False)[2]
    st = decide(*level, 0, 0, 1, st, o, False)[2]
    assert st.ds == 2 and decide(*level, 0, 1, 2, st, o, False)[0] == DRAW_ADJ
    st = decide(*bad, 0, 1, 2, st, o, False)[2]
    assert st.ds == 0


def test_min_ply_holds_a_full_streak_back_until_reached():
    o = options(resign_value=0.0, resign_patience=2, resign_min_ply=6)
    st, kinds = FRESH, []
    for ply in range(0, 8, 2):                                  # white's searches at plies 0, 2, 4, 6: the streak is full from ply 2 on
        kind, _, st, _ = decide([2], [1.0], 0, 1, ply, st, o, False)
        kinds.append(kind)
    assert kinds == [NONE, NONE, NONE, RESIGN] and st.rs1 == 4


def test_resign_beats_draw_and_nan_resets_both_streaks():
    o = options(resign_value=0.0, resign_patience=1, draw_value=0.0, draw_patience=1)
    assert decide([4], [0.0], 0, 1, 0, FRESH, o, False)[0] == RESIGN             # m = -0.0: both fire
    assert decide([4], [0.0], 0, 1, 0, FRESH, dict(o, resign_patience=0), False)[0] == DRAW_ADJ
    st = State(5, 5, 5, -1, 0, 0)
    kind, m, st2, _ = decide([4], [math.nan], 0, 1, 0, st, options(resign_value=1.0, resign_patience=1, draw_value=1.0, draw_patience=1), False)
    assert kind == NONE and math.isnan(m) and st2 == State(5, 0, 0, -1, 0, 0)
    # streaks saturate rather than wrap
    st = State(65535, 65535, 65535, -1, 0, 0)
    assert decide([4], [4.0], 0, 0, 0, st, options(resign_value=0.0, resign_patience=0, draw_value=1.0), False)[2] == st


def test_a_holdout_board_records_the_first_mark_only():
    o = options(resign_value=-0.5, resign_patience=1, draw_value=0.125, draw_patience=1)
    kind, _, st, marked = decide([4], [0.25], 0, 0, 7, FRESH, o, True)          # the draw rule fires at ply 7
    assert (kind, marked, st) == (NONE, True, State(0, 0, 1, 7, DRAW_ADJ, 0))
    kind, _, st, marked = decide([4], [3.0], 0, 1, 8, st, o, True)              # the resign rule fires at ply 8: nothing further is recorded
    assert (kind, marked, st) == (NONE, False, State(0, 1, 0, 7, DRAW_ADJ, 0))
    assert decide([4], [3.0], 0, 1, 8, st, o, False)[0] == RESIGN                # the same board without the flag


def test_proven_precedes_the_streaks_and_ignores_holdout():
    o = options(resign_value=1.0, resign_patience=1, draw_value=1.0, draw_patience=1, proven=1)
    st = State(2, 3, 4, -1, 0, 0)
    for code in (WIN, DRAW, LOSS):
        for hold in (False, True):
            kind, m, st2, marked = decide([4], [2.0], code, 1, 0, st, o, hold)
            assert (kind, m, st2, marked) == (PROVEN, -0.5, st, False)
    assert [ER.result_of(PROVEN, c, 1) for c in (WIN, DRAW, LOSS)] == [1, 0, -1] and [ER.result_of(PROVEN, c, 0) for c in (WIN, DRAW, LOSS)] == [-1, 0, 1]
    assert ER.result_of(RESIGN, 0, 1) == -1 and ER.result_of(RESIGN, 0, 0) == 1 and ER.result_of(DRAW_ADJ, 0, 1) == 0
    assert decide([4], [2.0], 0, 1, 0, st, o, False)[0] == RESIGN                # an unknown root: the streaks decide
    assert decide([4], [2.0], WIN, 1, 0, st, dict(o, proven=0), False)[0] == RESIGN


def test_cstar_uses_the_counted_not_the_pruned_visits():
    # forcedref's hand case: counted N = [12, 2, 6, 12, 1, 3], pruned [12, 0, 5, 6, 1, 0].  c* is the first maximum of the counted visits,
    # child 0, although child 3 has as many; m is child 0's
    N, W, P = [12, 2, 6, 12, 1, 3], [6.0, 2.0, -1.68, -12.0, -1.0, 3.0], [0.4, 0.01, 0.1, 0.2, 0.29, 0.04]
    assert ER.mover_value(N, W) == (0, -0.5)
    assert FR.prune(N, [0.0, 2.0, -1.68, 0.0, -1.0, 3.0], P, 37, 2.0, 8.0)[0].tolist() == [12, 0, 5, 6, 1, 0]
    # a count vector only pruning can produce would move c*: the rule never sees it
    assert ER.mover_value([5, 0, 5, 6, 1, 0], W)[0] == 3
    # ... and in a whole game: on the forced boards the record holds fewer visits than the m was computed from
    sc, games = _play("c960_endings", 1, False)
    g = games[0]
    assert g.termination == RESIGN and g.search.pruned is not None and g.search.pruned.sum() < g.search.root_children()[1].sum()
    acts, vis = g.search.root_children()
    f = int(g.search.first[0])
    assert g.last[1] == ER.mover_value(vis, g.search.W[f:f + len(acts)])[1]


# ------------------------------------------------------------------------------------------------ option off
def test_is_forcedref_with_the_option_off():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sc = FR.scenarios()[0]
        sc = sc._replace(plies=3)
        for L, solver in FR.OPTIONS:
            want, gam = FR.play(sc, L, solver), FR.gammas(sc)
            for b, (bd, w) in enumerate(zip(sc.boards, want)):
                g = ER.Game(bd.make(), sc.S, sc.edges_per_board, reuse=sc.reuse, L=L, lam=1.0, solver=solver, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt)
                for ply in range(sc.plies):
                    FR.begin_ply(sc, g, bd, b, ply, gam)
                    g.run()
                    g.play(bd.u(ply))
                    assert g.last[0] == NONE and math.isnan(g.last[1]) and g.state == FRESH
                assert g.chosen == w.chosen and g.starts == w.starts and g.goals == w.goals and g.pruned_visits == w.pruned_visits
                assert all(x.tobytes() == y.tobytes() for a, s in zip(g.searches, w.searches) for x, y in zip(a.tree(), s.tree()))


# ------------------------------------------------------------------------------------------------ scenarios and hook cases
_played = {}


def _play(name, L, solver):
    if (name, L, solver) not in _played:
        sc = next(s for s in ER.scenarios() if s.name == name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[(name, L, solver)] = (sc, ER.play(sc, L, solver))
    return _played[(name, L, solver)]


@pytest.mark.parametrize("L,solver", ER.OPTIONS)
def test_every_board_does_what_its_role_says(L, solver):
    for sc in ER.scenarios():
        _, games = _play(sc.name, L, solver)
        for bd, g in zip(sc.boards, games):
            assert g.error is None and ER.role_reached(bd, g, solver), "%s L=%d solver=%d %s: %r %r %r" % (sc.name, L, solver, bd.name, g.termination, g.ended, g.values)
            if g.termination is not None:                       # the game ended instead of a move: one record more than moves, nothing kept
                assert g.over and g.next is None and len(g.searches) == len(g.chosen) + 1
    sc, games = _play("c960_endings", L, solver)                # all four roles beside each other, on a reuse engine
    assert sc.reuse and all(sc.noise) and [b.role for b in sc.boards] == ["resigns", "draw", "holdout_mark", "plays_on"]
    assert games[2].state.would_kind == DRAW_ADJ and len(games[2].chosen) == sc.plies
    sc, games = _play("budgets_endings", L, solver)
    assert not sc.reuse and games[1].state[3:] == (3, RESIGN, 0)


def test_scenarios_and_hook_cases_reach_every_condition():
    hc = ER.hook_cases()
    widths = set(np.diff(hc.offsets).tolist())
    assert len(hc.R) >= 2000 and set(ER.HOOK_K) <= widths and max(widths) == ER.MAX_MOVES
    kind, m, state, hook = ER.hook_reference(hc)
    print("hook coverage:", dict(hook))
    assert all(hook[k] >= 1 for k in ER.HOOK_COVERAGE), dict(hook)
    played = [_play(sc.name, L, solver) for sc in ER.scenarios() for L, solver in ER.OPTIONS]
    cov = ER.coverage(played, hook)
    print("coverage:", dict(cov))
    assert all(cov[k] >= 1 for k in ER.COVERAGE), [k for k in ER.COVERAGE if cov[k] < 1]
    alone = ER.coverage(played)                                # whole games reach everything but the arithmetic corner cases of the hook
    rest = [k for k in ER.COVERAGE if alone[k] < 1]
    assert set(rest) <= {"resign_beat_draw", "nan_value", "exact_threshold", "wide_case", "cstar_tie"}, rest
    for L, solver in ER.OPTIONS:                               # with and without leaf batching / the solver, each on its own
        c = ER.coverage([v for (_, l, sv), v in _played.items() if (l, sv) == (L, solver)])
        assert c["resignations"] > 0 and c["adjudicated_draws"] > 0 and c["holdout_marks"] > 0 and c["ended_on_continued_ply"] > 0 and c["ended_forced_pruned"] > 0
        assert (c["proven_endings"] > 0) == solver and (c["win_root_played_option_on"] > 0) == solver


# ------------------------------------------------------------------------------------------------ validation of args["endings"]
def test_ending_options_of_validates():
    from sigma_zero_amd.selfplay import ending_options_of, ENDING_KEYS
    assert ending_options_of({}) is None
    full = ending_options_of({"solver": True, "endings": {"resign_value": -0.9, "resign_patience": 3, "resign_min_ply": 20, "draw_value": 0.05,
                                                          "draw_patience": 8, "draw_min_ply": 60, "proven": True, "holdout": 0.1}})
    assert set(full) == set(ENDING_KEYS) and full["resign_value"] == float(np.float32(-0.9)) and full["proven"] is True and full["holdout"] == 0.1
    off = ending_options_of({"endings": {}})                   # on, with every rule off
    assert off == dict(resign_value=0.0, resign_patience=0, resign_min_ply=0, draw_value=0.0, draw_patience=0, draw_min_ply=0, proven=False, holdout=0.0)
    assert ending_options_of({"endings": {"draw_value": np.float32(0.5), "draw_patience": np.int64(2)}})["draw_patience"] == 2
    bad = [{"resign_value": -1.5, "resign_patience": 1}, {"resign_value": 1.5}, {"resign_value": float("nan")}, {"resign_value": float("inf")},
           {"resign_value": "0"}, {"resign_value": True}, {"draw_value": -0.1}, {"draw_value": 1.5}, {"draw_value": float("nan")},
           {"resign_patience": 1}, {"draw_patience": 2}, {"resign_value": 0.0, "resign_patience": -1}, {"resign_value": 0.0, "resign_patience": 65536},
           {"resign_value": 0.0, "resign_patience": 1.5}, {"resign_value": 0.0, "resign_patience": True}, {"draw_value": 0.0, "draw_patience": 70000},
           {"resign_min_ply": -1}, {"draw_min_ply": -1}, {"draw_min_ply": 2.0}, {"holdout": -0.1}, {"holdout": 1.5}, {"holdout": float("nan")},
           {"holdout": True}, {"proven": 1}, {"proven": True}, {"resign": 1}, "on", 3]
    for b in bad:
        with pytest.raises(ValueError):
            ending_options_of({"endings": b})
    assert ending_options_of({"solver": True, "endings": {"proven": True}})["proven"] is True
    assert ending_options_of({"endings": {"resign_value": -1.0, "resign_patience": 65535, "draw_value": 1.0, "holdout": 1}})["holdout"] == 1.0


def test_ending_report_adds_up():
    from sigma_zero_amd.sim import ending_report
    g = lambda term, result, hold=False, would=None: dict(termination=term, result=result, holdout=hold, would_end=would)
    games = [g("resign", "0-1"), g("draw_adjudicated", "1/2-1/2"), g("proven", "1-0"), g("rules", "1-0"), g("max_plies", None),
             g("rules", "0-1", True, {"kind": "resign", "ply": 30, "colour": 1}),              # white would have resigned and lost: right
             g("rules", "1/2-1/2", True, {"kind": "resign", "ply": 30, "colour": 1}),          # ... and drew: a false positive
             g("rules", "0-1", True, {"kind": "resign", "ply": 31, "colour": 0}),              # black would have resigned and won: a false positive
             g("rules", "1/2-1/2", True, {"kind": "draw_adjudicated", "ply": 80, "colour": 0}),
             g("rules", "1-0", True, {"kind": "draw_adjudicated", "ply": 80, "colour": 1}),    # decisive after all: a false positive
             g("max_plies", None, True, None)]
    r = ending_report(games)
    assert r == dict(games=11, resigned=1, adjudicated_draws=1, adjudicated_proven=1, rules=6, max_plies=2, holdout_games=6, holdout_marks=5,
                     resign_marks=3, resign_false_positives=2, draw_marks=2, draw_false_positives=1)
