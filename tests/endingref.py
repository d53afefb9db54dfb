"""Plain-Python restatement of resignation and adjudicated game endings (sz_set_endings / sz_fetch_endings / sz_ending_stats / sz_debug_endings,
args["endings"], a NON-REFERENCE option; include/sigmazero.h is the specification).  It is what wave_ending and the ending branch of
k_play<.., EndOpts> in csrc/sz_engine.hip are held to, bit for bit (tests/test_gpu_endings.py).  Built on forcedref (Game), which already
composes visit targets, root noise, forced playouts, the solver and leaf batching, and stays as it is:

  * decide() is the rule on plain arrays, pure: children's counted N and W, the root's proven code, colour, ply, the board's state, the
    options and the holdout flag -> (kind, m, new state, marked);
  * Game.set_endings(opts, holdout) is sz_set_endings for this board (opts None: off); Game.play(u) applies the rule on the counted visits
    after the zero-visit check: where no ending fires it is forcedref's play, where one fires the game ends instead of a move (no push, no
    kept subtree, the record with chosen = -1); Game.last = (kind, m) is what sz_fetch_endings says about that sz_play;
  * Game.reset_endings() is what sz_new_games / sz_upload_game do to the board's state;
  * ended[4] counts resignations, adjudicated draws, proven endings and holdout marks like the engine's counters (sz_ending_stats).

With opts None everywhere it is forcedref (tests/test_ending_ref.py pins it).  scenarios() and hook_cases() are the inputs both test
modules use; cov counts, on the restatement alone, the conditions the GPU cases must reach (COVERAGE)."""
import collections
import math

import numpy as np

import forcedref as FR
from composeref import DRAW, LOSS, WIN
from forcedref import FULL, MAX_MOVES, WIDE_FEN, OPTIONS, gammas, position_record, worst_case      # noqa: F401 (re-exported)
from hashmodel import pack_planes

F64 = np.float64
NONE, RESIGN, DRAW_ADJ, PROVEN = 0, 1, 2, 3              # SZ_END_*
STREAK_MAX = 65535
KEYS = ("resign_value", "resign_patience", "resign_min_ply", "draw_value", "draw_patience", "draw_min_ply", "proven")

State = collections.namedtuple("State", "rs0 rs1 ds would_ply would_kind would_colour")
FRESH = State(0, 0, 0, -1, 0, 0)


def options(**kw):
    """an sz_ending_options as a dict: absent keys are that rule off; the two values as the f32 the struct holds"""
    assert set(kw) <= set(KEYS), kw
    o = dict(resign_value=0.0, resign_patience=0, resign_min_ply=0, draw_value=0.0, draw_patience=0, draw_min_ply=0, proven=0)
    o.update(kw)
    o["resign_value"], o["draw_value"] = float(np.float32(o["resign_value"])), float(np.float32(o["draw_value"]))
    return o


def mover_value(N, W):
    """(c*, m): the first maximum of the counted visits, and m = -(W_c* / (double)N_c*) in f64"""
    N = np.asarray(N, np.int64)
    cs = int(np.argmax(N))
    with np.errstate(all="ignore"):
        return cs, -(F64(np.asarray(W, F64)[cs]) / F64(N[cs]))


def result_of(kind, code, colour):
    """+1 white wins, -1 black wins, 0 draw"""
    mover = 1 if colour else -1
    if kind == RESIGN:
        return -mover
    if kind == PROVEN:
        return mover if code == WIN else (-mover if code == LOSS else 0)
    return 0


def decide(N, W, R_root, colour, ply, state, opts, holdout):
    """The rule of sz_set_endings on a finished search.  N, W: the root children's counted visits and value sums in action order; R_root: the
    root's proven code (0 / None: unknown, or no solver); state: State -> (kind that ends the game or 0, m, new State, a mark was recorded)"""
    _, m = mover_value(N, W)
    if opts["proven"] and R_root:
        return PROVEN, m, state, False
    col = 1 if colour else 0
    rs = [state.rs0, state.rs1]
    rs[col] = min(rs[col] + 1, STREAK_MAX) if m <= F64(np.float32(opts["resign_value"])) else 0
    ds = min(state.ds + 1, STREAK_MAX) if abs(m) <= F64(np.float32(opts["draw_value"])) else 0
    fire_resign = opts["resign_patience"] > 0 and rs[col] >= opts["resign_patience"] and ply >= opts["resign_min_ply"]
    fire_draw = opts["draw_patience"] > 0 and ds >= opts["draw_patience"] and ply >= opts["draw_min_ply"]
    kind = RESIGN if fire_resign else (DRAW_ADJ if fire_draw else NONE)
    would, marked = (state.would_ply, state.would_kind, state.would_colour), False
    if kind and holdout:
        if state.would_ply < 0:
            would, marked = (int(ply), kind, col), True
        kind = NONE
    return kind, m, State(rs[0], rs[1], ds, *would), marked


class Game(FR.Game):
    """forcedref.Game with the ending rules in play()"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.end_opts, self.holdout, self.state = None, False, FRESH
        self.last = (NONE, math.nan)                      # sz_fetch_endings' kind and mover_value of this board's last sz_play
        self.ended = [0, 0, 0, 0]                         # sz_ending_stats
        self.termination = None                           # the kind that ended the game
        self.values = []                                  # per ply m (option on)

    def set_endings(self, opts, holdout=False):
        """sz_set_endings: never touches the kept subtree, the streaks or the mark"""
        self.end_opts, self.holdout = (None if opts is None else dict(opts)), bool(holdout)

    def reset_endings(self):
        """sz_new_games / sz_upload_game on this board"""
        self.state = FRESH

    def root_ply(self):
        return int(self.game.export_ring()[1])

    def play(self, u):
        s = self.search
        if self.end_opts is None:                         # off: nothing is updated
            self.last = (NONE, math.nan)
            return super().play(u)
        acts, vis = s.root_children()
        k = len(acts)
        assert k > 0 and vis.sum() > 0, "SZ_ERR_ZERO_VISITS"     # first, on the counted visits
        f = int(s.first[0])
        colour, ply = int(bool(self.game.board.turn)), self.root_ply()
        code = int(s.R[0]) if s.solver else 0
        before = self.state
        kind, m, self.state, marked = decide(vis, s.W[f:f + k], code, colour, ply, before, dict(self.end_opts, proven=self.end_opts["proven"] and s.solver), self.holdout)
        self.last = (kind, float(m))
        self.values.append(float(m))
        self.ended[3] += marked
        c = self.cov
        c["holdout_mark"] += marked
        c["holdout_fired_again"] += bool(self.holdout and not marked and before.would_ply >= 0 and self._fires(before, m, colour, ply))
        c["nan_value"] += bool(np.isnan(m))
        c["streak_reset"] += (before.rs1 if colour else before.rs0) > 0 and (self.state.rs1 if colour else self.state.rs0) == 0 and kind != PROVEN
        c["cstar_not_first"] += int(np.argmax(vis)) > 0
        forced = bool(getattr(s, "forced_k", 0.0))
        if kind == NONE and not marked and not self.holdout:          # a full streak that min_ply alone holds back
            c["min_ply_held"] += decide(vis, s.W[f:f + k], 0, colour, ply, before, dict(self.end_opts, proven=0, resign_min_ply=0, draw_min_ply=0), False)[0] != NONE
        if kind == NONE:
            c["played_on_with_option_on"] += 1
            c["goal_0_ply_counted"] += bool(self.goals and self.goals[-1] == 0)
            if s.solver and code == WIN:
                c["win_root_played_option_on"] += 1
            return super().play(u)
        # ---- the game ends instead of a move
        self.ended[kind - 1] += 1
        self.termination = kind
        c["ended_%s" % ("", "resign", "draw", "proven")[kind]] += 1
        c["ended_on_continued_ply"] += self.starts[-1] == "reused"
        c["ended_on_goal_0_ply"] += bool(self.goals and self.goals[-1] == 0)
        c["ended_forced_pruned"] += forced
        if kind == PROVEN:
            c["proven_%s" % {WIN: "win", DRAW: "draw", LOSS: "loss"}[code]] += 1
            c["proven_on_holdout"] += self.holdout
        if kind == RESIGN:
            c["resign_beat_draw"] += bool(self.end_opts["draw_patience"] > 0 and self.state.ds >= self.end_opts["draw_patience"] and ply >= self.end_opts["draw_min_ply"])
            c["resign_by_%s" % ("white" if colour else "black")] += 1
        rec_vis = vis
        if forced:                                        # the record is pruned as always; the counter grows
            s.pruned, _, info = FR.prune(vis, s.W[f:f + k], s.P[f:f + k], int(s.N[0]), s.c, s.forced_k)
            self.pruned_visits += int((vis - s.pruned).sum())
            c.update(info)
            rec_vis = s.pruned
        rec = dict(packed=pack_planes(self.game.get_representation().numpy()), action=np.full(MAX_MOVES, -1, np.int32),
                   visits=np.zeros(MAX_MOVES, np.int32), n_child=k, colour=colour, chosen=-1)
        rec["action"][:k], rec["visits"][:k] = acts, rec_vis
        self.over, self.result = True, result_of(kind, code, colour)
        rec["game_over"], rec["result"] = 1, self.result
        return rec                                        # no move, no kept subtree: self.next stays None

    def _fires(self, before, m, colour, ply):
        return decide([1], [-m], 0, colour, ply, before, self.end_opts, False)[0] != NONE


# ---------------------------------------------------------------------------------------------------------------- scenarios
Scenario = collections.namedtuple("Scenario", "name S c960 learning edges_per_board plies boards noise k reuse endings")
# endings: per ply the options of sz_set_endings (a dict of options(), None = off); the rest as forcedref.Scenario
Board = collections.namedtuple("Board", "name make mode salt u targets quiet forced holdout role")
# holdout: the board's flag; role: what the board is there for, one of ROLES (asserted by coverage()); the rest as forcedref.Board
ROLES = ("resigns", "draw", "holdout_mark", "plays_on", "proven_win", "proven_loss", "proven_draw", "plays_win_move", "late_win")

FORCED_DRAW_FEN = "7k/8/8/8/8/8/1q6/K7 w - - 0 1"         # solver_cases.FENS["forced_draw"]
MATED_IN_2_FEN = "k7/8/1K6/8/8/p7/8/7R b - - 0 1"         # solver_cases.FENS["mated_in_2"]


def _u(b):
    return lambda ply: ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0


# The thresholds were chosen on the CPU from the m this restatement sees on these boards; tests/test_ending_ref.py asserts that every board
# does what its role says, under both option combinations.  The options are one set per engine, so the board "with every rule off beside
# them" is a board no rule ever fires on (and that is not forced): its m stays above both thresholds.
MAIN = options(resign_value=-0.1, resign_patience=2, draw_value=0.03, draw_patience=3)
LATE = options(resign_value=0.3, resign_patience=1, resign_min_ply=3, draw_value=0.03, draw_patience=2, draw_min_ply=1)
PROVE = options(proven=1)
NEVER = options(resign_value=-1.0, resign_patience=3)       # on, and nothing can fire within the plies played


def scenarios():
    import sigma_zero_amd as sz
    start = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    fen = lambda f: (lambda: sz.ChessTensor(fen=f))
    greedy = lambda ply: -1.0
    F = FULL
    out = []
    # 1. a reuse engine with visit targets, root noise at every ply and forced playouts: a board that resigns after two bad searches of one
    #    colour, a board adjudicated drawn on a goal-0 ply, a holdout board that gets its mark and plays on, a board nothing fires on
    out.append(Scenario("c960_endings", 64, True, True, worst_case(64), 5, [
        Board("sp400/resigns", start(400), "dyadic", 400, greedy, [F, F, 16, F, F], [0] * 5, [1] * 5, 0, "resigns"),
        Board("sp77/peaked/draw", start(77), "peaked", 77, greedy, [F, 32, 8, F, F], [0] * 5, [1] * 5, 0, "draw"),
        Board("sp200/peaked/holdout", start(200), "peaked", 200, greedy, [F, 32, F, F, 8], [0] * 5, [1] * 5, 1, "holdout_mark"),
        Board("sp959/plays_on", start(959), "dyadic", 959, _u(959), [F, F, 16, F, F], [0] * 5, [0] * 5, 0, "plays_on"),
    ], [True] * 5, [2.0, 2.0, 2.0, 0.5, 8.0], True, [MAIN] * 5))
    # 2. an engine without reuse_subtree: budgets; the option is off at ply 0 and on from ply 1; min_ply holds a full streak back; a holdout
    #    board is marked for resignation
    out.append(Scenario("budgets_endings", 64, True, True, None, 4, [
        Board("sp5/resigns", start(5), "dyadic", 5, greedy, [F, 24, F, 9], [0] * 4, [1] * 4, 0, "resigns"),
        Board("sp5/holdout", start(5), "dyadic", 5, greedy, [F, 24, F, 9], [0] * 4, [1] * 4, 1, "holdout_mark"),
        Board("sp811/plays_on", start(811), "dyadic", 811, greedy, [F, 24, F, 9], [0] * 4, [0] * 4, 0, "plays_on"),
    ], [True] * 4, [2.0] * 4, False, [None, LATE, LATE, LATE]))
    # 3. proven roots (with the solver; without it `proven` is ignored and every board plays on): the 218-move position is WIN for the mover,
    #    mated_in_2 LOSS, forced_draw DRAW; the WIN board is a holdout board, which a proof ignores.  A Chess960 engine (as forcedref's
    #    wide_forced): the sp333 board spells castling king-takes-rook, and sz_upload_game hands the engine no flag, so on a standard engine
    #    the two sides name a castling move differently once a search reaches one (under FPU's deeper trees it does, tests/fullref.py); the
    #    FEN boards have no castling rights
    out.append(Scenario("proven_endings", 64, True, True, worst_case(64), 2, [
        Board("moves_218/win/holdout", fen(WIDE_FEN), "dyadic", 1, greedy, [F] * 2, [0] * 2, [1] * 2, 1, "proven_win"),
        Board("mated_in_2/loss", fen(MATED_IN_2_FEN), "dyadic", 4, greedy, [F] * 2, [0] * 2, [1] * 2, 0, "proven_loss"),
        Board("forced_draw", fen(FORCED_DRAW_FEN), "dyadic", 3, greedy, [F] * 2, [0] * 2, [0] * 2, 0, "proven_draw"),
        Board("sp333/plays_on", start(333), "dyadic", 333, greedy, [F] * 2, [0] * 2, [1] * 2, 0, "plays_on"),
    ], [True] * 2, [4.0, 2.0], True, [PROVE] * 2))
    # 4. the second engine: the same position with the option on and `proven` off plays the proving move as always; `proven` comes on for
    #    ply 1, where the kept root of the mated_in_2 board is WIN for the side to move
    out.append(Scenario("proven_late", 64, True, True, worst_case(64), 2, [
        Board("moves_218/plays_win_move", fen(WIDE_FEN), "dyadic", 1, greedy, [F] * 2, [0] * 2, [1] * 2, 0, "plays_win_move"),
        Board("mated_in_2/late_win", fen(MATED_IN_2_FEN), "dyadic", 4, greedy, [F] * 2, [0] * 2, [1] * 2, 0, "late_win"),
        Board("forced_draw/plays_on", fen(FORCED_DRAW_FEN), "dyadic", 3, greedy, [F] * 2, [0] * 2, [0] * 2, 0, "plays_on"),
        Board("sp333/plays_on", start(333), "dyadic", 333, greedy, [F] * 2, [0] * 2, [1] * 2, 0, "plays_on"),
    ], [True] * 2, [4.0, 2.0], True, [NEVER, PROVE]))
    assert all(3 <= len(sc.boards) <= 4 and sc.plies <= 5 and sc.S == 64 and all(b.role in ROLES for b in sc.boards) for sc in out)
    return out


def new_game(sc, bd, L=1, solver=False):
    return Game(bd.make(), sc.S, sc.edges_per_board, reuse=sc.reuse, L=L, lam=1.0, solver=solver, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt)


def begin_ply(sc, g, bd, b, ply, gam):
    """the setter calls and sz_search_begin of one ply on one board"""
    g.set_endings(sc.endings[ply], bd.holdout)
    return FR.begin_ply(sc, g, bd, b, ply, gam)


def play(sc, L=1, solver=False):
    """the restatement alone: every board of the scenario through its plies"""
    games, gam = [new_game(sc, bd, L, solver) for bd in sc.boards], gammas(sc)
    for ply in range(sc.plies):
        for b, (g, bd) in enumerate(zip(games, sc.boards)):
            if g.live:
                begin_ply(sc, g, bd, b, ply, gam)
                g.run()
                if g.error is None:
                    g.play(bd.u(ply))
    return games


def role_reached(bd, g, solver):
    """whether board bd's game g did what its role says (the proven roles need the solver: without it those boards play on)"""
    played_all = g.termination is None and g.ended == [0, 0, 0, 0]
    if bd.role == "resigns":
        return g.termination == RESIGN
    if bd.role == "draw":
        return g.termination == DRAW_ADJ
    if bd.role == "holdout_mark":
        return g.termination is None and g.ended[3] == 1 and g.state.would_ply >= 0 and g.live
    if bd.role == "plays_on":
        return played_all
    if bd.role == "plays_win_move":                       # the WIN root's move, with the option on and `proven` off
        return played_all and (not solver or g.cov["win_root_played_option_on"] == 1)
    if bd.role == "late_win":                             # a LOSS root plays on while `proven` is off; the kept WIN root ends the game once it is on
        return (len(g.chosen) == 1 and g.termination == PROVEN and g.cov["proven_win"] == 1 and g.cov["ended_on_continued_ply"] == 1) if solver else played_all
    code = {"proven_win": "win", "proven_loss": "loss", "proven_draw": "draw"}[bd.role]
    return (g.termination == PROVEN and g.cov["proven_" + code] == 1) if solver else played_all


def coverage(played, hook=None):
    """played: [(Scenario, [Game])], hook: the Counter of hook_reference() -> Counter of the conditions of COVERAGE"""
    c = collections.Counter(hook or {})
    for sc, games in played:
        for g in games:
            c.update(g.cov)
            for i, k in enumerate(("resignations", "adjudicated_draws", "proven_endings", "holdout_marks")):
                c[k] += g.ended[i]
        c["option_switched_on_mid_game"] += any(a is None and b is not None for a, b in zip(sc.endings, sc.endings[1:]))
    return c


COVERAGE = ("resignations", "adjudicated_draws", "proven_endings", "holdout_marks", "holdout_fired_again", "streak_reset", "cstar_not_first",
            "played_on_with_option_on", "goal_0_ply_counted", "ended_on_continued_ply", "ended_on_goal_0_ply", "ended_forced_pruned",
            "proven_win", "proven_loss", "proven_draw", "proven_on_holdout", "win_root_played_option_on", "resign_by_white", "resign_by_black",
            "option_switched_on_mid_game", "min_ply_held", "resign_beat_draw", "nan_value", "exact_threshold", "wide_case", "cstar_tie")


# ---------------------------------------------------------------------------------------------------------------- sz_debug_endings cases
HookCases = collections.namedtuple("HookCases", "offsets N W R colour ply holdout state opts")
HOOK_K = (1, 64, 65, 218)
OPT_FIELDS = [("resign_value", np.float32), ("resign_patience", np.int32), ("resign_min_ply", np.int32), ("draw_value", np.float32),
              ("draw_patience", np.int32), ("draw_min_ply", np.int32), ("proven", np.int32)]     # sz_ending_options as a numpy record


def hook_cases(n_cases=3000, seed=31):
    """Seeded cases for sz_debug_endings: 1, 64, 65, 218 and random numbers of children, ties for c* (within and across the four lane passes),
    dyadic W / N so that m hits a dyadic threshold exactly, NaN and infinite m, streaks one short of the patience and saturated ones,
    min_ply at, below and above the ply, holdout boards with and without a mark, proven roots -> HookCases of flat arrays"""
    rng = np.random.default_rng(seed)
    Ns, Ws, off = [], [], [0]
    n = n_cases
    R, colour, ply, hold = np.zeros(n, np.int8), np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    state, opts = np.zeros((n, 6), np.int32), np.zeros(n, np.dtype(OPT_FIELDS))
    dyadic = np.array([-1.0, -0.75, -0.5, -0.25, -0.125, 0.0, 0.125, 0.25, 0.5, 0.75, 1.0])
    for i in range(n):
        k = HOOK_K[i % 6] if i % 6 < len(HOOK_K) else int(rng.integers(2, 219))
        kind = i % 11
        N = rng.integers(0, 40, size=k)
        if kind == 0:
            N[:] = rng.integers(1, 4)                                            # every child tied: c* is child 0
        if kind == 1 and k > 1:
            top = int(N.max()) + 1
            N[rng.choice(k, size=min(k, 3), replace=False)] = top                # c* tied with later children, across lane passes when k > 64
        if N.max() < 1:
            N[rng.integers(0, k)] = 1                                            # the maximum is at least 1 (k_play's zero-visit check) ...
        W = rng.uniform(-1.0, 1.0, size=k) * N
        cs = int(np.argmax(N))
        t = float(rng.choice(dyadic))
        opts[i] = (float(rng.choice(dyadic)), rng.integers(0, 4), rng.integers(0, 6), float(rng.choice(dyadic[5:])), rng.integers(0, 4), rng.integers(0, 6),
                   rng.integers(0, 2))
        if kind in (2, 3):                                                       # m exactly the resign threshold (2) / |m| exactly the draw one (3)
            N[cs] = 2 ** int(rng.integers(0, 6))
            N[np.arange(k) != cs] = np.minimum(N[np.arange(k) != cs], N[cs] - 1 if N[cs] > 1 else 0)
            cs = int(np.argmax(N))
            t = float(rng.choice(dyadic if kind == 2 else dyadic[5:]))
            sign = 1.0 if kind == 2 else float(rng.choice([-1.0, 1.0]))
            W[cs] = -(sign * t) * N[cs]                                          # exact: t dyadic, N a power of two
            opts[i]["resign_value" if kind == 2 else "draw_value"] = t
            opts[i]["resign_patience" if kind == 2 else "draw_patience"] = 1
        if kind == 4:
            N[:] = 0                                                             # ... except here: 0 / 0 = NaN, w / 0 = inf (the hook has no zero-visit check)
            W[0] = float(rng.choice([0.0, 0.0, 1.0, -1.0]))
        if kind == 5:
            W[cs] = np.nan
        state[i] = (rng.integers(0, 4), rng.integers(0, 4), rng.integers(0, 4), -1, 0, 0)
        if kind == 6:
            state[i, :3] = STREAK_MAX - int(rng.integers(0, 2))                  # saturation
            opts[i]["resign_patience"], opts[i]["draw_patience"] = STREAK_MAX, STREAK_MAX
            opts[i]["resign_value"], opts[i]["draw_value"] = 1.0, 1.0
        if kind == 7:                                                            # resign and draw both fire: |m| small, both streaks full
            W[cs] = 0.0
            opts[i] = (0.0, 1, 0, 0.0, 1, 0, 0)
        hold[i] = rng.random() < 0.3
        if hold[i] and rng.random() < 0.5:
            state[i, 3:] = (rng.integers(0, 50), rng.integers(1, 3), rng.integers(0, 2))      # already marked
        R[i] = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.int8))
        colour[i], ply[i] = rng.integers(0, 2), rng.integers(0, 8)
        Ns.append(N); Ws.append(W); off.append(off[-1] + k)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dt)
    return HookCases(np.array(off, np.int32), cat(Ns, np.int32), cat(Ws, np.float64), R, colour, ply, hold, state, opts)


def hook_reference(hc):
    """the restatement's answers to the cases -> (kind int32[n], m f64[n], state int32[n, 6], Counter)"""
    n = len(hc.R)
    kind, m, state, cov = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros((n, 6), np.int32), collections.Counter()
    with np.errstate(all="ignore"):
        for i in range(n):
            lo, hi = int(hc.offsets[i]), int(hc.offsets[i + 1])
            o = {k: hc.opts[i][k].item() for k, _ in OPT_FIELDS}
            before = State(*[int(x) for x in hc.state[i]])
            N = hc.N[lo:hi]
            kind[i], m[i], st, marked = decide(N, hc.W[lo:hi], int(hc.R[i]), int(hc.colour[i]), int(hc.ply[i]), before, o, bool(hc.holdout[i]))
            state[i] = st
            col = 1 if hc.colour[i] else 0
            cov["wide_case"] += hi - lo > 64 and int(np.argmax(N)) >= 64
            cov["cstar_tie"] += int((N == N.max()).sum()) >= 2
            cov["cstar_tie_across_passes"] += hi - lo > 64 and int((N == N.max()).sum()) >= 2 and int(np.nonzero(N == N.max())[0][-1]) >= 64 > int(np.argmax(N))
            cov["exact_threshold"] += bool(m[i] == np.float32(o["resign_value"]) and o["resign_patience"] > 0) or bool(abs(m[i]) == np.float32(o["draw_value"]) and o["draw_patience"] > 0)
            cov["nan_value"] += bool(np.isnan(m[i]))
            cov["inf_value"] += bool(np.isinf(m[i]))
            cov["negative_zero"] += bool(m[i] == 0.0 and np.signbit(m[i]))
            cov["saturated"] += kind[i] != PROVEN and STREAK_MAX in (st.rs0, st.rs1, st.ds) and STREAK_MAX in (before.rs0, before.rs1, before.ds)
            cov["hook_%s" % ("none", "resign", "draw", "proven")[kind[i]]] += 1
            cov["holdout_mark"] += marked
            cov["holdout_already_marked"] += bool(hc.holdout[i] and before.would_ply >= 0 and kind[i] == NONE and not marked
                                                  and decide(N, hc.W[lo:hi], int(hc.R[i]), col, int(hc.ply[i]), before, o, False)[0] != NONE)
            cov["proven_on_holdout"] += kind[i] == PROVEN and bool(hc.holdout[i])
            if kind[i] == RESIGN:
                cov["resign_beat_draw"] += o["draw_patience"] > 0 and st.ds >= o["draw_patience"] and hc.ply[i] >= o["draw_min_ply"]
            if kind[i] == NONE and not marked and not hc.holdout[i]:
                cov["min_ply_held"] += decide(N, hc.W[lo:hi], 0, col, int(hc.ply[i]), before, dict(o, proven=0, resign_min_ply=0, draw_min_ply=0), False)[0] != NONE
            cov["streak_reset"] += kind[i] != PROVEN and (before.rs1 if col else before.rs0) > 0 and (st.rs1 if col else st.rs0) == 0
    return kind, m, state, cov


HOOK_COVERAGE = ("wide_case", "cstar_tie", "cstar_tie_across_passes", "exact_threshold", "nan_value", "inf_value", "negative_zero", "saturated",
                 "hook_none", "hook_resign", "hook_draw", "hook_proven", "holdout_mark", "holdout_already_marked", "proven_on_holdout",
                 "resign_beat_draw", "min_ply_held", "streak_reset")
