"""The self-play options all at once as one plain-Python restatement: first-play urgency (fpuref) and the ending rules (endingref) on top of
forced playouts, visit targets, root noise, the solver and leaf batching (forcedref and below).  The two parents are siblings over forcedref;
Game(endingref.Game, fpuref.Game) has the MRO endingref -> fpuref -> forcedref -> targetref -> composeref: play() is endingref's, begin() is
fpuref's (which swaps in its Search), __init__ chains through both.  Nothing is restated here: the file only combines, and holds

  * scenarios(): endingref's role scenarios, run with FPU = fpuref.CONFIGS["red_both"] (new_game / begin_ply / play / coverage);
  * play_config(): the one args dict, the callbacks and the per-game restatement loop of sim.play_games with every option on, which
    tests/test_full_ref.py (CPU) and tests/test_gpu_full_config.py (device) share.  restate() walks the games through board slots the way
    play_games does (a slot whose game ends is refilled with the next game), so that it can say which game followed which on a slot, and
    so that the two `carry` variants can hand a refilled slot what a faulty refill would leave behind.

With fpu None it is endingref, with set_endings(None) it is fpuref (tests/test_full_ref.py pins both)."""
import collections

import numpy as np

import endingref as ER
import fpuref as FP
from endingref import DRAW_ADJ, NONE, PROVEN, RESIGN, role_reached                   # noqa: F401 (re-exported)
from forcedref import gammas, position_record, worst_case                            # noqa: F401 (re-exported)

FPU = FP.CONFIGS["red_both"]
OPTIONS = ER.OPTIONS                                       # (L, solver): the two pairs the play_games comparison runs under
RUNS = [(L, solver) for L in (1, 4) for solver in (False, True)]      # ... and the four the role scenarios run under: every board keeps its role


class Game(ER.Game, FP.Game):
    """every option in one board: endingref's play() over fpuref's begin()"""


def fpu_args(fp):
    """an Fpu as args["fpu"]"""
    return None if fp is None else {"mode": FP.MODE_NAMES[fp.tree_mode], "value": fp.tree_value, "root_mode": FP.MODE_NAMES[fp.root_mode], "root_value": fp.root_value}


# ---------------------------------------------------------------------------------------------------------------- role scenarios
def scenarios():
    return ER.scenarios()


def new_game(sc, bd, L=1, solver=False, fpu=FPU):
    return Game(bd.make(), sc.S, sc.edges_per_board, reuse=sc.reuse, L=L, lam=1.0, solver=solver, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt, fpu=fpu)


begin_ply = ER.begin_ply                                   # the setter calls and sz_search_begin of one ply on one board (the FPU setting stays)


def play(sc, L=1, solver=False, fpu=FPU):
    """the restatement alone: every board of the scenario through its plies"""
    games, gam = [new_game(sc, bd, L, solver, fpu) for bd in sc.boards], gammas(sc)
    for ply in range(sc.plies):
        for b, (g, bd) in enumerate(zip(games, sc.boards)):
            if g.live:
                begin_ply(sc, g, bd, b, ply, gam)
                g.run()
                if g.error is None:
                    g.play(bd.u(ply))
    return games


def coverage(games):
    """games: [Game] -> the counters of both parents merged: every Game.cov once, endingref's ending counts, forcedref's two sums"""
    c = collections.Counter()
    for g in games:
        c.update(g.cov)
        for i, k in enumerate(("resignations", "adjudicated_draws", "proven_endings", "holdout_marks")):
            c[k] += g.ended[i]
        c["forced_selections"] += g.forced_selections
        c["pruned_visits"] += g.pruned_visits
    return c


# what the combination is there for: the clamp of FPU's reduction, a forced child against FPU's choice, every way a game ends, on kept and
# on forced, pruned searches
COVERAGE = ("clamp_low", "forced_overruled_fpu", "ended_resign", "ended_draw", "holdout_mark", "ended_on_continued_ply", "ended_forced_pruned")
SOLVER_COVERAGE = ("ended_proven", "win_root_played_option_on")


def assert_coverage(cov, solver):
    names = COVERAGE + (SOLVER_COVERAGE if solver else ())
    missing = [k for k in names if cov[k] < 1]
    assert not missing, "conditions not reached: %s of %s" % (missing, dict(cov))


# ---------------------------------------------------------------------------------------------------------------- play_games, everything on
KIND = {RESIGN: "resign", DRAW_ADJ: "draw_adjudicated", PROVEN: "proven"}
RESULT = {1: "1-0", -1: "0-1", 0: "1/2-1/2"}
RECORD_KEYS = ("chosen_actions", "sample_plies", "actions", "packed_states", "colours", "result", "rewards", "termination", "would_end", "holdout")
STAT_KEYS = ("sims", "full_plies", "fast_plies", "forced_selections", "pruned_visits", "resigned", "adjudicated_draws", "adjudicated_proven",
             "holdout_games", "holdout_marks")
PlayConfig = collections.namedtuple("PlayConfig", "S fast salt mode starts caps held forced_k endings draws uniforms full_search root_gamma holdout")

# Chosen on the CPU from the m this restatement sees in these games (|m| runs from 0.005 to 0.6): with both (L, solver) pairs a game resigns,
# a game is adjudicated drawn early enough for its slot to be refilled, a holdout game gets its mark and games are cut at max_plies; and
# with the caps of play_config() the games that follow on a slot are games whose records change when they inherit the streaks or the mark
# of the game before them.  tests/test_full_ref.py asserts all of it.  `proven` joins them where the solver runs (args_of, restate).
ENDINGS = {"resign_value": -0.05, "resign_patience": 2, "resign_min_ply": 1, "draw_value": 0.13, "draw_patience": 2, "draw_min_ply": 0}


def play_config():
    """The configuration of the play_games tests: 8 Chess960 games, every option on.  -> PlayConfig; args_of(cfg, L, solver) is the args dict,
    the four callbacks are play_games' keyword arguments, restate(cfg, L, solver) the games the restatement plays"""
    draws = np.random.default_rng(12).standard_gamma(0.3, size=(8, 8, ER.MAX_MOVES)).astype(np.float32)
    held = [False, False, True, False, False, True, False, False]
    return PlayConfig(S=32, fast=8, salt=4, mode="dyadic", starts=[0, 959, 518, 400, 77, 5, 811, 333], caps=[6, 3, 5, 6, 3, 6, 5, 6], held=held, forced_k=2.0,
                      endings=dict(ENDINGS), draws=draws,
                      uniforms=lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0,
                      full_search=lambda g, ply: (g + ply) % 2 == 0,
                      root_gamma=lambda g, ply: draws[g, ply],
                      holdout=lambda g: held[g])


def args_of(cfg, L, solver, fpu=FPU, endings="config"):
    """args of play_games for one (L, solver) pair: the solver and leaf batching are the two keys the second pair leaves out"""
    end = dict(cfg.endings if endings == "config" else endings, proven=bool(solver), holdout=0.25)
    args = {"C": 2, "num_searches": cfg.S, "reuse_subtree": True, "visit_targets": True, "combine_options": True,
            "playout_cap": {"fast": cfg.fast, "p_full": 0.5}, "root_dirichlet_alpha": 0.3, "quiet_fast_plies": True, "forced_playouts": cfg.forced_k,
            "fpu": fpu_args(fpu), "endings": end}
    if L != 1:
        args.update(leaves_per_step=L, virtual_loss=1.0)
    if solver:
        args["solver"] = True
    return args


def _moves(actions, white):
    from sigma_zero_amd.chess_tensor import index_to_move
    return [index_to_move(int(a), bool(white)) for a in actions]        # no pawn reaches the last rank within the plies played here


def restate(cfg, L, solver, n_slots=None, carry=None, endings="config", fpu=FPU):
    """The games of play_games(args_of(cfg, L, solver), ...) on the restatement, walked through n_slots board slots in play_games' order
    (default: one slot per game).  Without `carry` every game starts from nothing, so its record does not depend on n_slots.
    carry = "endings": a refilled slot's game inherits the EndState of the game before it on that slot (set_endings without
    reset_endings); carry = "subtree": it inherits that game's kept subtree (`next`).  Both are bugs a refill could have.
    -> (records: per game a dict with RECORD_KEYS, stats: dict with STAT_KEYS, games: [Game], refills: [(slot, game before, game)])"""
    import sigma_zero_amd as sz
    n = len(cfg.starts)
    B = n if n_slots is None else min(n, int(n_slots))
    opts = ER.options(**(cfg.endings if endings == "config" else endings), proven=int(bool(solver)))
    games, fulls, recs, broke = [None] * n, [[] for _ in range(n)], [[] for _ in range(n)], [None] * n
    slot, last, refills, nxt = [-1] * B, [None] * B, [], 0

    def start(s):
        nonlocal nxt
        if nxt >= n:
            slot[s] = -1
            return
        g = nxt
        nxt += 1
        ref = Game(sz.ChessTensor(chess960=True, scharnagl=cfg.starts[g]), cfg.S, worst_case(cfg.S), reuse=True, L=L, lam=1.0, solver=solver, c=2.0,
                   learning=True, mode=cfg.mode, salt=cfg.salt, fpu=fpu)
        ref.set_endings(opts, cfg.held[g])
        if last[s] is not None:
            refills.append((s, last[s], g))
            if carry == "endings":
                ref.state = games[last[s]].state
            if carry == "subtree":                       # the noise mode is the engine's, not the game's: nothing drops the subtree
                ref.next, ref.noise_on = games[last[s]].next, True
        games[g], slot[s] = ref, g

    for s in range(B):
        start(s)
    while any(g >= 0 for g in slot):
        done = []
        for s in range(B):
            g = slot[s]
            if g < 0:
                continue
            ref, ply = games[g], len(recs[g])
            full = bool(cfg.full_search(g, ply))
            try:
                ref.set_root_noise(True)
                ref.begin(cfg.S if full else cfg.fast, cfg.root_gamma(g, ply), not full, cfg.forced_k if full else 0.0)
                ref.run()
                assert ref.error is None, ref.error
                recs[g].append(ref.play(cfg.uniforms(g, ply)))
            except Exception as e:                       # only a carried subtree of another game can do this: its moves are not this game's
                assert carry == "subtree", (g, ply, e)
                broke[g] = "%s: %s" % (type(e).__name__, e)
                recs[g].append(None)
                ref.over = True
            fulls[g].append(full)
            if not ref.live or len(recs[g]) >= cfg.caps[g]:
                done.append(s)
        for s in done:
            last[s] = slot[s]
            start(s)
    records, stats = [], collections.Counter({k: 0 for k in STAT_KEYS})
    for g, ref in enumerate(games):
        if broke[g] is not None:
            records.append({"broken": broke[g]})
            continue
        r = dict(chosen_actions=list(ref.chosen), sample_plies=[], actions=[], packed_states=[], colours=[], holdout=bool(cfg.held[g]))
        for ply, (rec, full) in enumerate(zip(recs[g], fulls[g])):
            if not full:
                continue
            k = int(rec["n_child"])
            vis = rec["visits"][:k].astype(np.int64)
            r["sample_plies"].append(ply)
            r["actions"].append((_moves(rec["action"][:k], rec["colour"]), (vis / int(vis.sum())).tolist()))
            r["packed_states"].append(rec["packed"].tobytes())
            r["colours"].append(bool(rec["colour"]))
        r["result"] = RESULT[ref.result] if ref.over else None
        reward = {"1-0": 1, "0-1": -1}.get(r["result"], 0)
        r["rewards"] = [reward if p % 2 == 0 else -reward for p in r["sample_plies"]]
        r["termination"] = KIND[ref.termination] if ref.termination is not None else ("rules" if ref.over else "max_plies")
        st = ref.state
        r["would_end"] = None if st.would_ply < 0 else {"kind": KIND[st.would_kind], "ply": st.would_ply, "colour": st.would_colour}
        records.append(r)
        stats["sims"] += sum(ref.goals)
        stats["full_plies"] += sum(fulls[g])
        stats["fast_plies"] += len(fulls[g]) - sum(fulls[g])
        stats["forced_selections"] += ref.forced_selections
        stats["pruned_visits"] += ref.pruned_visits
        for i, k in enumerate(("resigned", "adjudicated_draws", "adjudicated_proven", "holdout_marks")):
            stats[k] += ref.ended[i]
        stats["holdout_games"] += bool(cfg.held[g])
    return records, dict(stats), games, refills


def record_of(game):
    """a game dict of play_games in the form of restate()'s records"""
    r = {k: game[k] for k in RECORD_KEYS}
    r["actions"] = [(list(a.keys()), list(a.values())) for a in game["actions"]]
    r["packed_states"] = [np.ascontiguousarray(p).tobytes() for p in game["packed_states"]]
    return r
