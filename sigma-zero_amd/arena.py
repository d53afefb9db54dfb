"""Model-vs-model gating matches on the GPU engine (the role of /root/reference/test_update.py:12-97 and the
search-then-argmax usage of eval.py:92-94, play.py:40-41): both networks play greedy (`max` visit count) with
learning=False; every game is one board of a batch, colours alternate over the boards."""
import numpy as np
import torch

from .selfplay import SelfPlayEngine, temperature_options_of, temperature_at


@torch.no_grad()
def play_match(model_a, model_b, args, n_games, chess960=False, scharnagl=None, max_plies=512, planes_dtype=None, device="cuda:0"):
    """Returns {'a_wins', 'b_wins', 'draws', 'unfinished', 'results'}; model_a has white on even boards, black on odd ones."""
    import random
    if planes_dtype is None:
        planes_dtype = ("bits128" if getattr(model_a, "w16", False) and getattr(model_b, "w16", False) else "nhwc128") if hasattr(model_a, "tower") else torch.float32
    eng = SelfPlayEngine(None, args, n_games, chess960=chess960, learning=False, device=device, planes_dtype=planes_dtype)
    if chess960 and scharnagl is None:
        scharnagl = [random.randint(0, 959) for _ in range(n_games)]
    eng.new_games(scharnagl if chess960 else [-1] * n_games)
    a_is_white = (np.arange(n_games) % 2 == 0)
    results = np.full(n_games, 2, dtype=np.int8)            # +1 white won, -1 black won, 0 draw, 2 unfinished
    L = eng.L                                               # args["leaves_per_step"]: board b's leaves are network rows b*L .. b*L+L-1
    idx_dev = torch.arange(n_games * L, device=eng.device)
    for ply in range(max_plies):
        white_to_move = (ply % 2 == 0)                      # all games start together: one side to move per ply
        a_moves = torch.as_tensor(np.repeat(a_is_white == white_to_move, L), device=eng.device)
        ia, ib = idx_dev[a_moves], idx_dev[~a_moves]

        def evaluator(planes):
            policy = torch.empty(n_games * L, 4672, dtype=torch.float32, device=eng.device)
            value = torch.empty(n_games * L, dtype=torch.float32, device=eng.device)
            for model, ii in ((model_a, ia), (model_b, ib)):
                if ii.numel():
                    p, v = model(planes[ii].contiguous(), inference=True)
                    policy[ii] = p.float()
                    value[ii] = v.float().reshape(-1)
            return policy, value

        eng.search(evaluator)
        eng.check_errors()
        eng.play(np.full(n_games, -1.0))                    # greedy
        rec = eng.fetch_ply()
        over = rec["game_over"].astype(bool) & rec["active"].astype(bool)
        results[over] = rec["result"][over]
        if not (results == 2).any():
            break
    eng.close()
    a_score = np.where(a_is_white, results, -results)
    return {"a_wins": int(((a_score == 1) & (results != 2)).sum()), "b_wins": int(((a_score == -1) & (results != 2)).sum()),
            "draws": int((results == 0).sum()), "unfinished": int((results == 2).sum()), "results": results.tolist()}


SCORE_CLIP = 1e-3                                           # match_stats maps scores through the Elo formula inside [SCORE_CLIP, 1 - SCORE_CLIP]
Z95 = 1.959963984540054                                     # the 97.5 % point of the standard normal


def elo_of(score):
    """-400 * log10(1 / s - 1) with s clipped to [SCORE_CLIP, 1 - SCORE_CLIP] (s = 0 and s = 1 have no finite Elo difference)"""
    s = min(max(float(score), SCORE_CLIP), 1.0 - SCORE_CLIP)
    return -400.0 * float(np.log10(1.0 / s - 1.0)) + 0.0    # + 0.0: an even score reads 0.0, not -0.0


def match_stats(results_a):
    """Statistics of a match played in colour-swapped pairs.  results_a: per game, from configuration A's view, 1 = A won, 0 = draw, -1 = A
    lost, 2 = unfinished; games 2i and 2i+1 are pair i.  A pair with an unfinished game counts in `unfinished` alone.

    With g = (r + 1) / 2 the points of a game, pair i scores x_i = (g_2i + g_2i+1) / 2 in {0, 1/4, 1/2, 3/4, 1} and, over the n pairs,
        score     s   = sum(x_i) / n
        variance  var = sum((x_i - s)^2) / n                (of the pair score over the pairs: the two games of a pair share an opening, so the
                                                             pair and not the game is the independent unit)
        interval  s -+ Z95 * sqrt(var / n), cut to [0, 1]   (95 %, normal approximation)
        elo       -400 * log10(1 / s - 1), likewise elo_lo and elo_hi from the interval's ends; s is clipped to [SCORE_CLIP, 1 - SCORE_CLIP] first,
                  so a clean sweep reads +-1199.8 and not infinity.
    pentanomial[k] counts the pairs with k/2 points for A (k = 0..4).  Returns a dict; with no finished pair the figures are None."""
    r = np.asarray(results_a, dtype=np.int64).reshape(-1)
    if r.size % 2:
        raise ValueError("match_stats: games come in pairs, got %d results" % r.size)
    if not np.isin(r, (-1, 0, 1, 2)).all():
        raise ValueError("match_stats: results are 1, 0, -1 or 2 (unfinished)")
    done = r != 2
    pairs = r.reshape(-1, 2)[done.reshape(-1, 2).all(axis=1)]
    out = {"wins": int((r == 1).sum()), "draws": int((r == 0).sum()), "losses": int((r == -1).sum()), "unfinished": int((r == 2).sum()),
           "pairs": int(len(pairs)), "pentanomial": [0] * 5, "score": None, "variance": None, "score_lo": None, "score_hi": None,
           "elo": None, "elo_lo": None, "elo_hi": None}
    if not len(pairs):
        return out
    twice = (pairs + 1).sum(axis=1)                         # 2 * the pair's points: 0..4
    out["pentanomial"] = [int((twice == k).sum()) for k in range(5)]
    x = twice.astype(np.float64) / 4.0
    n = len(x)
    s = float(x.sum() / n)
    var = float(((x - s) ** 2).sum() / n)
    half = Z95 * float(np.sqrt(var / n))
    lo, hi = max(0.0, s - half), min(1.0, s + half)
    out.update(score=s, variance=var, score_lo=lo, score_hi=hi, elo=elo_of(s), elo_lo=elo_of(lo), elo_hi=elo_of(hi))
    return out


@torch.no_grad()
def play_options_match(model, args_a, args_b, n_pairs, chess960=True, scharnagl=None, openings=None, sample_plies=0, seed=0, max_plies=512,
                       model_b=None, device="cuda:0", edges_per_board=None, planes_dtype=None, check_positions=False, timing=None):
    """Search configuration A against configuration B: two engines, one per configuration, play 2 * n_pairs games against each other.

    args_a / args_b are engine args (num_searches, C and any search option); `model` evaluates for both unless model_b is given for B.  Games
    2i and 2i+1 are a pair: the same start (scharnagl[i]; drawn from default_rng(seed) when chess960 and None) and the same opening
    (openings[i % len(openings)], a list of action indices played into both engines before the first search), A white in game 2i and black
    in game 2i+1.  Each side's first sample_plies moves are sampled from the visits with uniforms of default_rng(seed); later moves are greedy.
    A side whose args have "temperature" (selfplay.temperature_options_of) samples every move with uniforms of default_rng(seed) at the
    temperature its schedule gives for the GAME's ply (opening included; a final temperature of 0 plays the most visited move); sample_plies
    must be 0 then (ValueError otherwise): the two are the same control.
    A side whose args have "lcb" (selfplay.lcb_options_of) plays its greedy moves by the lower-confidence bound, through its engine: no rule
    of the arena's own.

    One ply: each engine has exactly the boards active where its side is to move (set_active + compact), searches them, plays, and hands
    the chosen moves to the other engine by play_moves (sz_play_moves), which re-roots that engine's kept subtree on a reuse_subtree
    configuration.  An ending of args[...]["endings"] (chosen -1, game over) ends the game for both.  After every ply both engines must agree
    on game_over and result (AssertionError otherwise); check_positions=True also compares their 80-byte position records.

    edges_per_board: child slots per board of both engines (default: the worst case of each configuration; never 0, which would size the
    first engine to half of the free HBM).  timing: a dict that receives seconds_per_ply_a / _b (search + play + fetch, per searched ply) and
    searched_plies_a / _b.  Returns match_stats(results from A's view) plus "results" (per game: 1 white won, -1 black won, 0 draw, 2
    unfinished), "results_a" and "plies"."""
    import time
    n = 2 * int(n_pairs)
    if n <= 0:
        raise ValueError("play_options_match: n_pairs must be positive")
    model_b = model if model_b is None else model_b
    if planes_dtype is None:
        planes_dtype = ("bits128" if getattr(model, "w16", False) and getattr(model_b, "w16", False) else "nhwc128") if hasattr(model, "tower") else torch.float32
    rng = np.random.default_rng(seed)
    temps = [temperature_options_of(args_a), temperature_options_of(args_b)]
    if any(t is not None for t in temps) and sample_plies != 0:
        raise ValueError("play_options_match: a side with args['temperature'] needs sample_plies == 0 (the schedule says which plies are sampled)")
    if chess960:
        sch = rng.integers(0, 960, size=n_pairs) if scharnagl is None else np.asarray(scharnagl, np.int64).reshape(-1)
        if len(sch) != n_pairs:
            raise ValueError("play_options_match: %d Scharnagl numbers for %d pairs" % (len(sch), n_pairs))
        starts = np.repeat(sch, 2).astype(np.int32)
    else:
        starts = np.full(n, -1, np.int32)
    engines = []
    for m, args in ((model, args_a), (model_b, args_b)):
        cap = edges_per_board if edges_per_board else (2 if args.get("reuse_subtree", False) else 1) * int(args["num_searches"]) * 218 + 2
        engines.append(SelfPlayEngine(m, args, n, chess960=chess960, learning=False, device=device, planes_dtype=planes_dtype, edges_per_board=int(cap)))
    for e in engines:                                       # both engines exist before any game starts
        e.new_games(starts)
    plies = np.zeros(n, np.int64)                           # plies played per game, opening included
    moves_made = np.zeros((2, n), np.int64)                 # moves a side has chosen itself (the sampled ones come first)
    if openings:
        book = [list(openings[(g // 2) % len(openings)]) for g in range(n)]
        for k in range(max(len(b) for b in book)):
            acts = np.array([b[k] if k < len(b) else -1 for b in book], np.int32)
            for e in engines:
                e.play_moves(acts)
            plies += acts >= 0
        for e in engines:
            e.check_errors()
    a_is_white = np.arange(n) % 2 == 0
    results = np.full(n, 2, np.int8)
    spent, searched = [0.0, 0.0], [0, 0]
    for _ in range(int(max_plies)):
        live = results == 2
        if not live.any():
            break
        white_to_move = plies % 2 == 0
        to_move = [live & (a_is_white == white_to_move), live & (a_is_white != white_to_move)]
        draws = rng.random(n) if sample_plies > 0 or any(t is not None for t in temps) else None
        given = [np.full(n, -1, np.int32), np.full(n, -1, np.int32)]        # what each engine receives from the other
        recs = [None, None]
        for k, e in enumerate(engines):
            if not to_move[k].any():
                continue
            t0 = time.perf_counter()
            e.set_active(to_move[k])
            e.compact()
            e.search()
            e.check_errors()
            u = np.full(n, -1.0)
            if temps[k] is not None:                      # every move is the rule's: the schedule by game ply decides what is sampled
                u[to_move[k]] = draws[to_move[k]]
                e.set_temperatures([temperature_at(temps[k], int(p)) for p in plies])
            elif draws is not None:
                sample = to_move[k] & (moves_made[k] < sample_plies)
                u[sample] = draws[sample]
            e.play(u)
            rec = recs[k] = e.fetch_ply()
            spent[k] += time.perf_counter() - t0
            searched[k] += 1
            assert np.array_equal(rec["active"].astype(bool), to_move[k]), "play_options_match: the boards that played are not the boards to move"
            given[1 - k] = np.where(to_move[k], rec["chosen"], -1).astype(np.int32)
            moves_made[k] += to_move[k]
        for k, e in enumerate(engines):
            if (given[k] >= 0).any():
                e.play_moves(given[k])
        for k, e in enumerate(engines):                     # the receiver's view of the moves of the other side
            if recs[1 - k] is None:
                continue
            moved = given[k] >= 0
            if moved.any():
                e.check_errors()
                got, want = e.fetch_ply(), recs[1 - k]
                for key in ("chosen", "game_over", "result"):
                    assert np.array_equal(got[key][moved], want[key][moved]), "play_options_match: the engines disagree on %s after a ply" % key
        for k in range(2):
            if recs[k] is None:
                continue
            over = to_move[k] & recs[k]["game_over"].astype(bool)
            results[over] = recs[k]["result"][over]
            plies += to_move[k] & (recs[k]["chosen"] >= 0)
        if check_positions:
            for g in np.nonzero(results == 2)[0]:
                (pa, la), (pb, lb) = engines[0].debug_position(int(g)), engines[1].debug_position(int(g))
                assert la == lb == plies[g] and pa.tobytes() == pb.tobytes(), "play_options_match: the engines hold different positions on board %d" % g
    final = [[e.debug_position(g) for g in range(n)] for e in engines] if check_positions else None
    for e in engines:
        e.close()
    results_a = np.where(results == 2, 2, np.where(a_is_white, results, -results)).astype(np.int8)
    out = match_stats(results_a)
    out.update(results=results.tolist(), results_a=results_a.tolist(), plies=plies.tolist())
    if timing is not None:
        timing.update(seconds_per_ply_a=spent[0] / max(searched[0], 1), seconds_per_ply_b=spent[1] / max(searched[1], 1),
                      searched_plies_a=searched[0], searched_plies_b=searched[1])
        if final is not None:
            timing["final_positions"] = [[(p.tobytes(), l) for p, l in side] for side in final]
    return out
