"""Self-play of /root/reference/sim.py:31-123 — same functions, same return dict — with all games of a
call advanced concurrently on the GPU (one board per game, lock-step searches, one batched network call
per simulation)."""
import os

import numpy as np
import torch

from .chess_tensor import Move, index_to_move, QUEEN
from .selfplay import SelfPlayEngine, unpack_planes, model_device, visit_target_options_of, forced_playout_options_of, ending_options_of, gumbel_options_of, gumbel_tree_of, temperature_options_of, temperature_at, search_targets_of, lcb_options_of, ENDING_KINDS

device = "cuda" if torch.cuda.is_available() else "cpu"      # module global of the reference (sim.py:12); the engine itself follows the model's device


_DECODE = {}            # colour -> (from[4672], to[4672], promo[4672], maybe_queen[4672]) int arrays; from = -1 where the index leaves the board
_MOVES = {}             # (from, to, promo) -> Move: one shared object per distinct move (treat the Moves of a record as read-only)


def _decode_tables(colour_white):
    """index -> (from, to, under-promotion piece) for one colour, computed once with index_to_move (tensorToAction, chess_tensor.py:309-410)"""
    if colour_white not in _DECODE:
        frm = np.full(4672, -1, np.int64); to = np.zeros(4672, np.int64); pr = np.zeros(4672, np.int64); mq = np.zeros(4672, bool)
        for a in range(4672):
            try:
                mv = index_to_move(a, colour_white)
            except IndexError:
                continue
            frm[a], to[a], pr[a] = mv.from_square, mv.to_square, mv.promotion or 0
            plane, cell = divmod(a, 64)
            mq[a] = plane < 56 and cell // 8 == 1 and plane // 7 in (0, 1, 7) and plane % 7 == 0       # one step up / up-diagonal from view row 1
        _DECODE[colour_white] = (frm, to, pr, mq)
    return _DECODE[colour_white]


def _moves_for_record(action_idx, colour_white, packed_root):
    """Decode child action indices of one root into Move objects.  A sliding-plane move of a pawn from the
    7th to the 8th rank (mover's view rows 1 -> 0) is a queen promotion (tensorToAction + queen_promotion dict)."""
    frm, to, pr, mq = _decode_tables(bool(colour_white))
    a = np.asarray(action_idx, dtype=np.int64)
    f, t, p = frm[a], to[a], pr[a].copy()
    cand = mq[a]
    if cand.any():
        own_pawn_row1 = int(packed_root[0][1])                # plane 0 = mover's pawns, view row 1: bit j = column j
        cols = a[cand] % 8
        p[np.nonzero(cand)[0][((own_pawn_row1 >> cols) & 1).astype(bool)]] = QUEEN
    moves = []
    for key in zip(f.tolist(), t.tolist(), p.tolist()):
        mv = _MOVES.get(key)
        if mv is None:
            mv = _MOVES[key] = Move(key[0], key[1], key[2] or None)
        moves.append(mv)
    return moves


def playout_cap_of(args):
    """args["playout_cap"] = {"fast": n_fast, "p_full": p} checked against args["num_searches"]: (n_fast, p), or None when the option is off"""
    cap = args.get("playout_cap")
    if cap is None:
        return None
    full = int(args["num_searches"])
    if not isinstance(cap, dict) or set(cap) != {"fast", "p_full"}:
        raise ValueError("args['playout_cap'] must be {'fast': n_fast, 'p_full': p}, got %r" % (cap,))
    fast, p = cap["fast"], cap["p_full"]
    if isinstance(fast, bool) or not isinstance(fast, (int, np.integer)) or not 2 <= fast <= full:
        raise ValueError("args['playout_cap']['fast'] must be an integer in 2..num_searches (%d), got %r" % (full, fast))
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= p <= 1.0:       # NaN fails both comparisons
        raise ValueError("args['playout_cap']['p_full'] must be a probability in [0, 1], got %r" % (p,))
    if args.get("reuse_subtree", False) and not visit_target_options_of(args)[0]:
        raise ValueError("args['playout_cap'] and args['reuse_subtree'] exclude each other (sz_set_search_budgets)")
    return int(fast), float(p)


def play_games(model, args, n_games, c960=False, scharnagl=None, uniforms=None, learning=True, planes_dtype=None, max_plies=100000,
               verbose=False, n_boards=None, compact=True, stats=None, full_search=None, root_gamma=None, holdout=None, gumbel_noise=None, temperature=None):
    """Plays n_games games to the end and returns a list of per-game history dicts (sim.py:38-43 layout), game g at index g.

    The games run concurrently on `n_boards` board slots of one engine (default: one slot per game).  A slot whose game ends is
    REFILLED with the next game that has not started yet, so the GPU stays full until fewer than n_boards games remain; from then
    on the batch is COMPACTED (sz_compact): the network only evaluates the boards that still play.  With the MFMA networks
    (FastPolicyNet, SplitPolicyNet) a game's results do not depend on the slot it runs in, on the batch size or on what runs beside it —
    bit for bit (their kernels are per board and every reduction has a fixed order; tests/test_gpu_train_and_precision.py).  A plain
    torch module goes through MIOpen / hipBLASLt, whose algorithm choice and hence rounding can change with the batch size: there the
    records are reproducible for a fixed (n_games, n_boards) schedule only; pass compact=False to keep the batch size constant.

    scharnagl: start index per game (default: python `random.randint(0,959)` per game like chess_tensor.py:69, drawn in game order).
    uniforms(game, ply) -> float: the np.random.random_sample() draw of sim.py:68.  Default: the global numpy RNG, drawn once per ply
      for every running game in game order (n_games == 1 reproduces the reference's stream; for several concurrent games the order of
      the draws necessarily differs from the reference's one-game-after-another order — generate_training_data(rng_order="reference")).
    max_plies: a game still running after that many plies is cut (result None, rewards 0); one number or one per game.
    stats: optional dict, receives 'sims', 'nn_rows', 'plies' (work done; sims = new simulations, nn_rows = network rows evaluated), 'full_plies' / 'fast_plies' (game
      plies searched with the full / the fast budget), 'searches_without_network' (lock-step searches that made no network call: args["visit_targets"]) and 'host_seconds' (the host's wall time per phase of the ply loop: enqueue_search returns before the GPU is done,
      wait_search is the wait for it), 'forced_selections' / 'pruned_visits' (sz_forced_stats; 0 without args["forced_playouts"]), 'resigned' /
      'adjudicated_draws' / 'adjudicated_proven' / 'holdout_marks' (sz_ending_stats) and 'holdout_games' (0 without args["endings"]),
      and, with args["temperature"] only, 'tempered_plays' / 'greedy_plays' / 'excluded_children' (sz_temperature_stats).
    Every game dict has 'termination', one of "rules" | "resign" | "draw_adjudicated" | "proven" | "max_plies", 'holdout' (the game was a holdout
      game) and 'would_end', None or {"kind", "ply", "colour"}: the first ply at which a rule would have ended a holdout game.

    NON-REFERENCE option, off by default (the reference searches every ply with args['num_searches'] and records every ply, sim.py:46-76):
    args["playout_cap"] = {"fast": n_fast, "p_full": p}, playout-cap randomisation (KataGo).  Per ply every running game is searched with the
    full budget args["num_searches"] with probability p, else with n_fast simulations (2 <= n_fast <= num_searches); every ply is played, but ONLY
    full-search plies become training samples (states / actions / colours / packed_states); the game dict's 'sample_plies' lists the ply of
    each sample and 'rewards' takes its sign from that ply.  The batch shrinks to the full-search boards once the fast ones are done
    (SelfPlayEngine.search).  Noise is the same on fast and full plies (`learning` is per engine); so is the sampling temperature unless
    args["temperature"]["fast"] says otherwise.
    args["visit_targets"] = True (NON-REFERENCE, selfplay.visit_target_options_of): playout_cap and root_dirichlet_alpha together with
    args["reuse_subtree"].  The per-ply numbers np.where(sampled, num_searches, n_fast) are then root visit TARGETS: the visits of the kept
    subtree count, stats['sims'] are the new simulations actually made, and the root is noised at every ply.  With
    args["quiet_fast_plies"] = True fast plies are searched without root noise; their sampling temperature is args["temperature"]["fast"]
    (KataGo's "no temperature on fast plies" is fast: 0.0).  Strength effect unmeasured.
    args["forced_playouts"] = k (NON-REFERENCE, selfplay.forced_playout_options_of): forced playouts at the root and policy-target pruning of the
    record ('actions' are the pruned visit fractions; the move is sampled from them).  With args["playout_cap"] only full-search plies are forced
    (fast plies are not recorded, and KataGo leaves them un-forced); without it every ply is.  Needs learning.  Strength effect unmeasured.
    args["endings"] = {...} (NON-REFERENCE, selfplay.ending_options_of): resignation and adjudicated game endings (sz_set_endings).  A game a rule
    ends gets its result without a move: the ending ply is a training sample like any other recorded ply (with args["playout_cap"] only if it
    was a full-search ply), 'chosen_actions' gets no entry for it, and 'rewards' follow from 'result' as always.  A refill hands the engine the
    holdout flags of the games it starts.  The extra per-ply host copy (sz_fetch_endings) happens in this mode only.  Strength effect unmeasured.
    args["fpu"] = {...} (NON-REFERENCE, selfplay.fpu_options_of): first-play urgency, what selection takes an unvisited child to be worth
    (sz_set_fpu), one setting for the root and one below it, on fast and full plies alike; the engine applies it.  Strength effect unmeasured.
    args["cpuct"] = {...} (NON-REFERENCE, selfplay.cpuct_options_of): AlphaZero's visit-dependent exploration rate in the place of the constant
    C (sz_set_cpuct), one triple for the root and one below it, on fast and full plies alike; the engine applies it.  Strength effect unmeasured.
    args["kld_stop"] = {...} (NON-REFERENCE, selfplay.kld_stop_options_of): KLD-gain early stopping (sz_set_kld_stop), on fast and full plies
    alike: SelfPlayEngine.search checks every board's root every `interval` visits and a board whose visit distribution has stopped moving makes
    no further simulation; stats['sims'] stay the goals the searches began with (kld_stop_stats() has what was not made).  Strength effect unmeasured.
    args["search_targets"] = {...} (NON-REFERENCE, selfplay.search_targets_of): the search summary (sz_set_search_summary) is fetched after every
    play(); a game gets 'search_values' (the search's own value of each sampled position from the mover's side, root_q or best_q by q_source),
    'surprises' (its policy surprise KL(target || prior)) and 'value_targets' ((1 - q_ratio) * reward + q_ratio * search value, Python floats),
    all aligned with 'states'.  'rewards', 'actions' and the moves played are what they are without
    the key; train_rl takes the blended targets and the surprise weights from there.  Effect on training unmeasured.
    args["lcb"] = {...} (NON-REFERENCE, selfplay.lcb_options_of): the engine keeps every edge's value spread and plays the lower-confidence-bound
    move where a play is greedy (a negative uniform; T = 0 under args["temperature"]); sampled plays and every sample's fields are what they are
    without the key.  stats gains 'lcb_decided' / 'lcb_differs' (sz_lcb_stats).  Strength effect unmeasured.
    args["gumbel"] = {"m": m, "c_visit": x, "c_scale": y} (NON-REFERENCE, selfplay.gumbel_options_of): the Gumbel root search (sz_set_gumbel), on fast
    and full plies alike.  The move is the search's own choice (`uniforms` is still drawn as always and not read by the engine) and a sample's
    'actions' dict holds the completed-Q improved policy as Python floats instead of visit fractions.  With `learning` the Gumbel(0,1) draws
    g = -log(-log(u)) come per board and ply from a numpy Generator of its own; without it g is NULL, a deterministic search for match play.
    stats gets 'gumbel_fallbacks' (sz_gumbel_stats: root selections that found no child at their level, 0).  Strength effect unmeasured.
    args["gumbel_tree"] = True (NON-REFERENCE, selfplay.gumbel_tree_of; needs args["gumbel"]): below the root of every Gumbel search the
    completed-Q selection of sz_set_gumbel_tree replaces PUCT; the engine applies it and the per-ply set_gumbel leaves it on.  Strength effect unmeasured.
    args["temperature"] = {...} (NON-REFERENCE, selfplay.temperature_options_of): the move-selection temperature with lc0's visit offset and
    value cutoff (sz_set_move_temperature).  Every running game's temperature is computed at every ply from THAT GAME's ply (a game that starts
    on a refilled slot starts at t0 again) by selfplay.temperature_at, with full = the ply's full / fast decision under args["playout_cap"].
    The record is not tempered: 'actions' stay the visit fractions.  With the key absent nothing is drawn or consumed differently.
    Strength effect unmeasured.
    temperature(game, ply) -> float >= 0: that game's temperature at that ply, like `uniforms`; replaces the schedule.  Needs args["temperature"].
    gumbel_noise(game, ply) -> 218 floats: the Gumbel(0,1) draws of that game's root at that ply by root child, like `uniforms`; replaces
      the default above, with and without `learning`.
    holdout(game) -> bool: whether a game is a holdout game, like `uniforms`.  Default: a numpy Generator of its own, one draw per game in game
      order when the game starts, true with probability args["endings"]["holdout"].
    full_search(game, ply) -> bool: the full / fast decision, like `uniforms`.  Default: a numpy Generator of its own, drawn per ply for every
      running game in game order — never the global numpy or `random` state, whose draw order the callers above depend on.
    root_gamma(game, ply) -> 218 floats: the Gamma(alpha, 1) draws of args["root_dirichlet_alpha"] for that game's root at that ply, like
      `uniforms`.  Default: torch's generator, one draw per board slot and ply (the records then depend on the slot a game runs in)."""
    import random
    pcap = playout_cap_of(args)                             # validated before anything is created
    vt, quiet_fast = visit_target_options_of(args)
    forced_k = forced_playout_options_of(args)
    if forced_k is not None and not learning:
        raise ValueError("args['forced_playouts'] needs learning=True")
    end_opts = ending_options_of(args)
    gum = gumbel_options_of(args)
    gumbel_tree_of(args)
    if gumbel_noise is not None and gum is None:
        raise ValueError("gumbel_noise needs args['gumbel']")
    targets = search_targets_of(args)
    lcb_opts = lcb_options_of(args)
    temp_opts = temperature_options_of(args)
    if temperature is not None and temp_opts is None:
        raise ValueError("temperature needs args['temperature']")
    if holdout is not None and end_opts is None:
        raise ValueError("holdout needs args['endings']")
    if full_search is not None and pcap is None:
        raise ValueError("full_search needs args['playout_cap']")
    if root_gamma is not None and args.get("root_dirichlet_alpha") is None:
        raise ValueError("root_gamma needs args['root_dirichlet_alpha']")
    if not torch.cuda.is_available():
        raise RuntimeError("self-play needs an MI355X (HIP) device: the search has no CPU fallback")
    dev = model_device(model)                               # the model's own GPU (a rank with local_rank > 0 plays on ITS device)
    model = model.to(dev)
    if planes_dtype is None:
        if hasattr(model, "tower"):                       # FastPolicyNet: hand-written MFMA tower, NHWC planes
            planes_dtype = "bits128" if getattr(model, "w16", False) else "nhwc128"     # bit-packed: 1 KiB per board instead of 16
        else:
            planes_dtype = next(model.parameters()).dtype
            if planes_dtype not in (torch.float32, torch.bfloat16):
                planes_dtype = torch.float32
    if c960 and scharnagl is None:
        scharnagl = [random.randint(0, 959) for _ in range(n_games)]
    if not c960:
        scharnagl = [-1] * n_games
    cap = np.broadcast_to(np.asarray(max_plies, dtype=np.int64), (n_games,))
    B = max(1, min(int(n_games), int(n_boards) if n_boards else int(n_games)))
    S = int(args["num_searches"])
    eng = SelfPlayEngine(model, args, B, chess960=c960, learning=learning, planes_dtype=planes_dtype, device=dev)
    games = [dict(states=[], actions=[], rewards=[], colours=[], result=None, packed_states=[], sample_plies=[], chosen_actions=[], termination=None, holdout=False, would_end=None) for _ in range(n_games)]   # packed_states: the (119,8) uint8 form (train_RL.py:42)
    if targets is not None:
        for g_ in games:
            g_.update(search_values=[], surprises=[], value_targets=[])
    cap_rng = np.random.default_rng() if pcap is not None and full_search is None else None
    holdout_rng = np.random.default_rng() if end_opts is not None and holdout is None else None
    gumbel_rng = np.random.default_rng() if gum is not None and gumbel_noise is None and learning else None
    slot_holdout = np.zeros(B, dtype=np.uint8)            # the holdout flag of the game on each board slot
    slot_game = np.full(B, -1, dtype=np.int64)            # game running on each board slot, -1 = none
    plies = np.zeros(n_games, dtype=np.int64)             # plies played so far per game
    next_game = 0
    work = dict(sims=0, nn_rows=0, plies=0, full_plies=0, fast_plies=0, searches_without_network=0, forced_selections=0, pruned_visits=0,
                resigned=0, adjudicated_draws=0, adjudicated_proven=0, holdout_games=0, holdout_marks=0, gumbel_fallbacks=0)

    def refill(slots):
        """start the next waiting games on these slots (ChessTensor.__init__/start_board for each); the rest go dark"""
        nonlocal next_game
        sch, act = np.full(B, -1, dtype=np.int32), np.zeros(B, dtype=np.uint8)
        for s_ in slots:
            if next_game < n_games:
                slot_game[s_] = next_game
                sch[s_], act[s_] = scharnagl[next_game], 1
                if end_opts is not None:
                    slot_holdout[s_] = bool(holdout(next_game)) if holdout is not None else bool(holdout_rng.random() < end_opts["holdout"])
                    games[next_game]["holdout"] = bool(slot_holdout[s_])
                    work["holdout_games"] += int(slot_holdout[s_])
                next_game += 1
            else:
                slot_game[s_] = -1
                slot_holdout[s_] = 0
        if act.any():
            eng.new_games(sch, act)
            if end_opts is not None:
                eng.set_endings(end_opts, slot_holdout)    # the new games' holdout flags; streaks and marks of the games that go on stay
        eng.set_active((slot_game >= 0).astype(np.uint8))

    def absorb(rec, game_of_slot, sampled, ply_of_slot, improved=None, summary=None):
        """host-side bookkeeping of one ply's records (sim.py:71-73); runs while the GPU searches the next ply"""
        slots = np.nonzero((game_of_slot >= 0) & rec["active"].astype(bool))[0]
        for s_ in slots.tolist():                          # the move played, sample or not: chosen_actions has one action index per ply of the game
            if rec["chosen"][s_] >= 0:                     # -1: a rule ended the game instead of a move (args["endings"])
                games[int(game_of_slot[s_])]["chosen_actions"].append(int(rec["chosen"][s_]))
        for s_ in slots[~sampled[slots]].tolist():         # playout cap: a fast-search ply leaves no sample, only the game's outcome
            if rec["game_over"][s_]:
                games[int(game_of_slot[s_])]["result"] = {1: "1-0", -1: "0-1", 0: "1/2-1/2"}[int(rec["result"][s_])]
        slots = slots[sampled[slots]]
        if not len(slots):
            return
        states = torch.from_numpy(unpack_planes(rec["packed"][slots]))          # one unpack for the whole ply; a game's state is a view of it
        for i, s_ in enumerate(slots.tolist()):
            g = int(game_of_slot[s_])
            k = int(rec["n_child"][s_])
            white = bool(rec["colour"][s_])
            vis = rec["visits"][s_, :k].astype(np.int64)
            moves = _moves_for_record(rec["action"][s_, :k], white, rec["packed"][s_])
            games[g]["states"].append(states[i])
            games[g]["packed_states"].append(rec["packed"][s_])
            if improved is not None:                       # args["gumbel"]: the completed-Q improved policy, f32 values as Python floats
                games[g]["actions"].append(dict(zip(moves, improved[s_, :k].astype(np.float64).tolist())))
            else:
                games[g]["actions"].append(dict(zip(moves, (vis / int(vis.sum())).tolist())))      # int / int in float64: the reference's v / sum_values
            games[g]["colours"].append(white)
            games[g]["sample_plies"].append(int(ply_of_slot[s_]))
            if summary is not None:                        # args["search_targets"]: the search's own value and the policy surprise of this sample
                games[g]["search_values"].append(float(summary["best_q" if targets[1] == "best" else "root_q"][s_]))
                games[g]["surprises"].append(float(summary["surprise"][s_]))
            if rec["game_over"][s_]:
                games[g]["result"] = {1: "1-0", -1: "0-1", 0: "1/2-1/2"}[int(rec["result"][s_])]

    import time
    host = dict(compact=0.0, enqueue_search=0.0, absorb=0.0, wait_search=0.0, play_fetch=0.0, refill=0.0)     # host wall time per phase (stats["host_seconds"])
    def lap(key, t0):
        t1 = time.perf_counter()
        host[key] += t1 - t0
        return t1
    refill(range(B))
    pending = None
    while (slot_game >= 0).any():
        t0 = time.perf_counter()
        n_rows = eng.compact() if compact else B
        t0 = lap("compact", t0)
        running = np.nonzero(slot_game >= 0)[0]
        sampled = np.ones(B, dtype=bool)                   # boards whose ply becomes a training sample: all of them unless playout_cap
        if pcap is not None:
            for s_ in running[np.argsort(slot_game[running], kind="stable")]:      # decisions in game order
                g = int(slot_game[s_])
                sampled[s_] = bool(full_search(g, int(plies[g]))) if full_search is not None else bool(cap_rng.random() < pcap[1])
            if vt:
                eng.set_visit_targets(np.where(sampled, S, pcap[0]))
                if quiet_fast:
                    eng.set_quiet(~sampled)
            else:
                eng.set_budgets(np.where(sampled, S, pcap[0]))
            if forced_k is not None:
                eng.set_forced_playouts(forced_k, sampled)         # full-search plies only
        if root_gamma is not None:
            gam = np.zeros((B, 218), dtype=np.float32)
            for s_ in running:
                gam[s_] = np.asarray(root_gamma(int(slot_game[s_]), int(plies[slot_game[s_]])), dtype=np.float32)
            eng.next_gamma = torch.from_numpy(gam).to(dev)
        if gumbel_noise is not None or gumbel_rng is not None:
            gn = np.zeros((B, 218), dtype=np.float64)
            for s_ in running[np.argsort(slot_game[running], kind="stable")]:      # draws in game order
                g = int(slot_game[s_])
                gn[s_] = np.asarray(gumbel_noise(g, int(plies[g])), dtype=np.float64) if gumbel_noise is not None else -np.log(-np.log(gumbel_rng.random(218)))
            eng.set_gumbel(gum, gn)
        eng.search()                                       # enqueues num_searches x (network + tree step); returns before the GPU is done
        t0 = lap("enqueue_search", t0)
        if pending is not None:
            absorb(*pending)                               # previous ply's records, overlapped with this ply's search
            pending = None
        t0 = lap("absorb", t0)
        eng.check_errors()
        t0 = lap("wait_search", t0)
        u = np.zeros(B, dtype=np.float64)
        for s_ in running[np.argsort(slot_game[running], kind="stable")]:      # draws in game order
            g = int(slot_game[s_])
            u[s_] = uniforms(g, int(plies[g])) if uniforms is not None else np.random.random_sample()
        if temp_opts is not None:                          # each game's temperature from its own ply, not the slot's
            temps = np.zeros(B, dtype=np.float64)
            for s_ in running:
                g = int(slot_game[s_])
                temps[s_] = float(temperature(g, int(plies[g]))) if temperature is not None else temperature_at(temp_opts, int(plies[g]), full=bool(sampled[s_]))
            eng.set_temperatures(temps)
        eng.play(u)
        rec = eng.fetch_ply()
        ends = eng.fetch_endings() if end_opts is not None else None
        improved = eng.fetch_gumbel()["policy"] if gum is not None else None
        summary = eng.fetch_search_summary() if targets is not None else None
        if eng.stats()["boards_error"]:
            eng.check_errors()
        t0 = lap("play_fetch", t0)
        ply_of_slot = np.where(slot_game >= 0, plies[np.maximum(slot_game, 0)], -1)
        pending = (rec, slot_game.copy(), sampled, ply_of_slot, improved, summary)
        n_full = int(sampled[running].sum())
        if vt:                                             # the goals actually made: a kept root's visits count towards its target
            work["sims"] += int(eng.last_goals[running].sum()) if eng.last_goals is not None else 0
        else:
            work["sims"] += S * n_full + (pcap[0] if pcap is not None else 0) * (len(running) - n_full)
        work["nn_rows"] += eng.last_rows; work["plies"] += 1; work["searches_without_network"] += eng.last_steps == 0
        work["full_plies"] += n_full; work["fast_plies"] += len(running) - n_full
        plies[slot_game[running]] += 1
        done = [int(s_) for s_ in running if (rec["game_over"][s_] and rec["active"][s_]) or plies[slot_game[s_]] >= cap[slot_game[s_]]]
        for s_ in done:
            g = games[int(slot_game[s_])]
            over = bool(rec["game_over"][s_] and rec["active"][s_])
            g["termination"] = "max_plies" if not over else ("rules" if ends is None else ENDING_KINDS.get(int(ends["kind"][s_]), "rules"))
            if ends is not None and ends["would_ply"][s_] >= 0:
                g["would_end"] = {"kind": ENDING_KINDS[int(ends["would_kind"][s_])], "ply": int(ends["would_ply"][s_]), "colour": int(ends["would_colour"][s_])}
        if done:
            refill(done)
        lap("refill", t0)
        if verbose:
            print("ply %d: %d games running, %d waiting, %d network rows" % (work["plies"], int((slot_game >= 0).sum()), n_games - next_game, n_rows * eng.L))
    if pending is not None:
        absorb(*pending)
    for g in range(n_games):
        reward = {"1-0": 1, "0-1": -1}.get(games[g]["result"], 0)
        games[g]["rewards"] = [reward if ply % 2 == 0 else -reward for ply in games[g]["sample_plies"]]   # sim.py:94-97: the sign alternates with the ply the sample was taken at
        if targets is not None:                            # lc0's q_ratio blend in Python float64; every sampled ply played, so it has a value
            r_ = targets[0]
            games[g]["value_targets"] = [(1.0 - r_) * z + r_ * q for z, q in zip(games[g]["rewards"], games[g]["search_values"])]
    if forced_k is not None:
        work["forced_selections"], work["pruned_visits"] = eng.forced_stats()
    if end_opts is not None:
        work["resigned"], work["adjudicated_draws"], work["adjudicated_proven"], work["holdout_marks"] = eng.ending_stats()
    if gum is not None:
        work["gumbel_fallbacks"] = eng.gumbel_stats()[1]
    if temp_opts is not None:
        work["tempered_plays"], work["greedy_plays"], work["excluded_children"] = eng.temperature_stats()
    if lcb_opts is not None:
        work["lcb_decided"], work["lcb_differs"] = eng.lcb_stats()[:2]
    eng.close()
    if stats is not None:
        stats.update(work)
        stats["host_seconds"] = host
    return games


def ending_report(games):
    """What args["endings"] did to the games of play_games: the number of games each way of ending took, and over the holdout games that got a
    mark the false positives: a resign mark whose colour did not lose the game played out, a draw mark whose game ended decisively.  (A game
    cut at max_plies has no result: it counts as not lost and as not decisive.)"""
    r = dict(games=len(games), resigned=0, adjudicated_draws=0, adjudicated_proven=0, rules=0, max_plies=0, holdout_games=0, holdout_marks=0,
             resign_marks=0, resign_false_positives=0, draw_marks=0, draw_false_positives=0)
    key = {"resign": "resigned", "draw_adjudicated": "adjudicated_draws", "proven": "adjudicated_proven", "rules": "rules", "max_plies": "max_plies"}
    for g in games:
        r[key[g["termination"]]] += 1
        r["holdout_games"] += bool(g.get("holdout"))
        w = g.get("would_end")
        if w is None:
            continue
        r["holdout_marks"] += 1
        if w["kind"] == "resign":
            r["resign_marks"] += 1
            r["resign_false_positives"] += g["result"] != ("0-1" if w["colour"] else "1-0")
        elif w["kind"] == "draw_adjudicated":
            r["draw_marks"] += 1
            r["draw_false_positives"] += g["result"] in ("1-0", "0-1")
    return r


def play_game(model, args, c960=False):
    """One self-play game (sim.py:31-99): {'states','actions','rewards','colours'}."""
    g = play_games(model, args, 1, c960=c960)[0]
    return {k: g[k] for k in ("states", "actions", "rewards", "colours")}


def generate_training_data(model, num_games=1, args=None, return_dict=None, c960=False, rng_order="batched", n_boards=None):
    """sim.py:102-123: concatenated histories of num_games games; also stored under return_dict[os.getpid()].
    rng_order="batched" (default): all games run concurrently; python's `random` (Chess960 starts) and numpy's global RNG (move
      sampling) are consumed per ply across the running games, so the games differ from the ones the reference would draw from the
      same seeds (same distribution).
    rng_order="reference": one game after another, exactly the reference's order of RNG draws — same seeds, same games as
      sim.py:114-118 (bit for bit with a deterministic network); one board on the GPU, for checks rather than for throughput."""
    games_history = {"states": [], "actions": [], "rewards": [], "colours": []}
    if rng_order == "reference":
        games = [play_games(model, args, 1, c960=c960)[0] for _ in range(num_games)]
    elif rng_order == "batched":
        games = play_games(model, args, num_games, c960=c960, n_boards=n_boards)
    else:
        raise ValueError("rng_order must be 'batched' or 'reference'")
    for g in games:
        for key in games_history:
            games_history[key] += g[key]
    if return_dict is not None:
        return_dict[os.getpid()] = games_history
    return games_history
