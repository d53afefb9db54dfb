"""Batched self-play driver: B boards stepped in lock-step through the HIP engine with one batched
network call per simulation.  This is the GPU counterpart of sim.py:31-99 + mcts.py:39-122."""
import ctypes as C
import math

import numpy as np
import torch

from . import _native as N

NOISE_REFERENCE = float(np.float32(1.0) - np.float32(2.0 ** -24))     # degenerate Dirichlet draw, SURVEY §8(a) A19


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def model_device(model, default=None):
    """The CUDA device a network lives on (FastPolicyNet.device, or its first parameter's), else `default`, else the current device.
    Engines are created THERE: a rank with local_rank > 0 must not silently search on GPU 0."""
    dev = getattr(model, "device", None)
    if dev is None and hasattr(model, "parameters"):
        try:
            dev = next(iter(model.parameters())).device
        except (StopIteration, TypeError):
            dev = None
    if dev is not None and torch.device(dev).type == "cuda":
        dev = torch.device(dev)
        return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
    if default is not None:
        return torch.device(default)
    return torch.device("cuda", torch.cuda.current_device())


def search_segments(budgets, L=1, max_shrinks=4, num_searches=None):
    """Step counts of the segments a budgeted search is run in (SelfPlayEngine.search): after every segment but the last the network
    batch shrinks to the boards that still search (sz_compact_searching, one stream synchronisation each).

    budgets: simulations per board, or None (every board num_searches).  A board with budget s needs ceil(s / L) steps — exactly that many
    at L = 1, at least that many with leaf batching, where collisions end gathers early — so the candidate segment ends are the distinct
    values of ceil(s / L), and the last one, ceil(max / L), is the part of the search that runs without asking the device (with L > 1 the
    caller then steps until no board is pending).  At most max_shrinks interior ends are kept; when there are more candidates, the ones
    that minimise the network rows evaluated (segment length x boards searching during it), so nearby budget values share an end.
    Returns a list of positive step counts that sums to ceil(max / L); [] when nothing is to be searched."""
    L, max_shrinks = int(L), int(max_shrinks)
    if L < 1 or max_shrinks < 0:
        raise ValueError("search_segments: L must be >= 1 and max_shrinks >= 0")
    if budgets is None:
        total = -(-int(num_searches or 0) // L)
        return [total] if total > 0 else []
    b = np.asarray(budgets, dtype=np.int64).reshape(-1)
    if b.size and b.min() < 0:
        raise ValueError("search_segments: budgets must be >= 0")
    need = -(-b[b > 0] // L)                                     # steps each searching board needs
    if not need.size:
        return []
    ends, counts = np.unique(need, return_counts=True)          # candidate ends ascending, boards finishing at each
    k = len(ends)
    t = min(max_shrinks, k - 1)
    if t == k - 1:
        chosen = list(range(k))
    elif t == 0:
        chosen = [k - 1]
    else:
        alive = need.size - np.cumsum(counts)                   # boards still searching after candidate j
        ends_f = ends.astype(np.float64)
        best = ends_f * need.size                               # no interior end before candidate i
        back = []
        for _ in range(t):                                      # one more interior end per round
            cand = best[None, :] + (ends_f[:, None] - ends_f[None, :]) * alive[None, :]      # [i, j]: j the interior end before i
            cand[np.triu_indices(k)] = np.inf                   # j < i only
            back.append(np.argmin(cand, axis=1))
            best = cand.min(axis=1)
        chosen, i = [k - 1], k - 1
        for arg in reversed(back):
            i = int(arg[i])
            chosen.append(i)
        chosen.reverse()
    cuts = [0] + [int(ends[i]) for i in chosen]
    return [hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])]


def search_options_of(args):
    """The search options of args, checked: (leaves_per_step, virtual_loss, solver, combine_options).  All NON-REFERENCE, default off.

    args["leaves_per_step"] = L > 1 gathers up to L leaves per board per network call, steered apart by a virtual loss args["virtual_loss"]
    per descent in flight (sz_set_leaf_batching); board b's leaf i is network row slot(b)*L + i.
    args["solver"] = True carries proven results (forced wins, draws and losses) up the tree (sz_set_solver): descents end at proven nodes,
    refuted moves are not selected, play() takes the proving move of a won root.
    args["combine_options"] = True lets leaves_per_step > 1, solver and args["reuse_subtree"] run in one search, in any combination
    (sz_set_search_options); without it each pair is refused."""
    L, lam = args.get("leaves_per_step", 1), args.get("virtual_loss", 1.0)
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 1 <= L <= N.SZ_MAX_LEAVES_PER_STEP:
        raise ValueError("args['leaves_per_step'] must be an integer in 1..%d, got %r" % (N.SZ_MAX_LEAVES_PER_STEP, L))
    if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not (math.isfinite(lam) and lam >= 0):
        raise ValueError("args['virtual_loss'] must be a finite number >= 0, got %r" % (lam,))
    combine, solver, reuse = args.get("combine_options", False), args.get("solver", False), args.get("reuse_subtree", False)
    if not isinstance(combine, (bool, np.bool_)):
        raise ValueError("args['combine_options'] must be True or False, got %r" % (combine,))
    if L > 1 and reuse and not combine:
        raise ValueError("args['leaves_per_step'] > 1 and args['reuse_subtree'] exclude each other (without args['combine_options'])")
    if not isinstance(solver, (bool, np.bool_)):
        raise ValueError("args['solver'] must be True or False, got %r" % (solver,))
    if solver and reuse and not combine:
        raise ValueError("args['solver'] and args['reuse_subtree'] exclude each other (without args['combine_options'])")
    if solver and L > 1 and not combine:
        raise ValueError("args['solver'] and args['leaves_per_step'] > 1 exclude each other (without args['combine_options'])")
    return int(L), float(lam), bool(solver), bool(combine)


def visit_target_options_of(args):
    """The self-play configuration of subtree reuse, checked: (visit_targets, quiet_fast_plies).  NON-REFERENCE, default off.

    args["visit_targets"] = True lets args["reuse_subtree"] run together with args["playout_cap"] and args["root_dirichlet_alpha"], which are
    refused without it.  The engine then uses sz_set_visit_targets in place of sz_set_search_budgets (a board's number names its root's visit
    count at the END of the search; the visits a kept subtree already holds count towards it, so a cheap ply after a full one often needs no
    network call at all) and sz_set_search_root_noise in place of sz_set_root_noise (the root is noised at every search, kept roots included).
    Without args["playout_cap"] every board's target is num_searches.
    args["quiet_fast_plies"] = True (needs visit_targets, playout_cap and root_dirichlet_alpha): fast plies are searched without root noise
    (KataGo); their sampling temperature is args["temperature"]["fast"] (temperature_options_of).  The effect of either on playing strength
    is unmeasured."""
    vt, quiet = args.get("visit_targets", False), args.get("quiet_fast_plies", False)
    for key, val in (("visit_targets", vt), ("quiet_fast_plies", quiet)):
        if not isinstance(val, (bool, np.bool_)):
            raise ValueError("args[%r] must be True or False, got %r" % (key, val))
    if quiet and not (vt and args.get("playout_cap") is not None and args.get("root_dirichlet_alpha") is not None):
        raise ValueError("args['quiet_fast_plies'] needs args['visit_targets'], args['playout_cap'] and args['root_dirichlet_alpha']")
    return bool(vt), bool(quiet)


def forced_playout_options_of(args):
    """The forced-playout constant of args, checked: k, or None when the option is off.  NON-REFERENCE, default off.

    args["forced_playouts"] = k > 0 (KataGo uses 2) switches on forced playouts and policy-target pruning (sz_set_forced_playouts): at the root
    every child with n >= 1 visits is selected while n < sqrt(k * P * (N_root - 1)), whatever PUCT says, so a noised move gets enough visits
    to show what it is worth; play() then takes out of the recorded visit counts, and of the counts it samples from, the visits PUCT alone
    would not have made.  The tree keeps the counted visits.  Needs learning = True.  Its effect on playing strength is unmeasured."""
    k = args.get("forced_playouts")
    if k is None:
        return None
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, float, np.integer, np.floating)) or not (math.isfinite(k) and k > 0):      # NaN fails the comparison
        raise ValueError("args['forced_playouts'] must be a finite number > 0, got %r" % (k,))
    return float(k)


FPU_KEYS = ("mode", "value", "root_mode", "root_value")
FPU_MODES = {"reference": N.SZ_FPU_REFERENCE, "absolute": N.SZ_FPU_ABSOLUTE, "reduction": N.SZ_FPU_REDUCTION}


def fpu_options_of(args):
    """The first-play-urgency options of args, checked: (tree_mode, tree_value, root_mode, root_value) with the modes as SZ_FPU_* codes and
    the values rounded to f32, or None when the key is absent.  NON-REFERENCE, default off.

    args["fpu"] = {"mode": "reference" | "absolute" | "reduction", "value": x, "root_mode": ..., "root_value": ...} sets what selection takes a
    child without a visit to be worth (sz_set_fpu).  "reference": Node.get_ucb's 0.5, a dead draw.  "absolute": q0 = (x + 1) / 2, x in [-1, 1]
    a value from the mover's side.  "reduction": x in [0, 2] is taken off the parent's own value, scaled by the square root of the prior mass
    of the children already visited: v0 = vp - x * sqrt(mass), clamped to [-1, 1] (lc0, KataGo).  mode / value hold below the root, root_mode /
    root_value at the root of every search; each of the root's defaults to the tree's.  A "reference" site needs no value.  Checked in this
    order: the dict and its keys, mode, value, root_mode, root_value.  Its effect on playing strength is unmeasured."""
    opt = args.get("fpu")
    if opt is None:
        return None
    if not isinstance(opt, dict) or not set(opt) <= set(FPU_KEYS):
        raise ValueError("args['fpu'] must be a dict with keys from %s, got %r" % (FPU_KEYS, opt))
    if "mode" not in opt:
        raise ValueError("args['fpu'] needs 'mode'")
    sites = [("mode", "value", opt["mode"], opt.get("value")),
             ("root_mode", "root_value", opt.get("root_mode", opt["mode"]), opt.get("root_value", opt.get("value")))]
    out = []
    for mkey, vkey, mode, value in sites:
        if not isinstance(mode, str) or mode not in FPU_MODES:
            raise ValueError("args['fpu'][%r] must be one of 'reference', 'absolute', 'reduction', got %r" % (mkey, mode))
        if mode == "reference":
            out += [FPU_MODES[mode], 0.0]
            continue
        if value is None:
            raise ValueError("args['fpu'][%r] = %r needs %r" % (mkey, mode, vkey))
        lo, hi = (-1.0, 1.0) if mode == "absolute" else (0.0, 2.0)
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) or \
                not (math.isfinite(value) and lo <= float(np.float32(value)) <= hi):            # NaN fails the comparison
            raise ValueError("args['fpu'][%r] must be a number in [%g, %g] with %r, got %r" % (vkey, lo, hi, mode, value))
        out += [FPU_MODES[mode], float(np.float32(value))]
    return tuple(out)


CPUCT_KEYS = ("init", "base", "factor", "root_init", "root_base", "root_factor")
CPUCT_RANGES = {"init": (0.0, 100.0), "base": (1.0, 1e9), "factor": (0.0, 100.0)}


def cpuct_options_of(args):
    """The visit-dependent exploration rate of args, checked: (tree_init, tree_base, tree_factor, root_init, root_base, root_factor) rounded to
    f32, or None when the key is absent.  NON-REFERENCE, default off.

    args["cpuct"] = {"init": c, "base": 19652, "factor": 1, "root_init": ..., "root_base": ..., "root_factor": ...} replaces the constant C of
    selection by c(n_p) = init + factor * ln((n_p + base + 1) / base), n_p the parent's visit count (sz_set_cpuct): AlphaZero's schedule is
    {"init": 1.25}, lc0's CPuct / CPuctBase / CPuctFactor with its ...AtRoot triple map onto the six keys.  init / base / factor hold below
    the root, the root_ keys where a child of the root is selected and in policy-target pruning; each of the root's defaults to the tree's.
    init is required and lies in [0, 100], base in [1, 1e9], factor in [0, 100].  factor 0 is the constant init.  Refused with args["gumbel"].
    Checked in this order: the dict and its keys, init, base, factor, root_init, root_base, root_factor, the combinations.  Its effect on
    playing strength is unmeasured."""
    opt = args.get("cpuct")
    if opt is None:
        return None
    if not isinstance(opt, dict) or not set(opt) <= set(CPUCT_KEYS):
        raise ValueError("args['cpuct'] must be a dict with keys from %s, got %r" % (CPUCT_KEYS, opt))
    if "init" not in opt:
        raise ValueError("args['cpuct'] needs 'init'")
    tree = {"init": opt["init"], "base": opt.get("base", 19652.0), "factor": opt.get("factor", 1.0)}
    out = []
    for prefix in ("", "root_"):
        for key in ("init", "base", "factor"):
            x = opt.get(prefix + key, tree[key])
            lo, hi = CPUCT_RANGES[key]
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) or \
                    not (math.isfinite(x) and lo <= float(np.float32(x)) <= float(np.float32(hi))):     # NaN fails the comparison
                raise ValueError("args['cpuct'][%r] must be a number in [%g, %g], got %r" % (prefix + key, lo, hi, x))
            out.append(float(np.float32(x)))
    if args.get("gumbel") is not None:
        raise ValueError("args['cpuct'] and args['gumbel'] exclude each other: the Gumbel rule is a chain of its own, combining them is a follow-up")
    return tuple(out)


KLD_STOP_KEYS = ("min_gain", "interval", "min_simulations")


def kld_stop_options_of(args):
    """The KLD-gain early stopping options of args, checked: (min_gain, interval, min_simulations), or None when the key is absent.
    NON-REFERENCE, default off.

    args["kld_stop"] = {"min_gain": 5e-6, "interval": 100, "min_simulations": 0} (lc0's minimum-kldgain-per-node and kldgain-average-interval;
    the values are those of its training runs and the defaults here) lets a board's search stop before its goal (sz_set_kld_stop): whenever
    the root's children gained `interval` visits since the last snapshot, the Kullback-Leibler divergence of the snapshot's visit distribution
    from the one now, per new visit, is compared with min_gain, and below it the board makes no further simulation, provided it has made
    min_simulations.  Obvious recaptures and forced replies then cost a fraction of num_searches, sharp positions all of it.  min_gain lies in
    (0, 1], interval in 1..num_searches, min_simulations in 0..num_searches.  Budgets, visit targets and every other option work underneath;
    refused with args["gumbel"], whose sequential halving plans on the goal.  Checked in this order: the dict and its keys, min_gain, interval,
    min_simulations, the combinations.  Its effect on playing strength is unmeasured."""
    opt = args.get("kld_stop")
    if opt is None:
        return None
    if not isinstance(opt, dict) or not set(opt) <= set(KLD_STOP_KEYS):
        raise ValueError("args['kld_stop'] must be a dict with keys from %s, got %r" % (KLD_STOP_KEYS, opt))
    g = opt.get("min_gain", 5e-6)
    if isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, float, np.integer, np.floating)) or not (math.isfinite(g) and 0.0 < g <= 1.0):   # NaN fails the comparison
        raise ValueError("args['kld_stop']['min_gain'] must be a number in (0, 1], got %r" % (g,))
    S = int(args["num_searches"])
    out = [float(g)]
    for key, default, lo in (("interval", min(100, max(S, 1)), 1), ("min_simulations", 0, 0)):
        x = opt.get(key, default)
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not lo <= x <= S:
            raise ValueError("args['kld_stop'][%r] must be an integer in %d..num_searches = %d, got %r" % (key, lo, S, x))
        out.append(int(x))
    if args.get("gumbel") is not None:
        raise ValueError("args['kld_stop'] and args['gumbel'] exclude each other: sequential halving plans on the goal the stop would lower")
    return tuple(out)


SEARCH_TARGET_KEYS = ("q_ratio", "q_source", "surprise_fraction")
Q_SOURCES = ("root", "best")


def search_targets_of(args):
    """The training-target options of args, checked: (q_ratio, q_source, surprise_fraction), or None when the key is absent.  NON-REFERENCE,
    default off.

    args["search_targets"] = {"q_ratio": r, "q_source": "root" | "best", "surprise_fraction": f} switches the engine's search summary on
    (sz_set_search_summary) and tells play_games and train_rl what to do with it.  q_ratio in [0, 1] (default 0): a sample's value target
    becomes (1 - r) * z + r * q, z the game's result and q the search's own value of the position from the mover's side (lc0's q_ratio);
    q_source "root" (default) takes the mover's expected outcome over all of the root's visits, "best" over the most visited child's (the m of
    args["endings"]).  surprise_fraction in [0, 1] (default 0): the share of training effort handed out in proportion to each sample's policy
    surprise KL(target || prior) (KataGo's policy surprise weighting; train_rl.surprise_weights / resample_by_weight).  The key alone, with
    both at 0, records search_values and surprises and changes no target.  The surprise reads the priors the search used: a divergence >= 0
    where those sum to 1 (learning off, or args["root_dirichlet_alpha"]); under the reference's learning noise (0.75 p + 0.25 * a constant near 1
    on every child) they do not, the figure can be negative and surprise_weights counts it as 0: set root_dirichlet_alpha beside it.
    The search itself is untouched.  Refused with args["gumbel"], whose record is the improved policy and which exports v_mix itself.  Checked in this order: the dict and its keys, q_ratio, q_source,
    surprise_fraction, the combination.  Its effect on training is unmeasured."""
    opt = args.get("search_targets")
    if opt is None:
        return None
    if not isinstance(opt, dict) or not set(opt) <= set(SEARCH_TARGET_KEYS):
        raise ValueError("args['search_targets'] must be a dict with keys from %s, got %r" % (SEARCH_TARGET_KEYS, opt))
    def unit(key):
        x = opt.get(key, 0.0)
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) or not 0.0 <= x <= 1.0:       # NaN fails the comparison
            raise ValueError("args['search_targets'][%r] must be a number in [0, 1], got %r" % (key, x))
        return float(x)

    q_ratio = unit("q_ratio")
    src = opt.get("q_source", "root")
    if not isinstance(src, str) or src not in Q_SOURCES:
        raise ValueError("args['search_targets']['q_source'] must be one of %s, got %r" % (Q_SOURCES, src))
    fraction = unit("surprise_fraction")
    if args.get("gumbel") is not None:
        raise ValueError("args['search_targets'] and args['gumbel'] exclude each other: Gumbel's record is its improved policy and it exports v_mix itself")
    return q_ratio, src, fraction


LCB_KEYS = ("stdevs", "min_visit_prop", "select")


def lcb_options_of(args):
    """The lower-confidence-bound move selection of args, checked: (stdevs, min_visit_prop, select) with the two numbers as the f32 the engine
    holds, or None when the key is absent.  NON-REFERENCE, default off.

    args["lcb"] = {"stdevs": 5.0, "min_visit_prop": 0.15, "select": True} (the defaults, KataGo's lcbStdevs and minVisitPropForLCB) makes the
    tree keep the sum of the squares of the values backed up through every edge (sz_set_lcb) and, where play() would play the most visited
    move (a negative uniform, or T = 0 under args["temperature"]), play the move whose mean value is best after `stdevs` standard errors are
    taken off, among the root moves with at least two visits and at least `min_visit_prop` of the most visited move's.  A sampled play is
    chosen as without the key.  select False only observes: the moves are those without the key, fetch_lcb() / lcb_stats() still report
    what the rule would have played.  Refused with args["gumbel"], which chooses its own move, and with args["reuse_subtree"], whose kept
    subtree would have to carry the square sums along.  Checked in this order: the dict and its keys, stdevs, min_visit_prop, select, the
    combinations.  Its effect on playing strength is unmeasured."""
    opt = args.get("lcb")
    if opt is None:
        return None
    if not isinstance(opt, dict) or not set(opt) <= set(LCB_KEYS):
        raise ValueError("args['lcb'] must be a dict with keys from %s, got %r" % (LCB_KEYS, opt))
    number = lambda x: not isinstance(x, (bool, np.bool_)) and isinstance(x, (int, float, np.integer, np.floating))
    z = opt.get("stdevs", 5.0)
    if not number(z) or not (math.isfinite(z) and 0 <= z <= float(np.finfo(np.float32).max)):       # NaN fails the comparison; the struct holds an f32
        raise ValueError("args['lcb']['stdevs'] must be a finite number >= 0, got %r" % (z,))
    p = opt.get("min_visit_prop", 0.15)
    if not number(p) or not 0.0 <= p <= 1.0:
        raise ValueError("args['lcb']['min_visit_prop'] must be a number in [0, 1], got %r" % (p,))
    sel = opt.get("select", True)
    if not isinstance(sel, (bool, np.bool_)):
        raise ValueError("args['lcb']['select'] must be True or False, got %r" % (sel,))
    if args.get("gumbel") is not None:
        raise ValueError("args['lcb'] and args['gumbel'] exclude each other: the Gumbel search chooses its own move")
    if args.get("reuse_subtree", False):
        raise ValueError("args['lcb'] and args['reuse_subtree'] exclude each other: the kept subtree does not carry the square sums")
    return float(np.float32(z)), float(np.float32(p)), bool(sel)


GUMBEL_KEYS = ("m", "c_visit", "c_scale")


def gumbel_options_of(args):
    """The Gumbel root search options of args, checked: (m, c_visit, c_scale) with the constants rounded to f32, or None when the key is
    absent.  NON-REFERENCE, default off.

    args["gumbel"] = {"m": int, "c_visit": x, "c_scale": y} (defaults 16 / 50 / 1) switches the root of every search from PUCT with root noise
    to Gumbel AlphaZero's rule (sz_set_gumbel): m root moves are sampled without replacement by Gumbel-top-k, the simulations are spent on
    them by sequential halving, play() takes the best of the most visited moves, and the policy target is the completed-Q improved policy
    (fetch_gumbel) instead of the visit fractions.  Below the root nothing changes unless args["gumbel_tree"] says so (gumbel_tree_of).  Refused with a reuse_subtree engine, leaves_per_step > 1,
    the solver, forced playouts, endings and root_dirichlet_alpha: each combination is a follow-up.  Checked in this order: the dict and its
    keys, m, c_visit, c_scale, the combinations.  Its effect on playing strength is unmeasured."""
    opt = args.get("gumbel")
    if opt is None:
        return None
    if not isinstance(opt, dict) or not set(opt) <= set(GUMBEL_KEYS):
        raise ValueError("args['gumbel'] must be a dict with keys from %s, got %r" % (GUMBEL_KEYS, opt))
    m = opt.get("m", 16)
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or not 1 <= m <= N.SZ_MAX_MOVES:
        raise ValueError("args['gumbel']['m'] must be an integer in 1..%d, got %r" % (N.SZ_MAX_MOVES, m))
    out = [int(m)]
    for key, default in (("c_visit", 50.0), ("c_scale", 1.0)):
        x = opt.get(key, default)
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) or \
                not (math.isfinite(x) and math.isfinite(float(np.float32(x))) and x >= 0):          # NaN fails the comparison
            raise ValueError("args['gumbel'][%r] must be a finite number >= 0, got %r" % (key, x))
        out.append(float(np.float32(x)))
    for key, on in (("reuse_subtree", args.get("reuse_subtree", False)), ("leaves_per_step", args.get("leaves_per_step", 1) != 1),
                    ("solver", args.get("solver", False)), ("forced_playouts", args.get("forced_playouts") is not None),
                    ("endings", args.get("endings") is not None), ("root_dirichlet_alpha", args.get("root_dirichlet_alpha") is not None)):
        if on:
            raise ValueError("args['gumbel'] and args[%r] exclude each other" % key)
    return tuple(out)


def gumbel_tree_of(args):
    """args["gumbel_tree"], checked: True or False (absent: False).  NON-REFERENCE, default off.

    args["gumbel_tree"] = True, a key of its own beside args["gumbel"], switches the selection below the root of every Gumbel search from PUCT
    to the paper's deterministic completed-Q rule (sz_set_gumbel_tree): an inner node picks the child whose share of the visits lags furthest
    behind the completed-Q improved policy of that node.  Neither C nor args["fpu"] is consulted there then.  Needs args["gumbel"].  Its
    effect on playing strength is unmeasured."""
    on = args.get("gumbel_tree", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("args['gumbel_tree'] must be True or False, got %r" % (on,))
    if on and args.get("gumbel") is None:
        raise ValueError("args['gumbel_tree'] needs args['gumbel']: the rule is a part of the Gumbel search")
    return bool(on)


ENDING_KEYS =("resign_value", "resign_patience", "resign_min_ply", "draw_value", "draw_patience", "draw_min_ply", "proven", "holdout")
ENDING_KINDS = {N.SZ_END_RESIGN: "resign", N.SZ_END_DRAW: "draw_adjudicated", N.SZ_END_PROVEN: "proven"}


def ending_options_of(args):
    """The ending options of args, checked: a dict with every key of ENDING_KEYS, or None when the option is off.  NON-REFERENCE, default off.

    args["endings"] = {"resign_value": v, "resign_patience": n, "resign_min_ply": p, "draw_value": d, "draw_patience": n, "draw_min_ply": p,
    "proven": bool, "holdout": q} switches on resignation and adjudicated game endings (sz_set_endings): play() ends a game instead of a move
    when the mover's most visited move had an expected outcome m <= v in n of the mover's searches in a row (from ply p on), when |m| <= d in n
    searches in a row, or when the root is proven (needs args["solver"]).  Absent keys mean that rule is off (patience 0); a patience > 0 needs
    its value.  holdout in [0, 1]: the probability with which play_games plays a game out and only marks where a rule would have ended it
    (sim.ending_report counts how often the mark was wrong).  Its effect on playing strength is unmeasured."""
    opt = args.get("endings")
    if opt is None:
        return None
    if not isinstance(opt, dict) or not set(opt) <= set(ENDING_KEYS):
        raise ValueError("args['endings'] must be a dict with keys from %s, got %r" % (ENDING_KEYS, opt))
    number = lambda x: not isinstance(x, (bool, np.bool_)) and isinstance(x, (int, float, np.integer, np.floating))
    out = {}
    for rule, lo in (("resign", -1.0), ("draw", 0.0)):
        v, n, p = opt.get(rule + "_value"), opt.get(rule + "_patience", 0), opt.get(rule + "_min_ply", 0)
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 0 <= n <= 65535:
            raise ValueError("args['endings']['%s_patience'] must be an integer in 0..65535, got %r" % (rule, n))
        if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, np.integer)) or not 0 <= p <= 2 ** 31 - 1:
            raise ValueError("args['endings']['%s_min_ply'] must be an integer >= 0, got %r" % (rule, p))
        if v is None:
            if n > 0:
                raise ValueError("args['endings']['%s_patience'] = %d needs '%s_value'" % (rule, n, rule))
            v = 0.0
        if not number(v) or not (math.isfinite(v) and lo <= float(np.float32(v)) <= 1.0):       # NaN fails the comparison
            raise ValueError("args['endings']['%s_value'] must be a number in [%g, 1], got %r" % (rule, lo, v))
        out[rule + "_value"], out[rule + "_patience"], out[rule + "_min_ply"] = float(np.float32(v)), int(n), int(p)
    proven = opt.get("proven", False)
    if not isinstance(proven, (bool, np.bool_)):
        raise ValueError("args['endings']['proven'] must be True or False, got %r" % (proven,))
    if proven and not args.get("solver", False):
        raise ValueError("args['endings']['proven'] needs args['solver']: only the solver proves a root")
    h = opt.get("holdout", 0.0)
    if not number(h) or not 0.0 <= h <= 1.0:                     # NaN fails both comparisons
        raise ValueError("args['endings']['holdout'] must be a probability in [0, 1], got %r" % (h,))
    out["proven"], out["holdout"] = bool(proven), float(h)
    return out


TEMPERATURE_KEYS = ("t0", "t_final", "plies", "halflife", "fast", "visit_offset", "value_cutoff")


def temperature_options_of(args):
    """The move-selection temperature of args, checked: a dict with every key of TEMPERATURE_KEYS, or None when the key is absent.
    NON-REFERENCE, default off.

    args["temperature"] = {"t0": 1.0, "t_final": 0.0, "plies": 60, "halflife": None, "fast": None, "visit_offset": 0.0, "value_cutoff": None}
    (the defaults) switches play() from sampling the visit counts as they are, at every ply, to sampling child c with a probability
    proportional to (n_c + visit_offset) ** (1 / T) (sz_set_move_temperature), T from temperature_at(): t0 for the first `plies` plies of a
    game and t_final from then on, or with `halflife` a decay from t0 towards t_final that halves the distance every `halflife` plies after
    them.  T = 0 plays the most visited move.  fast: the temperature of args["playout_cap"]'s fast plies (KataGo: 0.0), whatever the ply.
    visit_offset (lc0's TempVisitOffset, usually negative) is added to every count, a child it leaves at or below 0 is not sampled;
    value_cutoff (lc0's TempValueCutoff) keeps moves out whose value lies more than that below the most visited move's.  The training
    record is not tempered.  Refused with args["gumbel"], which chooses its own move.  Checked in this order: the dict and its keys, t0,
    t_final, plies, halflife, fast, visit_offset, value_cutoff, the combinations.  Its effect on playing strength is unmeasured."""
    opt = args.get("temperature")
    if opt is None:
        return None
    if not isinstance(opt, dict) or not set(opt) <= set(TEMPERATURE_KEYS):
        raise ValueError("args['temperature'] must be a dict with keys from %s, got %r" % (TEMPERATURE_KEYS, opt))
    number = lambda x: not isinstance(x, (bool, np.bool_)) and isinstance(x, (int, float, np.integer, np.floating))
    out = {}
    for key, default in (("t0", 1.0), ("t_final", 0.0)):
        t = opt.get(key, default)
        if not number(t) or not (math.isfinite(t) and t >= 0):                   # NaN fails the comparison
            raise ValueError("args['temperature'][%r] must be a finite number >= 0, got %r" % (key, t))
        out[key] = float(t)
    n = opt.get("plies", 60)
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 0 <= n <= 2 ** 31 - 1:
        raise ValueError("args['temperature']['plies'] must be an integer >= 0, got %r" % (n,))
    out["plies"] = int(n)
    h = opt.get("halflife")
    if h is not None and (not number(h) or not (math.isfinite(h) and h > 0)):
        raise ValueError("args['temperature']['halflife'] must be None or a finite number > 0, got %r" % (h,))
    out["halflife"] = None if h is None else float(h)
    f = opt.get("fast")
    if f is not None and (not number(f) or not (math.isfinite(f) and f >= 0)):
        raise ValueError("args['temperature']['fast'] must be None or a finite number >= 0, got %r" % (f,))
    out["fast"] = None if f is None else float(f)
    v = opt.get("visit_offset", 0.0)
    if not number(v) or not (math.isfinite(v) and abs(v) <= float(np.finfo(np.float32).max)):       # the struct holds an f32
        raise ValueError("args['temperature']['visit_offset'] must be a finite number, got %r" % (v,))
    out["visit_offset"] = float(np.float32(v))
    c = opt.get("value_cutoff")
    if c is not None and (not number(c) or not (math.isfinite(c) and math.isfinite(float(np.float32(c))) and c >= 0)):
        raise ValueError("args['temperature']['value_cutoff'] must be None or a finite number >= 0, got %r" % (c,))
    out["value_cutoff"] = None if c is None else float(np.float32(c))
    if out["fast"] is not None and args.get("playout_cap") is None:
        raise ValueError("args['temperature']['fast'] needs args['playout_cap']: there are no fast plies without it")
    if args.get("gumbel") is not None:
        raise ValueError("args['temperature'] and args['gumbel'] exclude each other: the Gumbel search chooses its own move")
    return out


def temperature_at(opts, ply, full=True):
    """The schedule of args["temperature"]: the temperature of game ply `ply` (0 = the game's first move) under opts, a dict as
    temperature_options_of returns it.  full = False: a fast ply of args["playout_cap"], which takes opts["fast"] when that is set.  Pure,
    f64: t0 while ply < plies; then t_final, or with a halflife t_final + (t0 - t_final) * 0.5 ** ((ply - plies) / halflife)."""
    if not full and opts["fast"] is not None:
        return float(opts["fast"])
    t0, t_final, ply = float(opts["t0"]), float(opts["t_final"]), int(ply)
    if opts["halflife"] is None:
        return t0 if ply < opts["plies"] else t_final
    return t_final + (t0 - t_final) * 0.5 ** (max(0, ply - opts["plies"]) / float(opts["halflife"]))


def raise_if_overflowed(model):
    """ValueError when `model` keeps a range flag (FastPolicyNet / SplitPolicyNet: overflowed()) and a forward since the last look returned inf / NaN:
    with f16 operands a stored activation of 65520 or more is inf, the heads make NaN of it, and the search keeps a NaN prior without complaint.
    A model without overflowed() (a torch module, a bf16 network's always-False one) passes."""
    ov = getattr(model, "overflowed", None)
    if callable(ov) and ov():
        raise ValueError("%s(operands=%r): an activation left f16's range during the search (f16 holds at most 65504; from 65520 on a stored activation is inf) "
                         "and the network returned inf / NaN policies or values; the trees searched since the last check are not to be used "
                         "— use operands=\"bf16\" or SplitPolicyNet" % (type(model).__name__, getattr(model, "operands", None)))


class SelfPlayEngine:
    def __init__(self, model, args, n_boards, chess960=False, learning=True, device=None, planes_dtype=torch.float32,
                 noise_value=NOISE_REFERENCE, edges_per_board=0):
        if not torch.cuda.is_available():
            raise RuntimeError("SelfPlayEngine needs an MI355X (HIP) device: the search has no CPU fallback")
        self.device = torch.device(device) if device is not None else model_device(model)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.model = model
        self.args = dict(args)
        self.B = int(n_boards)
        self.S = int(args["num_searches"])
        self.chess960 = bool(chess960)
        self.planes_dtype = planes_dtype
        # NON-REFERENCE options (default off): leaf batching, the solver and their combinations, see search_options_of
        self.L, self.virtual_loss, self.solver, self.combine = search_options_of(self.args)
        self.last_steps = 0           # network calls made by the last search()
        self.last_rows = 0            # network rows evaluated by the last search()
        # NON-REFERENCE option (default off): per-board search budgets (set_budgets) with in-search batch shrinking; at most
        # args["max_shrinks"] shrinks per search on top of the one right after the roots were made (each costs a stream synchronisation)
        ms = self.args.get("max_shrinks", 4)
        if isinstance(ms, bool) or not isinstance(ms, (int, np.integer)) or ms < 0:
            raise ValueError("args['max_shrinks'] must be an integer >= 0, got %r" % (ms,))
        self.max_shrinks = int(ms)
        self.budgets = None           # host copy of the budgets in force (None: every board num_searches)
        # NON-REFERENCE option (default off): reuse_subtree as a self-play configuration, see visit_target_options_of
        self.visit_targets, self.quiet_fast_plies = visit_target_options_of(self.args)
        self.targets = None           # host copy of the visit targets in force (set_visit_targets)
        # NON-REFERENCE option (default off): forced playouts and policy-target pruning, see forced_playout_options_of
        self.forced_k = forced_playout_options_of(self.args)
        if self.forced_k is not None and not learning:
            raise ValueError("args['forced_playouts'] needs learning=True: it is an exploration option of self-play, like root noise")
        # NON-REFERENCE option (default off): first-play urgency for unvisited children, see fpu_options_of
        self.fpu = fpu_options_of(self.args)
        # NON-REFERENCE option (default off): AlphaZero's visit-dependent exploration rate in C's place, see cpuct_options_of
        self.cpuct = cpuct_options_of(self.args)
        # NON-REFERENCE option (default off): KLD-gain early stopping of a board's search, see kld_stop_options_of
        self.kld_stop = kld_stop_options_of(self.args)
        # NON-REFERENCE option (default off): the search summary and what training does with it, see search_targets_of
        self.search_targets = search_targets_of(self.args)
        self.search_summary = False   # sz_set_search_summary is on (set_search_summary)
        # NON-REFERENCE option (default off): per-edge value spread and lower-confidence-bound move selection, see lcb_options_of
        self.lcb = lcb_options_of(self.args)
        # NON-REFERENCE option (default off): Gumbel root search with sequential halving and the completed-Q policy target, see gumbel_options_of
        self.gumbel = gumbel_options_of(self.args)
        self._gumbel_g = None         # the device copy of the Gumbel draws in force (set_gumbel)
        # NON-REFERENCE option (default off): completed-Q selection below the root of a Gumbel search, see gumbel_tree_of
        self.gumbel_tree = gumbel_tree_of(self.args)
        # NON-REFERENCE option (default off): resignation and adjudicated game endings, see ending_options_of
        self.endings = ending_options_of(self.args)
        # NON-REFERENCE option (default off): move-selection temperature, visit offset and value cutoff, see temperature_options_of
        self.temperature = temperature_options_of(self.args)
        self._temps = None            # the device array [B] f64 sz_play reads its temperatures from (set_move_temperature)
        self.quiet = None             # boards whose next searches get no root noise (set_quiet; visit_targets mode)
        self.last_goals = None        # visit_targets mode: search_goals() of the last search()
        self._compact_on = False      # the mapping chosen by the last compact() call
        self._restore = False         # a search shrank the batch: the caller's mapping is put back before the next search begins
        # planes_dtype: torch.float32 / torch.bfloat16 -> [B,119,8,8] NCHW (reference layout);
        #               "nhwc128" -> [B,64,128] bf16 position-major for FastPolicyNet (csrc/sz_nn.hip)
        #               "bits128" -> the same image bit-packed, [B,1024] uint8 (1 KiB per board), expanded by the stem kernel
        self.nhwc = planes_dtype == "nhwc128"
        self.bits = planes_dtype == "bits128"
        code = N.SZ_PLANES_NHWC128_BITS if self.bits else N.SZ_PLANES_NHWC128_BF16 if self.nhwc else (N.SZ_PLANES_BF16 if planes_dtype == torch.bfloat16 else N.SZ_PLANES_F32)
        cfg = N.sz_config(self.B, self.S, float(args["C"]), int(bool(learning)), float(noise_value), int(self.chess960),
                          int(edges_per_board), code, self.device.index or 0, int(bool(self.args.get("reuse_subtree", False))))
        self._e = C.c_void_p()
        N.check(N.lib().sz_create(C.byref(cfg), C.byref(self._e)), "sz_create")
        dev = self.device
        rows = self.B * self.L        # network rows
        if self.bits:
            self.planes = torch.zeros(rows, 1024, dtype=torch.uint8, device=dev)
        elif self.nhwc:
            self.planes = torch.zeros(rows, 64, 128, dtype=torch.bfloat16, device=dev)
        else:
            self.planes = torch.zeros(rows, N.SZ_PLANES, 8, 8, dtype=planes_dtype, device=dev)
        if self.combine:
            self.set_search_options(self.L, self.virtual_loss, self.solver)
        else:
            if self.L > 1:
                N.check(N.lib().sz_set_leaf_batching(self._e, self.L, self.virtual_loss, self._stream()), "sz_set_leaf_batching")
            if self.solver:
                N.check(N.lib().sz_set_solver(self._e, 1, self._stream()), "sz_set_solver")
        self.uniforms = torch.zeros(self.B, dtype=torch.float64, device=dev)
        self._moves = None            # play_moves' device buffer [B] int32, allocated on first use
        self.root_action = torch.zeros(self.B, N.SZ_MAX_MOVES, dtype=torch.int32, device=dev)
        self.root_visits = torch.zeros(self.B, N.SZ_MAX_MOVES, dtype=torch.int32, device=dev)
        self.root_nchild = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.root_prior = torch.zeros(self.B, N.SZ_MAX_MOVES, dtype=torch.float32, device=dev)
        self.root_wsum = torch.zeros(self.B, N.SZ_MAX_MOVES, dtype=torch.float64, device=dev)
        self.nn_seconds = 0.0
        self.n_rows = self.B          # rows of the network batch in use (sz_compact: live boards only)
        # NON-REFERENCE option (default off): args["root_dirichlet_alpha"] = alpha switches from the reference's noise (the constant
        # 1-2^-24 at every expansion, mcts.py:91-98) to AlphaZero's Dirichlet(alpha) noise on the root's children only
        self.root_alpha = self.args.get("root_dirichlet_alpha")
        if self.root_alpha is not None and self.args.get("reuse_subtree", False) and not self.visit_targets:
            raise ValueError("args['root_dirichlet_alpha'] and args['reuse_subtree'] exclude each other: a reused root was expanded as an inner node "
                             "(un-noised priors) and is never expanded again, so the root noise would reach the first ply of a game only")
        self._gamma = None
        self.next_gamma = None        # [B, SZ_MAX_MOVES] draws for the next begin() in place of torch's generator (play_games' root_gamma)
        if self.visit_targets:        # every board's target is num_searches until set_visit_targets says otherwise
            self.set_visit_targets(np.full(self.B, self.S, np.int32))
        if self.forced_k is not None:  # every board is forced until set_forced_playouts says otherwise
            self.set_forced_playouts(self.forced_k)
        if self.fpu is not None:
            self.set_fpu(self.fpu)
        if self.cpuct is not None:
            self.set_cpuct(self.cpuct)
        if self.kld_stop is not None:
            self.set_kld_stop(self.kld_stop)
        if self.search_targets is not None:
            self.set_search_summary(True)
        if self.lcb is not None:
            self.set_lcb(self.lcb)
        if self.gumbel is not None:    # g = None (a deterministic search) until set_gumbel hands over draws
            self.set_gumbel(self.gumbel)
        if self.gumbel_tree:
            self.set_gumbel_tree(True)
        if self.endings is not None:  # no holdout board until set_endings says otherwise
            self.set_endings(self.endings)
        if self.temperature is not None:  # every board at t0 until set_temperatures says otherwise
            self.set_move_temperature(self.temperature, np.full(self.B, self.temperature["t0"], np.float64))

    def close(self):
        if self._e:
            N.lib().sz_destroy(self._e)
            self._e = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def new_games(self, scharnagl=None, active=None):
        sch = None if scharnagl is None else np.ascontiguousarray(scharnagl, dtype=np.int32)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        N.check(N.lib().sz_new_games(self._e, None if sch is None else sch.ctypes.data_as(C.c_void_p),
                                     None if act is None else act.ctypes.data_as(C.c_void_p), self._stream()), "sz_new_games")

    def upload_game(self, board, chess_tensor):
        ring, ply, _ = chess_tensor.export_ring()
        N.check(N.lib().sz_upload_game(self._e, int(board), ring, int(ply), self._stream()), "sz_upload_game")

    def set_active(self, active):
        act = np.ascontiguousarray(active, dtype=np.uint8)
        N.check(N.lib().sz_set_active(self._e, act.ctypes.data_as(C.c_void_p), self._stream()), "sz_set_active")

    def compact(self, enable=True):
        """Number the boards that will search next 0..n_live-1 (sz_compact): the network then runs on planes[:n_live] only.
        Call between searches after play() / new_games() / set_active() changed the live set.  Returns n_live."""
        n = C.c_int32()
        N.check(N.lib().sz_compact(self._e, int(bool(enable)), C.byref(n), self._stream()), "sz_compact")
        self.n_rows = int(n.value) if enable else self.B
        self._compact_on, self._restore = bool(enable), False
        return self.n_rows

    def set_search_options(self, leaves_per_step, virtual_loss, solver):
        """leaves_per_step / virtual_loss and the solver in one call, any combination, with and without reuse_subtree (sz_set_search_options);
        between searches only.  On a reuse_subtree engine a change of leaves_per_step or of the solver drops every kept subtree.  The planes
        buffer grows with leaves_per_step (network rows = boards * leaves_per_step)."""
        opt = N.sz_search_options(int(leaves_per_step), float(virtual_loss), int(bool(solver)))
        N.check(N.lib().sz_set_search_options(self._e, C.byref(opt), self._stream()), "sz_set_search_options")
        self.L, self.virtual_loss, self.solver = int(leaves_per_step), float(virtual_loss), bool(solver)
        if self.planes.shape[0] < self.B * self.L:
            self.planes = torch.zeros((self.B * self.L,) + tuple(self.planes.shape[1:]), dtype=self.planes.dtype, device=self.device)

    def set_budgets(self, budgets):
        """Per-board search budgets (sz_set_search_budgets, a NON-REFERENCE option): budgets[b] in 0..num_searches simulations for board b
        from the next search on, until changed; None = every board num_searches again.  A board searched with budget s has, bit for bit,
        the tree it has in an engine created with num_searches = s."""
        if budgets is None:
            N.check(N.lib().sz_set_search_budgets(self._e, None, self._stream()), "sz_set_search_budgets")
            self.budgets = None
            return
        b = np.ascontiguousarray(budgets, dtype=np.int32).reshape(-1)
        if b.shape[0] != self.B:
            raise ValueError("set_budgets: %d budgets for %d boards" % (b.shape[0], self.B))
        N.check(N.lib().sz_set_search_budgets(self._e, b.ctypes.data_as(C.POINTER(C.c_int32)), self._stream()), "sz_set_search_budgets")
        self.budgets = b.copy()

    def set_visit_targets(self, targets):
        """Per-board root visit targets (sz_set_visit_targets, a NON-REFERENCE option): board b's next searches end with root visit count
        max(N_kept, 1 + targets[b]); on a fresh root that is a budget of targets[b], a kept root's visits count towards it.  None = off.
        Targets and budgets exclude each other: the later call wins."""
        if targets is None:
            N.check(N.lib().sz_set_visit_targets(self._e, None, self._stream()), "sz_set_visit_targets")
            self.targets = None
            return
        t = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
        if t.shape[0] != self.B:
            raise ValueError("set_visit_targets: %d targets for %d boards" % (t.shape[0], self.B))
        N.check(N.lib().sz_set_visit_targets(self._e, t.ctypes.data_as(C.POINTER(C.c_int32)), self._stream()), "sz_set_visit_targets")
        self.targets, self.budgets = t.copy(), None

    def search_goals(self):
        """after begin(): the new simulations each board's search makes (sz_search_goals; synchronises the stream) -> int32 [B]"""
        g = np.zeros(self.B, np.int32)
        N.check(N.lib().sz_search_goals(self._e, g.ctypes.data_as(C.POINTER(C.c_int32)), self._stream()), "sz_search_goals")
        return g

    def set_search_root_noise(self, gamma, quiet=None):
        """set_root_noise for every search's root, continued searches on a kept subtree included (sz_set_search_root_noise).  quiet: per board,
        != 0 = no root noise for that board in the searches that follow; None = no board is quiet.  On a reuse_subtree engine switching
        between None and a tensor drops every kept subtree."""
        self._gamma = None if gamma is None else gamma.to(self.device, torch.float32).contiguous()
        q = None if quiet is None else np.ascontiguousarray(quiet, dtype=np.uint8).reshape(-1)
        if q is not None and q.shape[0] != self.B:
            raise ValueError("set_search_root_noise: %d quiet flags for %d boards" % (q.shape[0], self.B))
        N.check(N.lib().sz_set_search_root_noise(self._e, _ptr(self._gamma), None if q is None else q.ctypes.data_as(C.c_void_p), self._stream()),
                "sz_set_search_root_noise")

    def set_forced_playouts(self, k, boards=None):
        """Forced playouts and policy-target pruning (sz_set_forced_playouts, a NON-REFERENCE option) from the next begin() on, until changed:
        k > 0 for the boards with boards[b] != 0 (None: all of them), k = 0 switches the option off.  Between searches only; kept subtrees
        are not dropped."""
        m = None if boards is None else np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1)
        if m is not None and m.shape[0] != self.B:
            raise ValueError("set_forced_playouts: %d flags for %d boards" % (m.shape[0], self.B))
        N.check(N.lib().sz_set_forced_playouts(self._e, float(k), None if m is None else m.ctypes.data_as(C.c_void_p), self._stream()), "sz_set_forced_playouts")
        self.forced_k = float(k) if k else None

    def forced_stats(self):
        """(root selections decided by a forced child, visits pruning took out of the records), all boards, cumulative (sz_forced_stats)"""
        out = (C.c_uint64 * 2)()
        N.check(N.lib().sz_forced_stats(self._e, out, self._stream()), "sz_forced_stats")
        return int(out[0]), int(out[1])

    def set_fpu(self, opts):
        """First-play urgency (sz_set_fpu, a NON-REFERENCE option) from the next begin() on, until changed.  opts: (tree_mode, tree_value,
        root_mode, root_value) as fpu_options_of returns it (SZ_FPU_* codes), or None = off.  Between searches only; kept subtrees are not
        dropped."""
        o = None if opts is None else N.sz_fpu_options(int(opts[0]), float(opts[1]), int(opts[2]), float(opts[3]))
        N.check(N.lib().sz_set_fpu(self._e, None if o is None else C.byref(o), self._stream()), "sz_set_fpu")
        self.fpu = None if opts is None else tuple(opts)

    def set_cpuct(self, opts):
        """The visit-dependent exploration rate (sz_set_cpuct, a NON-REFERENCE option) from the next begin() on, until changed.  opts: (tree_init,
        tree_base, tree_factor, root_init, root_base, root_factor) as cpuct_options_of returns it, or None = off (args["C"] again).  Between
        searches only; kept subtrees are not dropped; refused while the Gumbel search is on."""
        o = None if opts is None else N.sz_cpuct_options(*[float(x) for x in opts])
        N.check(N.lib().sz_set_cpuct(self._e, None if o is None else C.byref(o), self._stream()), "sz_set_cpuct")
        self.cpuct = None if opts is None else tuple(float(x) for x in opts)

    def set_kld_stop(self, opts):
        """KLD-gain early stopping (sz_set_kld_stop, a NON-REFERENCE option) from the next begin() on, until changed.  opts: (min_gain, interval,
        min_simulations) as kld_stop_options_of returns it, or None = off.  Between searches only; kept subtrees are not touched; refused
        while the Gumbel search is on."""
        o = None if opts is None else N.sz_kld_stop_options(float(opts[0]), int(opts[1]), int(opts[2]))
        N.check(N.lib().sz_set_kld_stop(self._e, None if o is None else C.byref(o), self._stream()), "sz_set_kld_stop")
        self.kld_stop = None if opts is None else (float(opts[0]), int(opts[1]), int(opts[2]))

    def check_stop(self):
        """One check of every searching board against the stopping rule (sz_search_check_stop: one launch, no synchronisation); a no-op
        while the option is off.  A stopped board takes the leaves it has in flight through one more step() and is done."""
        N.check(N.lib().sz_search_check_stop(self._e, self._stream()), "sz_search_check_stop")

    def fetch_kld_stop(self):
        """sz_fetch_kld_stop: dict of [B] arrays of each board's last search: stopped_at (the simulations it was stopped at, -1: not stopped),
        checks (checks that formed a gain) and last_gain (the last of them, per new visit; NaN: none)"""
        out = dict(stopped_at=np.zeros(self.B, np.int32), checks=np.zeros(self.B, np.int32), last_gain=np.zeros(self.B, np.float64))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_fetch_kld_stop(self._e, p(out["stopped_at"]), p(out["checks"]), p(out["last_gain"]), self._stream()), "sz_fetch_kld_stop")
        return out

    def kld_stop_stats(self):
        """(boards stopped early, checks evaluated, simulations not made), all boards, cumulative (sz_kld_stop_stats)"""
        out = (C.c_uint64 * 3)()
        N.check(N.lib().sz_kld_stop_stats(self._e, out, self._stream()), "sz_kld_stop_stats")
        return tuple(int(x) for x in out)

    def set_search_summary(self, on):
        """The search summary (sz_set_search_summary, a NON-REFERENCE option) from the next play() on, until changed: every play() also records
        each playing board's root_q, best_q and policy surprise.  Between searches only; no tree is touched; refused while the Gumbel search
        is on."""
        N.check(N.lib().sz_set_search_summary(self._e, int(bool(on)), self._stream()), "sz_set_search_summary")
        self.search_summary = bool(on)

    def fetch_search_summary(self):
        """sz_fetch_search_summary: dict of [B] arrays of the last play() made with the summary on: root_q (the mover's expected outcome over
        all of the root's visits), best_q (over the most visited child's), surprise (KL(record's visit fractions || the priors the search
        used)) and valid (0: the board did not play, the three are NaN)"""
        B = self.B
        out = dict(root_q=np.zeros(B, np.float64), best_q=np.zeros(B, np.float64), surprise=np.zeros(B, np.float64), valid=np.zeros(B, np.uint8))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_fetch_search_summary(self._e, p(out["root_q"]), p(out["best_q"]), p(out["surprise"]), p(out["valid"]), self._stream()),
                "sz_fetch_search_summary")
        return out

    def search_summary_stats(self):
        """(summaries made, surprise terms dropped because the stored prior was no normal positive f32), all boards, cumulative
        (sz_search_summary_stats)"""
        out = (C.c_uint64 * 2)()
        N.check(N.lib().sz_search_summary_stats(self._e, out, self._stream()), "sz_search_summary_stats")
        return int(out[0]), int(out[1])

    def set_lcb(self, opts):
        """Per-edge value spread and LCB move selection (sz_set_lcb, a NON-REFERENCE option) from the next begin() on, until changed.  opts:
        (stdevs, min_visit_prop, select) as lcb_options_of returns it, or None = off.  Between searches only; refused on a reuse_subtree
        engine and while the Gumbel search is on."""
        if opts is None:
            N.check(N.lib().sz_set_lcb(self._e, None, self._stream()), "sz_set_lcb")
            self.lcb = None
            return
        z, p, sel = opts
        o = N.sz_lcb_options(float(z), float(p), int(bool(sel)))
        N.check(N.lib().sz_set_lcb(self._e, C.byref(o), self._stream()), "sz_set_lcb")
        self.lcb = (float(np.float32(z)), float(np.float32(p)), bool(sel))

    def fetch_lcb(self):
        """sz_fetch_lcb after play(): dict of [B] arrays: move (the rule's move as a root-child index), cstar (the most visited child),
        lcb_move / lcb_cstar (their bounds, NaN where the child has fewer than two visits), n_candidates, decided (1: the rule decided the
        move played).  -1, -1, NaN, NaN, 0, 0 for a board that made no choice."""
        B = self.B
        out = dict(move=np.zeros(B, np.int32), cstar=np.zeros(B, np.int32), lcb_move=np.zeros(B, np.float64), lcb_cstar=np.zeros(B, np.float64),
                   n_candidates=np.zeros(B, np.int32), decided=np.zeros(B, np.uint8))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_fetch_lcb(self._e, p(out["move"]), p(out["cstar"]), p(out["lcb_move"]), p(out["lcb_cstar"]), p(out["n_candidates"]),
                                     p(out["decided"]), self._stream()), "sz_fetch_lcb")
        return out

    def lcb_stats(self):
        """(plays the rule decided, plays at which its move differs from the most visited one, ssqrt arguments treated as 0), all boards,
        cumulative (sz_lcb_stats)"""
        out = (C.c_uint64 * 3)()
        N.check(N.lib().sz_lcb_stats(self._e, out, self._stream()), "sz_lcb_stats")
        return tuple(int(x) for x in out)

    def root_value_spread(self):
        """The root children's sums of squared backed-up values [B, SZ_MAX_MOVES] f64 in root_children()'s order (sz_root_value_spread); the
        search begun last must have run under set_lcb"""
        q = torch.zeros(self.B, N.SZ_MAX_MOVES, dtype=torch.float64, device=self.device)
        N.check(N.lib().sz_root_value_spread(self._e, _ptr(q), self._stream()), "sz_root_value_spread")
        torch.cuda.synchronize(self.device)
        return q.cpu().numpy()

    def debug_tree_spread(self, board):
        """the sum of squared backed-up values of every edge of one board's tree (f64), rows in debug_tree()'s order (sz_debug_tree_spread; a
        search under set_lcb only)"""
        n = C.c_int32()
        N.check(N.lib().sz_debug_tree_spread(self._e, int(board), 0, None, C.byref(n), self._stream()), "sz_debug_tree_spread")
        q = np.zeros(n.value, np.float64)
        N.check(N.lib().sz_debug_tree_spread(self._e, int(board), n.value, q.ctypes.data_as(C.c_void_p), C.byref(n), self._stream()), "sz_debug_tree_spread")
        return q

    def set_gumbel(self, opts, g=None):
        """Gumbel root search (sz_set_gumbel, a NON-REFERENCE option) from the next begin() on, until changed.  opts: (m, c_visit, c_scale) as
        gumbel_options_of returns it, or None = off.  g: [B, SZ_MAX_MOVES] Gumbel(0,1) draws by root child (a float64 tensor or array; the
        engine keeps its device copy alive and unchanged until the next call), None = all zeros, a deterministic search.  Between searches
        only; a refused call changes nothing."""
        o = None if opts is None else N.sz_gumbel_options(int(opts[0]), float(opts[1]), float(opts[2]))
        gd = None
        if o is not None and g is not None:
            gd = torch.as_tensor(np.asarray(g, dtype=np.float64) if not torch.is_tensor(g) else g).to(self.device, torch.float64).contiguous()
            if tuple(gd.shape) != (self.B, N.SZ_MAX_MOVES):
                raise ValueError("set_gumbel: g must be [%d, %d], got %r" % (self.B, N.SZ_MAX_MOVES, tuple(gd.shape)))
        N.check(N.lib().sz_set_gumbel(self._e, None if o is None else C.byref(o), _ptr(gd), self._stream()), "sz_set_gumbel")
        # the search that ended last still reads its own draws in play(): the previous copy stays alive for one more call
        self.gumbel, self._gumbel_g, self._gumbel_g_prev = (None if opts is None else tuple(opts)), gd, self._gumbel_g
        if opts is None:
            self.gumbel_tree = False  # sz_set_gumbel(NULL) clears sz_set_gumbel_tree's flag

    def set_gumbel_tree(self, on):
        """Completed-Q selection below the root of a Gumbel search (sz_set_gumbel_tree, a NON-REFERENCE option) from the next begin() on, until
        changed or until set_gumbel(None).  Between searches only; switching it on needs Gumbel on; a refused call changes nothing."""
        N.check(N.lib().sz_set_gumbel_tree(self._e, int(bool(on)), self._stream()), "sz_set_gumbel_tree")
        self.gumbel_tree = bool(on)

    def gumbel_tree_stats(self):
        """selections below the root made by the completed-Q rule, all boards, cumulative (sz_gumbel_tree_stats)"""
        out = (C.c_uint64 * 1)()
        N.check(N.lib().sz_gumbel_tree_stats(self._e, out, self._stream()), "sz_gumbel_tree_stats")
        return int(out[0])

    def fetch_gumbel(self):
        """sz_fetch_gumbel after play(): dict of policy [B, SZ_MAX_MOVES] f32 (the improved policy by root child, in fetch_ply()'s action
        order), v_mix [B] f64 and root_value [B] f32; rows are valid where fetch_ply()'s active is 1"""
        B = self.B
        out = dict(policy=np.zeros((B, N.SZ_MAX_MOVES), np.float32), v_mix=np.zeros(B, np.float64), root_value=np.zeros(B, np.float32))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_fetch_gumbel(self._e, p(out["policy"]), p(out["v_mix"]), p(out["root_value"]), self._stream()), "sz_fetch_gumbel")
        return out

    def gumbel_stats(self):
        """(root selections made by the Gumbel rule, those of them that found no child at the level), all boards, cumulative (sz_gumbel_stats)"""
        out = (C.c_uint64 * 2)()
        N.check(N.lib().sz_gumbel_stats(self._e, out, self._stream()), "sz_gumbel_stats")
        return int(out[0]), int(out[1])

    def set_endings(self, opts, holdout=None):
        """Resignation and adjudicated game endings (sz_set_endings, a NON-REFERENCE option) from the next play() on, until changed.  opts: a
        dict with keys of ENDING_KEYS (absent: that rule off; 'holdout' is play_games' business and ignored here), or None = off.  holdout:
        the boards [B] that play on and only mark where a rule would have ended them (None: none).  Between searches only; kept subtrees,
        streaks and marks are not touched."""
        h = None if holdout is None else np.ascontiguousarray(holdout, dtype=np.uint8).reshape(-1)
        if h is not None and h.shape[0] != self.B:
            raise ValueError("set_endings: %d flags for %d boards" % (h.shape[0], self.B))
        o = None
        if opts is not None:
            o = N.sz_ending_options(float(opts.get("resign_value", 0.0)), int(opts.get("resign_patience", 0)), int(opts.get("resign_min_ply", 0)),
                                    float(opts.get("draw_value", 0.0)), int(opts.get("draw_patience", 0)), int(opts.get("draw_min_ply", 0)),
                                    int(bool(opts.get("proven", False))))
        N.check(N.lib().sz_set_endings(self._e, None if o is None else C.byref(o), None if h is None else h.ctypes.data_as(C.c_void_p), self._stream()),
                "sz_set_endings")
        self.endings = None if opts is None else dict(opts)

    def fetch_endings(self):
        """sz_fetch_endings: dict of [B] arrays: kind (SZ_END_*) and mover_value (m) of the last play(), and the boards' sticky holdout marks
        would_ply (-1: none), would_kind, would_colour"""
        B = self.B
        out = dict(kind=np.zeros(B, np.uint8), mover_value=np.zeros(B, np.float64), would_ply=np.zeros(B, np.int32),
                   would_kind=np.zeros(B, np.uint8), would_colour=np.zeros(B, np.uint8))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_fetch_endings(self._e, p(out["kind"]), p(out["mover_value"]), p(out["would_ply"]), p(out["would_kind"]), p(out["would_colour"]),
                                         self._stream()), "sz_fetch_endings")
        return out

    def ending_stats(self):
        """(resignations, adjudicated draws, proven endings, holdout marks), all boards, cumulative (sz_ending_stats)"""
        out = (C.c_uint64 * 4)()
        N.check(N.lib().sz_ending_stats(self._e, out, self._stream()), "sz_ending_stats")
        return tuple(int(x) for x in out)

    def set_temperatures(self, temps):
        """Rewrite the per-board temperatures the next play() reads (no engine call: the device array sz_set_move_temperature was given is
        overwritten in stream order, as play() does with the uniforms).  temps: [B] numbers >= 0; a negative or NaN entry is a ValueError."""
        t = np.ascontiguousarray(temps, dtype=np.float64).reshape(-1)
        if t.shape[0] != self.B:
            raise ValueError("set_temperatures: %d temperatures for %d boards" % (t.shape[0], self.B))
        if not (t >= 0).all():                                   # NaN fails the comparison
            raise ValueError("set_temperatures: temperatures must be >= 0, got %r" % (t.tolist(),))
        if self._temps is None:
            self._temps = torch.zeros(self.B, dtype=torch.float64, device=self.device)
        self._temps.copy_(torch.from_numpy(t))

    def set_move_temperature(self, opts, temps=None):
        """Move-selection temperature (sz_set_move_temperature, a NON-REFERENCE option) from the next play() on, until changed.  opts: a dict
        with 'visit_offset' and 'value_cutoff' (None: no cutoff), as temperature_options_of returns it (the schedule keys are the caller's
        business and ignored here), or None = off.  temps: the boards' temperatures [B], uploaded (None: left as they are, 1.0 at first);
        set_temperatures() rewrites them between plies.  Between searches only; refused while Gumbel is on; kept subtrees are not touched."""
        if opts is None:
            N.check(N.lib().sz_set_move_temperature(self._e, None, None, self._stream()), "sz_set_move_temperature")
            self.temperature = None
            return
        if temps is not None or self._temps is None:
            self.set_temperatures(np.ones(self.B) if temps is None else temps)
        cut = opts.get("value_cutoff")
        o = N.sz_temperature_options(float(opts.get("visit_offset", 0.0)), 0.0 if cut is None else float(cut), int(cut is not None))
        N.check(N.lib().sz_set_move_temperature(self._e, C.byref(o), _ptr(self._temps), self._stream()), "sz_set_move_temperature")
        self.temperature = dict(opts)

    def fetch_temperature(self):
        """sz_fetch_temperature after play(): dict of [B] arrays: n_eligible (children the rule could have sampled; 1 on a greedy or
        proven-win play, 0 for a board that played no move) and p_chosen (the probability the move played had; 1.0 / NaN likewise)"""
        out = dict(n_eligible=np.zeros(self.B, np.int32), p_chosen=np.zeros(self.B, np.float64))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_fetch_temperature(self._e, p(out["n_eligible"]), p(out["p_chosen"]), self._stream()), "sz_fetch_temperature")
        return out

    def temperature_stats(self):
        """(plays sampled by the rule, greedy plays under the option, visited children excluded), all boards, cumulative (sz_temperature_stats)"""
        out = (C.c_uint64 * 3)()
        N.check(N.lib().sz_temperature_stats(self._e, out, self._stream()), "sz_temperature_stats")
        return tuple(int(x) for x in out)

    def set_quiet(self, quiet):
        """visit_targets mode with root_dirichlet_alpha: the boards whose searches get no root noise from the next begin() on (None: none)"""
        self.quiet = None if quiet is None else np.ascontiguousarray(quiet, dtype=np.uint8).reshape(-1).copy()

    def _compact_searching(self):
        """sz_compact_searching; returns n_live, or 0 when no board searches any more (the mapping is left alone then)"""
        n = C.c_int32()
        rc = N.lib().sz_compact_searching(self._e, _ptr(self.planes), C.byref(n), self._stream())
        if rc == N.SZ_ERR_STATE:
            return 0
        N.check(rc, "sz_compact_searching")
        self.n_rows, self._restore = int(n.value), True
        return self.n_rows

    def compact_searching(self):
        """In the middle of a search (between begin() and its last step): shrink the network batch to the boards that still search
        (sz_compact_searching); their pending network inputs move to rows 0..n_live*leaves_per_step-1 of self.planes.  Returns n_live.
        search() puts the caller's mapping (compact() on or off) back before the next search."""
        n = self._compact_searching()
        if n == 0:
            raise N.NativeError(N.SZ_ERR_STATE, "sz_compact_searching")
        return n

    def evaluate(self, planes):
        """model(x, inference=True) -> (policy probabilities [B,4672] f32, value [B] f32)"""
        policy, value = self.model(planes, inference=True)
        return policy.float().contiguous(), value.float().reshape(-1).contiguous()

    def set_root_noise(self, gamma):
        """gamma: [B, SZ_MAX_MOVES] f32 device tensor of Gamma(alpha,1) draws, or None for the reference behaviour"""
        self._gamma = None if gamma is None else gamma.to(self.device, torch.float32).contiguous()
        N.check(N.lib().sz_set_root_noise(self._e, _ptr(self._gamma)), "sz_set_root_noise")

    def begin(self):
        if self._restore:               # the last search shrank the batch: back to the mapping the caller chose (synchronises, like compact())
            self.compact(self._compact_on)
        if self.root_alpha is not None:
            gamma, self.next_gamma = self.next_gamma, None
            if gamma is None:
                gamma = torch._standard_gamma(torch.full((self.B, N.SZ_MAX_MOVES), float(self.root_alpha), device=self.device))
            if self.visit_targets:
                self.set_search_root_noise(gamma, self.quiet)
            else:
                self.set_root_noise(gamma)
        N.check(N.lib().sz_search_begin(self._e, _ptr(self.planes), self._stream()), "sz_search_begin")

    def step(self, policy, value):
        N.check(N.lib().sz_search_step(self._e, _ptr(policy), _ptr(value), _ptr(self.planes), self._stream()), "sz_search_step")

    def pending_boards(self):
        """boards still waiting for a network evaluation (sz_pending_boards; synchronises the stream)"""
        n = C.c_int32()
        N.check(N.lib().sz_pending_boards(self._e, C.byref(n), self._stream()), "sz_pending_boards")
        return int(n.value)

    def _run_steps(self, ev, n):
        """n network calls and search steps on the n_rows in use"""
        rows = self.n_rows * self.L
        planes = self.planes if rows == self.planes.shape[0] else self.planes[:rows]
        for _ in range(n):
            policy, value = ev(planes)
            self.step(policy, value)
        self.last_steps += n
        self.last_rows += n * rows

    def _run_pending(self, ev):
        """leaf batching: a collision ends a board's gather early, so the number of steps depends on the trees (at most S): after the
        ceil(S/L) steps that run without a host sync, one step at a time until no board waits for the network"""
        if self.L > 1:
            while self.last_steps < self.S and self.pending_boards():
                self._run_steps(ev, 1)

    @torch.no_grad()
    def search(self, evaluator=None):
        """All num_searches simulations for every active board (mcts.py:49-109).  The network sees n_rows * leaves_per_step rows.
        With budgets set the steps run in segments that end where boards run out of budget (search_segments), and after each segment
        the batch shrinks to the boards that still search; with max_shrinks > 0 it is also shrunk once right after the roots were made:
        boards with budget 0 and terminal roots never take a row.  Without budgets there is one segment and no shrink.
        args["visit_targets"]: the segments are planned from search_goals(), read after begin(); a board whose kept root already holds its
        target is done at begin and never takes a row.
        args["kld_stop"]: the steps run in chunks of ceil(interval / leaves_per_step); after a chunk comes check_stop(), then the first step
        of the next chunk, which takes in what the stopped boards had in flight, then the batch shrinks to the boards that still search (one
        stream synchronisation per check) and the search ends when there is none.  Segment ends shrink where they did."""
        ev = evaluator or self.evaluate
        self.begin()
        self.last_steps = self.last_rows = 0
        self.last_goals = None
        if self.n_rows <= 0:
            return
        budgets = self.budgets
        if self.visit_targets and self.targets is not None:
            # the goals are known only once the roots are made (a kept root's visits count): one more stream synchronisation, in this mode only
            budgets = self.last_goals = self.search_goals()
        segs = search_segments(budgets, self.L, self.max_shrinks, self.S)
        if budgets is not None and self.max_shrinks > 0 and self._compact_searching() == 0:
            return                                          # nothing to search: every board was done at begin
        if self.kld_stop is not None:
            return self._search_checked(ev, segs)
        for i, n in enumerate(segs):
            self._run_steps(ev, n)
            if i + 1 < len(segs) and self._compact_searching() == 0:
                return
        self._run_pending(ev)

    def _search_checked(self, ev, segs):
        """search()'s segments under args["kld_stop"]"""
        chunk = -(-self.kld_stop[1] // self.L)
        since, drain = 0, False                             # steps since the last check; a check was issued and its boards' leaves are still in flight
        for i, n in enumerate(segs):
            while n > 0:
                k = 1 if drain else min(n, chunk - since)
                self._run_steps(ev, k)
                n, since = n - k, since + k
                if drain:
                    drain = False
                    if self._compact_searching() == 0:
                        return
                if since == chunk:
                    self.check_stop()
                    since, drain = 0, True
            if i + 1 < len(segs) and self._compact_searching() == 0:
                return
        self._run_pending(ev)

    def stats(self):
        st = N.sz_stats()
        N.check(N.lib().sz_get_stats(self._e, C.byref(st), self._stream()), "sz_get_stats")
        return {k: getattr(st, k) for k, _ in N.sz_stats._fields_}

    def check_errors(self):
        """raises on a board that ended in an error state (NativeError) and on an f16 network whose forwards left f16's range since the last check
        (ValueError, raise_if_overflowed); stats() has synchronised the stream by then"""
        st = self.stats()
        if st["boards_error"]:
            raise N.NativeError(st["first_error"], "search (%d boards)" % st["boards_error"])
        raise_if_overflowed(self.model)
        return st

    def root_children(self):
        N.check(N.lib().sz_root_children(self._e, _ptr(self.root_action), _ptr(self.root_visits), _ptr(self.root_nchild),
                                         _ptr(self.root_prior), _ptr(self.root_wsum), self._stream()), "sz_root_children")
        torch.cuda.synchronize(self.device)
        return (self.root_action.cpu().numpy(), self.root_visits.cpu().numpy(), self.root_nchild.cpu().numpy(),
                self.root_prior.cpu().numpy(), self.root_wsum.cpu().numpy())

    def root_proven(self):
        """Proven results of the last search (sz_root_proven; all 0 without args["solver"]): (root [B] int8, children [B, SZ_MAX_MOVES] int8
        in action order as root_children()).  Codes _native.SZ_PROVEN_*: 0 unknown, 1 WIN, 2 DRAW, 3 LOSS, each for the side to move in
        that node's own position, so a root child with 3 is a winning move for the root."""
        root = torch.zeros(self.B, dtype=torch.int8, device=self.device)
        child = torch.zeros(self.B, N.SZ_MAX_MOVES, dtype=torch.int8, device=self.device)
        N.check(N.lib().sz_root_proven(self._e, _ptr(root), _ptr(child), self._stream()), "sz_root_proven")
        torch.cuda.synchronize(self.device)
        return root.cpu().numpy(), child.cpu().numpy()

    def solver_stats(self):
        """(simulations that ended on a proven non-terminal node, nodes proven by the update rule), all boards, cumulative (sz_solver_stats)"""
        out = (C.c_uint64 * 2)()
        N.check(N.lib().sz_solver_stats(self._e, out, self._stream()), "sz_solver_stats")
        return int(out[0]), int(out[1])

    def play(self, uniforms):
        """sim.py:68-76 for every board: sample with the given uniforms (one per board), play, test game over."""
        self.uniforms.copy_(torch.as_tensor(np.asarray(uniforms, dtype=np.float64)))
        N.check(N.lib().sz_play(self._e, _ptr(self.uniforms), self._stream()), "sz_play")

    def play_moves(self, actions):
        """Play given moves (sz_play_moves): actions is an integer array [n_boards], -1 = leave the board alone, else the action index to
        play there: another engine's move, a book move, a person's.  Legality is checked on the device (an illegal move flags the board,
        check_errors() raises); with reuse_subtree the board's tree is re-rooted at the move.  No training record; fetch_ply() reports
        chosen, game_over and result."""
        a = np.ascontiguousarray(actions, dtype=np.int32).reshape(-1)
        if a.shape[0] != self.B:
            raise ValueError("play_moves: %d actions for %d boards" % (a.shape[0], self.B))
        if self._moves is None:
            self._moves = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._moves.copy_(torch.from_numpy(a))
        N.check(N.lib().sz_play_moves(self._e, _ptr(self._moves), self._stream()), "sz_play_moves")

    def fetch_ply(self):
        B = self.B
        rec = dict(packed=np.zeros((B, N.SZ_PLANES, 8), np.uint8), action=np.zeros((B, N.SZ_MAX_MOVES), np.int32),
                   visits=np.zeros((B, N.SZ_MAX_MOVES), np.int32), n_child=np.zeros(B, np.int32), colour=np.zeros(B, np.uint8),
                   chosen=np.zeros(B, np.int32), game_over=np.zeros(B, np.uint8), result=np.zeros(B, np.int8), active=np.zeros(B, np.uint8))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_fetch_ply(self._e, p(rec["packed"]), p(rec["action"]), p(rec["visits"]), p(rec["n_child"]), p(rec["colour"]),
                                     p(rec["chosen"]), p(rec["game_over"]), p(rec["result"]), p(rec["active"]), self._stream()), "sz_fetch_ply")
        return rec

    def debug_pending(self):
        B = self.B
        mask = np.zeros((B, N.SZ_MASK_WORDS), np.uint64)
        depth, n_nodes, n_edges, status = (np.zeros(B, np.int32) for _ in range(4))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_debug_pending(self._e, p(mask), p(depth), p(n_nodes), p(n_edges), p(status), self._stream()), "sz_debug_pending")
        return mask, depth, n_nodes, n_edges, status

    def debug_tree(self, board):
        """whole tree of one board, depth-first in child order: (depth, action, visits, value_sum, prior) arrays; row 0 = the root"""
        n = C.c_int32()
        N.check(N.lib().sz_debug_tree(self._e, int(board), 0, None, None, None, None, None, C.byref(n), self._stream()), "sz_debug_tree")
        k = n.value
        d, a, v = (np.zeros(k, np.int32) for _ in range(3))
        w, pr = np.zeros(k, np.float64), np.zeros(k, np.float32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_debug_tree(self._e, int(board), k, p(d), p(a), p(v), p(w), p(pr), C.byref(n), self._stream()), "sz_debug_tree")
        return d, a, v, w, pr

    def debug_tree_proven(self, board):
        """(proven codes, complete bits) of every node of one board's tree, rows in debug_tree()'s order (sz_debug_tree_proven)"""
        n = C.c_int32()
        N.check(N.lib().sz_debug_tree_proven(self._e, int(board), 0, None, None, C.byref(n), self._stream()), "sz_debug_tree_proven")
        r, c = np.zeros(n.value, np.int8), np.zeros(n.value, np.uint8)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(N.lib().sz_debug_tree_proven(self._e, int(board), n.value, p(r), p(c), C.byref(n), self._stream()), "sz_debug_tree_proven")
        return r, c

    def debug_tree_values(self, board):
        """the stored network value of every node of one board's tree (f32, NaN where the node was never expanded), rows in debug_tree()'s
        order (sz_debug_tree_values; a search under set_gumbel_tree only)"""
        n = C.c_int32()
        N.check(N.lib().sz_debug_tree_values(self._e, int(board), 0, None, C.byref(n), self._stream()), "sz_debug_tree_values")
        val = np.zeros(n.value, np.float32)
        N.check(N.lib().sz_debug_tree_values(self._e, int(board), n.value, val.ctypes.data_as(C.c_void_p), C.byref(n), self._stream()), "sz_debug_tree_values")
        return val

    def debug_position(self, board):
        pos = np.zeros(10, np.uint64)
        ply = C.c_int32()
        N.check(N.lib().sz_debug_position(self._e, int(board), pos.ctypes.data_as(C.c_void_p), C.byref(ply), self._stream()), "sz_debug_position")
        return pos, ply.value


def unpack_bits128(planes):
    """[B,1024] uint8 (SZ_PLANES_NHWC128_BITS) -> [B,64,128] bf16 NHWC image (tests / inspection)."""
    B = planes.shape[0]
    v = planes.view(B, 4, 16, 16)                                   # [psub][cq][q] bytes
    bits = (v.unsqueeze(-1) >> torch.arange(8, device=planes.device, dtype=torch.uint8)) & 1      # [B,psub,cq,q,k]
    img = bits.permute(0, 3, 1, 2, 4).reshape(B, 64, 128)           # position = q*4 + psub, channel = cq*8 + k
    return img.to(torch.bfloat16)


def unpack_planes(packed):
    """(…,119,8) uint8 -> (…,119,8,8) bool; bit j of a byte = column j (train_RL.py:42 collatefn)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    return np.unpackbits(packed[..., None], axis=-1, bitorder="little").view(np.bool_)
