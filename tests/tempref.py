"""Plain-Python restatement of the move-selection temperature (sz_set_move_temperature / sz_fetch_temperature / sz_temperature_stats /
sz_debug_temperature, args["temperature"], a NON-REFERENCE option; include/sigmazero.h is the specification).  It is what wave_temperature and
the temperature branch of k_play<.., TempOpts> in csrc/sz_engine.hip are held to, bit for bit (tests/test_gpu_temperature.py).  Built on
fullref (Game), which already composes the ending rules, first-play urgency, forced playouts, visit targets, root noise, the solver and leaf
batching, and stays as it is:

  * choose() is the rule on plain arrays, pure: the counts sampled from, the tree's N and W, T, u, the options and the proving move of a WIN
    root -> Choice(move, kind, n_eligible, p_chosen, excluded, weights, eligible).  slog / sexp are gumbelref's, operator for operator the
    device's (csrc/sz_gumbel.h);
  * Game.set_move_temperature(opts, T) is sz_set_move_temperature plus the board's entry of temps_dev (opts None: off); Game.play(u) is
    fullref's play with the move choice replaced: the ending decision and the pruning run first, as in k_play; Game.last_temp =
    (n_eligible, p_chosen) is what sz_fetch_temperature says about that sz_play, Game.temp_stats what sz_temperature_stats counts;
  * CONFIGS / new_game() / begin_ply() / temps_of() / uniform_of() are the three engine configurations both test modules play, hook_cases() /
    hook_reference() the cases of sz_debug_temperature; cov counts, on the restatement alone, the branches the GPU cases must reach.

With opts None everywhere it is fullref (tests/test_temp_ref.py pins it)."""
import collections
import math

import numpy as np

import fullref as FU
import fpuref as FP
from composeref import LOSS, WIN
from forcedref import worst_case
from gumbelref import EXP_CUTOFF, sexp, slog                                       # noqa: F401 (re-exported)

F64 = np.float64
SAMPLED, GREEDY, PROVEN_WIN = 0, 1, 2                      # sz_debug_temperature's kind
Temp = collections.namedtuple("Temp", "visit_offset value_cutoff use_cutoff")      # sz_temperature_options
Choice = collections.namedtuple("Choice", "move kind n_eligible p_chosen excluded weights eligible")


def options(visit_offset=0.0, value_cutoff=None):
    """an sz_temperature_options with the two values as the f32 the struct holds; value_cutoff None = use_cutoff 0"""
    return Temp(float(np.float32(visit_offset)), 0.0 if value_cutoff is None else float(np.float32(value_cutoff)), int(value_cutoff is not None))


def first_max(n):
    return int(np.argmax(np.asarray(n, np.int64)))


def choose(n, N, W, T, u, opts, pmove=-1):
    """The rule of sz_set_move_temperature on a finished search.  n: the counts today's sampling reads, in child order (the counted visits,
    or the pruned ones); N, W: the tree's counted visits and value sums; T, u: the board's temperature and uniform; pmove: the first LOSS
    child of a root proven WIN, -1 = none -> Choice; weights / eligible are None on a greedy or proven-win play"""
    n = [int(x) for x in n]
    K = len(n)
    cs = first_max(n)
    off = float(np.float32(opts.visit_offset))
    astar = float(n[cs]) + off
    if pmove >= 0:
        return Choice(int(pmove), PROVEN_WIN, 1, 1.0, 0, None, None)
    T, u = float(T), float(u)
    if u < 0.0 or not (T > 0.0) or astar <= 0.0:
        return Choice(cs, GREEDY, 1, 1.0, 0, None, None)
    with np.errstate(all="ignore"):
        m = [-(F64(W[c]) / F64(float(N[c]))) for c in range(K)]
        floor_m = m[cs] - F64(float(np.float32(opts.value_cutoff)))
        lstar = slog(astar) if T != 1.0 else 0.0
        w, elig = [0.0] * K, [False] * K
        for c in range(K):
            if n[c] < 1:
                continue
            a = float(n[c]) + off
            ok = a > 0.0
            if ok and opts.use_cutoff:
                ok = bool(m[c] >= floor_m)
            if not ok:
                continue
            elig[c] = True
            if T == 1.0:
                w[c] = a
            else:
                d = slog(a) - lstar
                if d > 0.0:
                    d = 0.0
                w[c] = sexp(d / T)
        S = F64(0.0)
        for c in range(K):
            S = S + F64(w[c])
        acc = F64(0.0)
        for c in range(K):
            acc = acc + F64(w[c]) / S
        last = acc
        acc, idx = F64(0.0), 0
        for c in range(K):
            acc = acc + F64(w[c]) / S
            if acc / last <= u:
                idx = c + 1
        idx = min(idx, K - 1)
        p = float(F64(w[idx]) / S)
    visited = sum(1 for x in n if x >= 1)
    return Choice(idx, SAMPLED, sum(elig), p, visited - sum(elig), w, elig)


class Game(FU.Game):
    """fullref.Game with the temperature rule as the move choice of play()"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.temp_opts, self.T = None, 1.0
        self.last_temp = (0, math.nan)                    # sz_fetch_temperature's n_eligible and p_chosen of this board's last sz_play
        self.temp_stats = [0, 0, 0]                       # sz_temperature_stats
        self.choices = []                                 # per play under the option: (ply index, Choice)

    def set_move_temperature(self, opts, T=1.0):
        """sz_set_move_temperature and this board's temps_dev entry: never touches the kept subtree"""
        self.temp_opts, self.T = opts, float(T)

    def play(self, u):
        self.last_temp = (0, math.nan)                    # a board that plays no move (an ending fires) keeps this
        if self.temp_opts is None:
            return super().play(u)
        s = self.search

        def move(u_):
            acts, vis = s.root_children()
            k, f = len(acts), int(s.first[0])
            counts = s.pruned if getattr(s, "pruned", None) is not None else vis
            pmove = -1
            if s.solver and int(s.R[0]) == WIN:
                loss = np.nonzero(np.asarray(s.R[f:f + k]) == LOSS)[0]
                if len(loss):
                    pmove = int(loss[0])
            ch = choose(counts, vis, s.W[f:f + k], self.T, u_, self.temp_opts, pmove)
            self.last_temp = (ch.n_eligible, ch.p_chosen)
            self.temp_stats[0 if ch.kind == SAMPLED else 1] += 1
            self.temp_stats[2] += ch.excluded
            self.choices.append((len(self.chosen), ch))
            c = self.cov
            c["temp_sampled"] += ch.kind == SAMPLED
            c["temp_proven_win"] += ch.kind == PROVEN_WIN
            if ch.kind == GREEDY:
                c["temp_greedy_u"] += u_ < 0.0
                c["temp_greedy_T"] += not (self.T > 0.0)
                c["temp_greedy_offset"] += float(counts[first_max(counts)]) + self.temp_opts.visit_offset <= 0.0
            if ch.kind == SAMPLED:
                c["temp_T_is_1"] += self.T == 1.0
                c["temp_T_not_1"] += self.T != 1.0
                c["temp_excluded"] += ch.excluded > 0
                c["temp_on_pruned_counts"] += counts is not vis and bool((np.asarray(counts) != np.asarray(vis)).any())
                c["temp_not_cstar"] += ch.move != first_max(counts)
                c["temp_on_continued_ply"] += self.starts[-1] == "reused"
            return ch.move

        s.choose = move                                   # forcedref / composeref play() ask the search for the move
        try:
            return super().play(u)
        finally:
            del s.choose


# ---------------------------------------------------------------------------------------------------------------- the engine configurations
Config = collections.namedtuple("Config", "name S plies starts L solver reuse forced_k endings fpu salt")
# one engine each: 8 Chess960 boards, 24 simulations, 8 plies, HashModel("dyadic", salt); the option's settings change from ply to ply (OPTS)
STARTS = (0, 959, 518, 400, 77, 5, 811, 333)
BACK_RANK_FEN = "6k1/5ppp/8/8/8/8/8/R3K3 w - - 0 1"
CONFIGS = (
    Config("plain", 24, 8, STARTS, 1, False, False, 0.0, None, None, 3),
    # the last board is a back-rank mate in one: its root is proven WIN and the proving move is played whatever T is (`proven` endings stay off)
    Config("solver_forced_endings_fpu_L2", 24, 8, STARTS[:7] + (BACK_RANK_FEN,), 2, True, False, 2.0,
           dict(resign_value=-0.3, resign_patience=2, resign_min_ply=2, draw_value=0.0, draw_patience=0, draw_min_ply=0, proven=0), FP.CONFIGS["red_both"], 4),
    Config("reuse_subtree", 24, 8, STARTS, 1, False, True, 0.0, None, None, 5),
)
# sz_temperature_options by ply: none; lc0's offset with a cutoff; an offset that takes one-visit children out; a positive offset with cutoff 0
OPTS = (options(), options(-0.8, 0.1), options(-1.0), options(2.0, 0.0), options(-0.5, 2.0), options(), options(-1.0, 0.1), options(0.0, 0.1))
TEMPS = (1.0, 0.5, 0.25, 4.0, 0.05, 1.5, 0.0, 1.0)


def temps_of(ply, n_boards=8):
    """the boards' temperatures at a ply: different per board and per ply, every value of TEMPS on every board over 8 plies"""
    return [TEMPS[(b + 3 * ply) % len(TEMPS)] for b in range(n_boards)]


def uniform_of(b, ply):
    """board b's uniform at a ply: in [0, 1), exactly 0 and the largest double below 1 once each per board, negative (greedy) once"""
    k = (b + ply) % 8
    if k == 5:
        return -1.0
    if k == 2:
        return 0.0
    if k == 6:
        return float(np.nextafter(1.0, 0.0))
    return ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0


def engine_args(cfg):
    """the args of the SelfPlayEngine of a configuration (the temperature itself is set through set_move_temperature, ply by ply)"""
    args = {"C": 2, "num_searches": cfg.S}
    if cfg.L != 1 or cfg.solver:
        args.update(combine_options=True, leaves_per_step=cfg.L, virtual_loss=1.0, solver=cfg.solver)
    if cfg.reuse:
        args["reuse_subtree"] = True
    if cfg.forced_k:
        args["forced_playouts"] = cfg.forced_k
    if cfg.fpu is not None:
        args["fpu"] = FU.fpu_args(cfg.fpu)
    if cfg.endings is not None:
        args["endings"] = dict(cfg.endings, proven=bool(cfg.endings["proven"]))
    return args


def new_game(cfg, b, temperature=True):
    import sigma_zero_amd as sz
    st = cfg.starts[b]                                    # a Scharnagl number, or a FEN
    g = Game(sz.ChessTensor(fen=st) if isinstance(st, str) else sz.ChessTensor(chess960=True, scharnagl=st), cfg.S, worst_case(cfg.S) if cfg.reuse else None, reuse=cfg.reuse, L=cfg.L, lam=1.0,
             solver=cfg.solver, c=2.0, learning=True, mode="dyadic", salt=cfg.salt, fpu=cfg.fpu)
    if cfg.endings is not None:
        g.set_endings(FU.ER.options(**cfg.endings), False)
    g.with_temperature = bool(temperature)
    return g


def begin_ply(cfg, g, b, ply, opts="schedule", T="schedule"):
    """the setter calls and sz_search_begin of one ply on one board"""
    if g.with_temperature:
        g.set_move_temperature(OPTS[ply % len(OPTS)] if opts == "schedule" else opts, temps_of(ply, len(cfg.starts))[b] if T == "schedule" else T)
    return g.begin(None, None, False, cfg.forced_k)


def play(cfg, temperature=True, opts="schedule", T="schedule", u=uniform_of):
    """the restatement alone: every board of the configuration through its plies -> ([Game], per ply per board the record or None)"""
    games = [new_game(cfg, b, temperature) for b in range(len(cfg.starts))]
    recs = []
    for ply in range(cfg.plies):
        row = []
        for b, g in enumerate(games):
            if not g.live:
                row.append(None)
                continue
            begin_ply(cfg, g, b, ply, opts, T)
            g.run()
            assert g.error is None, g.error
            row.append(g.play(u(b, ply)))
        recs.append(row)
    return games, recs


def coverage(games, hook=None):
    c = collections.Counter(hook or {})
    for g in games:
        c.update(g.cov)
    return c


# what the engine configurations are there for (over the three of them together), and what each hook run must reach
COVERAGE = ("temp_sampled", "temp_greedy_u", "temp_greedy_T", "temp_greedy_offset", "temp_T_is_1", "temp_T_not_1", "temp_excluded", "temp_not_cstar",
            "temp_on_pruned_counts", "temp_on_continued_ply", "temp_proven_win")
HOOK_COVERAGE = ("greedy_u", "greedy_T_zero", "greedy_T_nan", "greedy_offset", "proven_win", "offset_excluded", "cutoff_excluded", "T_is_1", "T_not_1",
                 "single_visited", "cstar_tie", "zeros", "wide_case", "u_zero", "u_max_trailing_zero_weight", "u_zero_leading_zero_weight", "pruned_counts",
                 "plain_T1")


# ---------------------------------------------------------------------------------------------------------------- sz_debug_temperature cases
HookCases = collections.namedtuple("HookCases", "offsets n N W T u pmove opts")
HOOK_K = (1, 2, 63, 64, 65, 218)
HOOK_T = (0.0, 0.05, 0.25, 0.5, 1.0, 1.5, 4.0, math.nan)
HOOK_OFFSETS = (0.0, -0.5, -0.8, 2.0, "minus_max", -1.0)                         # -1.0: a one-visit child is out while c* stays in
HOOK_CUTOFFS = (None, 0.0, 0.1, 2.0)
OPT_FIELDS = [("visit_offset", np.float32), ("value_cutoff", np.float32), ("use_cutoff", np.int32)]      # sz_temperature_options as a numpy record


def hook_cases(n_cases=3840, seed=43):
    """Seeded cases for sz_debug_temperature: K of 1, 2, 63, 64, 65, 218; counts with zeros, ties for the maximum and a single visited child,
    large counts (800: 800^20 at T = 0.05) and pruned counts below the tree's; every T of HOOK_T, offset of HOOK_OFFSETS (the last one is
    minus the case's maximum count) and cutoff of HOOK_CUTOFFS; u = 0, a grid, the largest double below 1 and -1; a proving move now and then
    -> HookCases of flat arrays"""
    rng = np.random.default_rng(seed)
    ns, Ns, Ws, off = [], [], [], [0]
    T, u, pm, opts = np.zeros(n_cases), np.zeros(n_cases), np.full(n_cases, -1, np.int32), np.zeros(n_cases, np.dtype(OPT_FIELDS))
    top = float(np.nextafter(1.0, 0.0))
    for i in range(n_cases):
        k = HOOK_K[i % 6]
        kind = (i // 6) % 8
        n = rng.integers(0, 40, size=k)
        if kind == 0:
            n[rng.random(k) < 0.6] = 0                                           # many zeros
        if kind == 1 and k > 1:
            n[rng.choice(k, size=min(k, 3), replace=False)] = int(n.max()) + 1   # ties for the maximum, across lane passes when k > 64
        if kind == 2:
            n[:] = 0
            n[rng.integers(0, k)] = int(rng.integers(1, 30))                     # a single visited child
        if kind == 3:
            n = rng.integers(0, 4, size=k)                                       # small counts: the offsets take many out
        if kind == 4:
            n[rng.integers(0, k)] = 800                                          # 800 ^ 20
        if kind == 5 and k > 2:
            n[-(k // 3):] = 0                                                    # trailing children without a visit
        if kind == 6 and k > 2:
            n[:k // 3] = 0                                                       # leading children without a visit
        if n.max() < 1:
            n[rng.integers(0, k)] = 1                                            # k_play's zero-visit check: the maximum is at least 1
        N = n.copy()
        if kind == 7:                                                            # pruned counts: the tree's are larger, c* keeps its count
            cs = int(np.argmax(n))
            N = n + rng.integers(0, 3, size=k) * (n > 0)
            N[cs] = n[cs]
            N = np.minimum(N, n[cs])
            N = np.maximum(N, n)
        W = rng.uniform(-1.0, 1.0, size=k) * N
        T[i] = HOOK_T[int(rng.integers(0, len(HOOK_T)))]                         # independent draws: every combination of the three occurs (asserted)
        o = HOOK_OFFSETS[int(rng.integers(0, len(HOOK_OFFSETS)))]
        c = HOOK_CUTOFFS[int(rng.integers(0, len(HOOK_CUTOFFS)))]
        opts[i] = options(-float(n.max()) if o == "minus_max" else o, c)
        r = int(rng.integers(0, 20))
        u[i] = 0.0 if r == 0 else (top if r in (1, 2) else (-1.0 if r == 3 else int(rng.integers(0, 64)) / 64.0 if r < 12 else rng.random()))
        if rng.random() < 0.04:
            pm[i] = int(rng.integers(0, k))
        ns.append(n); Ns.append(N); Ws.append(W); off.append(off[-1] + k)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dt)
    return HookCases(np.array(off, np.int32), cat(ns, np.int32), cat(Ns, np.int32), cat(Ws, np.float64), T, u, pm, opts)


def hook_reference(hc):
    """the restatement's answers to the cases -> (move, kind, n_eligible, p_chosen, excluded, weights (NaN where none is written), Counter)"""
    n_cases = len(hc.T)
    move, kind, ne, ex = (np.zeros(n_cases, np.int32) for _ in range(4))
    p, w = np.zeros(n_cases), np.full(len(hc.n), np.nan)
    cov = collections.Counter()
    top = float(np.nextafter(1.0, 0.0))
    for i in range(n_cases):
        lo, hi = int(hc.offsets[i]), int(hc.offsets[i + 1])
        o = Temp(float(hc.opts[i]["visit_offset"]), float(hc.opts[i]["value_cutoff"]), int(hc.opts[i]["use_cutoff"]))
        n, N, W = hc.n[lo:hi], hc.N[lo:hi], hc.W[lo:hi]
        ch = choose(n, N, W, hc.T[i], hc.u[i], o, int(hc.pmove[i]))
        move[i], kind[i], ne[i], p[i], ex[i] = ch.move, ch.kind, ch.n_eligible, ch.p_chosen, ch.excluded
        cov["proven_win"] += ch.kind == PROVEN_WIN
        if ch.kind == GREEDY:
            cov["greedy_u"] += hc.u[i] < 0.0
            cov["greedy_T_zero"] += hc.T[i] == 0.0
            cov["greedy_T_nan"] += bool(np.isnan(hc.T[i]))
            cov["greedy_offset"] += float(n.max()) + o.visit_offset <= 0.0 and hc.u[i] >= 0.0 and hc.T[i] > 0.0
        if ch.kind != SAMPLED:
            continue
        w[lo:hi] = ch.weights
        assert ch.eligible[ch.move] or not (0.0 <= hc.u[i] < 1.0), i
        a = n.astype(np.float64) + o.visit_offset
        by_offset = int(((n >= 1) & ~(a > 0.0)).sum())
        cov["offset_excluded"] += by_offset > 0
        cov["cutoff_excluded"] += ch.excluded > by_offset
        cov["T_is_1"] += hc.T[i] == 1.0
        cov["T_not_1"] += hc.T[i] != 1.0
        cov["plain_T1"] += hc.T[i] == 1.0 and o.visit_offset == 0.0 and not o.use_cutoff
        cov["single_visited"] += int((n >= 1).sum()) == 1
        cov["cstar_tie"] += int((n == n.max()).sum()) >= 2
        cov["zeros"] += bool((n == 0).any())
        cov["wide_case"] += hi - lo > 64 and ch.move >= 64
        cov["u_zero"] += hc.u[i] == 0.0
        cov["u_zero_leading_zero_weight"] += hc.u[i] == 0.0 and ch.weights[0] == 0.0
        cov["u_max_trailing_zero_weight"] += hc.u[i] == top and ch.weights[-1] == 0.0
        cov["weight_cut_to_0"] += any(e and x == 0.0 for e, x in zip(ch.eligible, ch.weights))
        cov["pruned_counts"] += bool((N != n).any())
    return move, kind, ne, p, ex, w, cov
