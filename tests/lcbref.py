"""Plain-Python restatement of the per-edge value spread and of lower-confidence-bound move selection (sz_set_lcb / sz_fetch_lcb / sz_lcb_stats /
sz_root_value_spread / sz_debug_tree_spread / sz_debug_lcb, args["lcb"], a NON-REFERENCE option; include/sigmazero.h is the specification).  It
is what wave_lcb, the SpreadOpts instantiations of k_search_begin / k_search_step and the LcbOpts instantiations of k_play (csrc/sz_engine.hip)
and csrc/sz_lcb.h are held to, bit for bit (tests/test_gpu_lcb.py).  Built on summaryref, the top of the chain, which stays as it is:

  * ssqrt / mean / spread / radius / lcb_value / candidate repeat csrc/sz_lcb.h operator for operator on Python floats (IEEE f64, one rounding
    per operator); choose(n, N, W, Q, opts) is wave_lcb on plain arrays, lanes and butterfly included;
  * the second moment: begin() turns the ply's search, whatever kldref made of it, into one whose _backprop adds sv * sv to Q[e] wherever it
    adds sv to W[e] (the one backup of the whole chain: the network leaf, every pending leaf under leaf batching in leaf order, the visited and
    the new terminal, the solver's proven stop, a proven root's count-out one simulation at a time); Q is 0.0 where an edge is created (a
    fresh array per search: the option is refused with reuse_subtree); run() adds the terminal root's count-out Q[0] = (tv * tv) * S;
  * Game.lcb is sz_set_lcb for this board (an Lcb, or None = off), taken up by begin() for the whole search and its play(); play(u) is the
    chain's play with the rule where the move is "the most visited one": the negative-uniform path without the temperature option (never the
    proving move of a root proven WIN), tempref.choose's GREEDY kind with it.  Game.last_lcb is what sz_fetch_lcb says about that sz_play,
    Game.lcb_stats what sz_lcb_stats counts;
  * exact_ssqrt / exact_lcb are the same quantities by math.sqrt and rational arithmetic on the inputs, what tests/test_lcb_ref.py measures the
    restatement against.

Deviation of the restatement from the exact forms, measured by tests/test_lcb_ref.py: ssqrt within MEASURED_SSQRT_DEV of math.sqrt, relative,
over 200,000 seeded arguments in 2^+-200 and the hook cases' own arguments; lcb within MEASURED_LCB_DEV of max(1, |exact|) on hook_cases(),
whose spreads are either exactly 0 (equal values with short significands) or a search's worth.  The lcb figure (1.01e-13 measured, 2.22e-16
for ssqrt) is the cancellation in Q / N - m * m, not the square root: a child whose few values lie close together has a spread near 1e-5, the
difference carries an absolute error near 1e-16, and the square root of the quotient turns a relative 1e-11 into the figure seen at z = 5.
The test bounds are four times those.

CONFIGS and hook_cases() are the inputs both test modules use; cov counts, on the restatement alone, the conditions the GPU cases must reach."""
import collections
import fractions
import math
import struct

import numpy as np

import summaryref as SR
import kldref as KR
import tempref as TM
from composeref import WIN
from kldref import bits                                    # noqa: F401 (re-exported)

MAX_MOVES = 218
NAN = float("nan")
NONE_IDX = 0x7fffffff
MEASURED_SSQRT_DEV = 2.3e-16
MEASURED_LCB_DEV = 1.1e-13
SSQRT_BOUND = 4 * MEASURED_SSQRT_DEV
LCB_BOUND = 4 * MEASURED_LCB_DEV

Lcb = collections.namedtuple("Lcb", "stdevs min_visit_prop select")        # sz_lcb_options
Found = collections.namedtuple("Found", "move cstar lcb n_candidates bad")  # wave_lcb: the rule's move, c*, every child's bound, candidates, bad ssqrt arguments
Last = collections.namedtuple("Last", "move cstar lcb_move lcb_cstar n_candidates decided")      # sz_fetch_lcb of one board
NO_LCB = Last(-1, -1, NAN, NAN, 0, 0)                      # a board that made no choice in this sz_play


def options(stdevs=5.0, min_visit_prop=0.15, select=True):
    """an sz_lcb_options with the two values as the f32 the struct holds"""
    return Lcb(float(np.float32(stdevs)), float(np.float32(min_visit_prop)), int(bool(select)))


def checked(o):
    """sz_set_lcb's refusals (SZ_ERR_INVALID) -> the Lcb with f32 values"""
    o = options(*o)
    assert math.isfinite(o.stdevs) and o.stdevs >= 0.0 and 0.0 <= o.min_visit_prop <= 1.0, "SZ_ERR_INVALID"
    return o


# ---------------------------------------------------------------------------------------------------------------- csrc/sz_lcb.h
def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _f64(u):
    return struct.unpack("<d", struct.pack("<Q", u & 0xffffffffffffffff))[0]


def ssqrt(x):
    """sz_ssqrt -> (value, bad)"""
    x = float(x)
    if x == 0.0:
        return 0.0, 0
    u = _bits(x)
    be = (u >> 52) & 0x7ff
    if (u >> 63) != 0 or be == 0 or be == 0x7ff:
        return 0.0, 1
    e = be - 1023
    mb = (u & 0x000fffffffffffff) | 0x3ff0000000000000
    if e & 1:                                              # Python's & on a negative int is two's complement too
        mb, e = mb + 0x0010000000000000, e - 1
    m = _f64(mb)
    y = 0.5 * (1.0 + m)
    for _ in range(6):
        y = 0.5 * (y + m / y)
    return y * _f64((e // 2 + 1023) << 52), 0              # e is even: // is exact


def mean(w, n):
    """sz_lcb_mean"""
    return -(float(w) / float(int(n)))


def spread(q, n, m):
    """sz_lcb_spread"""
    s = float(q) / float(int(n)) - m * m
    if not (s > 0.0):
        s = 0.0
    return s


def radius(z, s, n):
    """sz_lcb_radius -> (r, bad)"""
    r, bad = ssqrt(s / float(int(n) - 1))
    return z * r, bad


def lcb_value(n, w, q, z):
    """sz_lcb_value -> (lcb, bad); NaN with n < 2"""
    if int(n) < 2:
        return NAN, 0
    m = mean(w, n)
    r, bad = radius(z, spread(q, n, m), n)
    return m - r, bad


def candidate(N_c, n_c, n_star, p):
    """sz_lcb_candidate"""
    return int(N_c) >= 2 and int(n_c) >= 1 and float(int(n_c)) >= p * float(int(n_star))


def first_max(n):
    return int(np.argmax(np.asarray(n, np.int64)))


def choose(n, N, W, Q, opts):
    """wave_lcb.  n: the counts the move choice reads, in child order; N, W, Q: the tree's -> Found"""
    with np.errstate(all="ignore"):
        K = len(n)
        cs = first_max(n)
        z, p = float(np.float32(opts.stdevs)), float(np.float32(opts.min_visit_prop))
        best, bi = [0.0] * 64, [NONE_IDX] * 64
        vals, cand, bad = [], 0, 0
        for c in range(K):
            v, b = lcb_value(N[c], float(W[c]), float(Q[c]), z)
            vals.append(v)
            bad += b
            if not candidate(N[c], n[c], n[cs], p):
                continue
            cand += 1
            l = c % 64
            if bi[l] == NONE_IDX or v > best[l]:
                best[l], bi[l] = v, c
        off = 32
        while off >= 1:
            nb, ni = list(best), list(bi)
            for l in range(64):
                ob, oi = best[l ^ off], bi[l ^ off]
                if oi != NONE_IDX and (bi[l] == NONE_IDX or ob > best[l] or (ob == best[l] and oi < bi[l])):
                    nb[l], ni[l] = ob, oi
            best, bi = nb, ni
            off >>= 1
    return Found(cs if bi[0] == NONE_IDX else bi[0], cs, vals, cand, bad)


def exact_ssqrt(x):
    return math.sqrt(x)


def exact_lcb(n, w, q, z):
    """lcb of the inputs as they are: the mean and the variance in rational arithmetic, one math.sqrt"""
    F = fractions.Fraction
    m = -F(float(w)) / int(n)
    s = max(F(float(q)) / int(n) - m * m, F(0)) / (int(n) - 1)
    return float(m) - float(z) * math.sqrt(s)


# ---------------------------------------------------------------------------------------------------------------- the second moment
class Spread:
    """Mixed in front of the class a ply's search has (Game.begin): every backup adds the square beside the value, in the same order"""
    lcb = None                                             # the Lcb the search runs under

    def _backprop(self, path, v):
        d = len(path) - 1
        for j, e in enumerate(path):
            sv = v if (d - j) % 2 == 0 else -v
            self.Q[e] = self.Q[e] + sv * sv
        self.q_backups += 1
        super()._backprop(path, v)

    def tree_spread(self):
        """Q of every edge in tree()'s order (sz_debug_tree_spread)"""
        out, stack = [], [0]
        while stack:
            e = stack.pop()
            out.append(float(self.Q[e]))
            if self.first[e] >= 0:
                stack += [int(self.first[e]) + k for k in range(int(self.n[e]) - 1, -1, -1)]
        return np.array(out, np.float64)

    def root_spread(self):
        f, k = int(self.first[0]), int(self.n[0])
        return self.Q[f:f + k].copy() if f >= 0 else np.zeros(0, np.float64)


_classes = {}


def with_spread(cls):
    if cls not in _classes:
        _classes[cls] = type("Spread" + cls.__name__, (Spread, cls), {})
    return _classes[cls]


class Game(KR.Game):
    """kldref.Game with the option as a setting of the board: g.lcb = Lcb(...) or None between plies is sz_set_lcb"""

    def __init__(self, *a, lcb=None, **kw):
        super().__init__(*a, **kw)
        assert not self.reuse or lcb is None, "SZ_ERR_STATE: refused on a reuse_subtree engine"
        self.lcb = lcb
        self.lcb_plies = []                              # per ply: the setting the search ran with
        self.last_lcb = NO_LCB
        self.lcb_stats = [0, 0, 0]                       # sz_lcb_stats of this board
        self.lcb_log = []                                # per play under the option: (ply index, Found, decided, greedy)

    def begin(self, target=None, gamma=None, quiet=False, forced_k=0.0):
        s = super().begin(target, gamma, quiet, forced_k)
        lo = None if self.lcb is None else checked(self.lcb)
        assert lo is None or not self.reuse, "SZ_ERR_STATE"
        self.lcb_plies.append(lo)
        if lo is not None:
            s.__class__ = with_spread(s.__class__)
            s.lcb, s.Q, s.q_backups = lo, np.zeros(len(s.W), np.float64), 0
        return s

    def run(self):
        s = super().run()
        if getattr(s, "lcb", None) is not None and s.q_backups == 0 and int(s.n[0]) == 0:
            tv, term = s.games[0].get_value_and_terminated()        # a terminal root (or no budget): counted out at once in k_search_begin
            S = max(int(s.goal0), 0)
            tv = float(tv) if term else 0.0
            s.Q[0] = (tv * tv) * float(S)
            self.cov["lcb_terminal_root_counted_out"] += term and S > 0
        return s

    def _rule(self, n, N, W, greedy):
        """wave_lcb and its bookkeeping in k_play -> the Found and whether the rule decides"""
        s = self.search
        f = int(s.first[0])
        fd = choose(n, N, W, s.Q[f:f + len(n)], s.lcb)
        decided = bool(greedy) and bool(s.lcb.select)
        self.last_lcb = Last(fd.move, fd.cstar, fd.lcb[fd.move], fd.lcb[fd.cstar], fd.n_candidates, int(decided))
        self.lcb_stats[0] += decided
        self.lcb_stats[1] += fd.move != fd.cstar
        self.lcb_stats[2] += fd.bad
        self.lcb_log.append((len(self.chosen), fd, decided, bool(greedy)))
        c = self.cov
        c["lcb_decided_differs"] += decided and fd.move != fd.cstar
        c["lcb_decided_same"] += decided and fd.move == fd.cstar
        c["lcb_observed_differs"] += (not decided) and fd.move != fd.cstar
        c["lcb_no_candidate"] += fd.n_candidates == 0
        c["lcb_cstar_not_candidate"] += fd.n_candidates > 0 and not candidate(N[fd.cstar], n[fd.cstar], n[fd.cstar], s.lcb.min_visit_prop)
        c["lcb_on_pruned_counts"] += bool((np.asarray(n) != np.asarray(N)).any())
        c["lcb_wide_root"] += len(n) > 64
        return fd, decided

    def play(self, u):
        self.last_lcb = NO_LCB                            # a board that makes no choice (an ending fires) keeps this
        s = self.search
        if getattr(s, "lcb", None) is None:
            return super().play(u)
        if self.temp_opts is not None:                    # tempref.Game.play asks tempref.choose: its GREEDY kind is where the rule applies
            inner = TM.choose

            def tempered(n, N, W, T, u_, opts, pmove=-1):
                ch = inner(n, N, W, T, u_, opts, pmove)
                fd, decided = self._rule(n, N, W, ch.kind == TM.GREEDY)
                self.cov["lcb_proving_move"] += ch.kind == TM.PROVEN_WIN
                self.cov["lcb_greedy_by_T"] += ch.kind == TM.GREEDY and not (u_ < 0.0)
                return ch._replace(move=fd.move) if decided else ch

            TM.choose = tempered
            try:
                return super().play(u)
            finally:
                TM.choose = inner
        base = s.choose                                   # forcedref / composeref play() ask the search for the move

        def move(u_):
            i = base(u_)
            acts, vis = s.root_children()
            f, k = int(s.first[0]), len(acts)
            counts = s.pruned if getattr(s, "pruned", None) is not None else vis
            proven = bool(s.solver) and int(s.R[0]) == WIN
            fd, decided = self._rule(counts, vis, s.W[f:f + k], u_ < 0.0 and not proven)
            self.cov["lcb_proving_move"] += proven
            return fd.move if decided else i

        s.choose = move
        try:
            return super().play(u)
        finally:
            del s.choose


# ---------------------------------------------------------------------------------------------------------------- the engine configurations
Config = collections.namedtuple("Config", "name S plies boards L solver forced_k endings fpu budgets kld temperature summary lcb learning")
# one engine each, without reuse_subtree; budgets: per ply per board or None; kld: the KldStop of every ply; temperature: per ply (Temp,
# temperatures per board) or None; summary: the search summary is on; lcb: per ply the Lcb of sz_set_lcb
Board = KR.Board
ENDINGS = dict(resign_value=-0.05, resign_patience=2, resign_min_ply=2, draw_value=0.0, draw_patience=0, draw_min_ply=0, proven=0)
# min_visit_prop over 0, 0.15, 0.5, 1 and stdevs over 0, 1, 5, ply by ply; the last one observes
LCBS = (options(0.0, 0.0), options(5.0, 0.15), options(1.0, 0.5), options(0.0, 1.0), options(1.0, 0.0), options(5.0, 0.5), options(1.0, 0.15, False), options(0.0, 0.15))


def _boards(spec):
    import sigma_zero_amd as sz
    start = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    fen = lambda f: (lambda: sz.ChessTensor(fen=f))
    greedy = lambda ply: -1.0
    mixed = lambda b: (lambda ply: -1.0 if (b + ply) % 3 else KR.PR._u(b)(ply))
    out = []
    for b, (name, mode, salt, kind) in enumerate(spec):
        make = fen(KR.WIDE_FEN) if name == "wide" else (fen(KR.MATE_IN_1_FEN) if name == "mate1" else start(int(name[2:])))
        u = greedy if kind == "greedy" else (KR.PR._u(salt + 1) if kind == "sampled" else mixed(b))
        out.append(Board("%s/%s/%s" % (name, mode, kind), make, mode, salt, u))
    return out


def configs():
    """8 boards, 24 simulations, 6-8 plies: plain with greedy plays; leaf batching L = 2 + the solver + forced playouts + FPU + endings + the
    move temperature with T = 0 on some boards and plies; playout-cap budgets + kld_stop + the search summary"""
    import fpuref as FP
    S = 24
    plain = _boards([("wide", "rational", 1, "greedy"), ("sp518", "rational", 518, "greedy"), ("sp77", "peaked", 77, "greedy"), ("sp333", "peaked", 333, "mixed"),
                     ("sp0", "dyadic", 0, "greedy"), ("sp959", "dyadic", 959, "sampled"), ("sp400", "rational", 400, "greedy"), ("mate1", "rational", 2, "greedy")])
    full = _boards([("sp0", "dyadic", 4, "mixed"), ("sp959", "dyadic", 4, "mixed"), ("sp518", "dyadic", 4, "mixed"), ("sp400", "dyadic", 4, "mixed"),
                    ("sp77", "dyadic", 4, "mixed"), ("sp5", "dyadic", 4, "mixed"), ("wide", "dyadic", 4, "mixed"), ("mate1", "rational", 2, "mixed")])
    caps = _boards([("sp518", "rational", 518, "greedy"), ("sp77", "peaked", 77, "greedy"), ("sp0", "dyadic", 0, "mixed"), ("sp333", "peaked", 333, "greedy"),
                    ("sp959", "dyadic", 959, "sampled"), ("sp400", "rational", 400, "greedy"), ("sp17", "dyadic", 17, "greedy"), ("sp811", "rational", 811, "mixed")])
    budgets = [[S if (b + ply) % 3 else 12 for b in range(8)] for ply in range(6)]
    temps = [(TM.OPTS[ply % len(TM.OPTS)], TM.temps_of(ply, 8)) for ply in range(8)]
    out = [
        Config("plain_greedy", S, 6, plain, 1, False, 0.0, None, None, None, None, None, False, LCBS, True),
        Config("L2_solver_forced_fpu_endings_temperature", S, 8, full, 2, True, 2.0, ENDINGS, FP.CONFIGS["red_both"], None, None, temps, False, LCBS, True),
        Config("playout_cap_budgets_kld_summary", S, 6, caps, 1, False, 0.0, None, None, budgets, KR.KldStop(6e-3, 8, 8), None, True, LCBS, True),
    ]
    assert all(len(c.boards) == 8 and c.S == 24 and 6 <= c.plies <= 8 for c in out)
    return out


def engine_args(cfg):
    """the args of the SelfPlayEngine of a configuration; the option itself is set through set_lcb, ply by ply"""
    args = {"C": 2, "num_searches": cfg.S}
    if cfg.L != 1 or cfg.solver:
        args.update(combine_options=True, leaves_per_step=cfg.L, virtual_loss=1.0, solver=cfg.solver)
    if cfg.fpu is not None:
        args["fpu"] = KR.PR.FU.fpu_args(cfg.fpu)
    return args


def lcb_of(cfg, ply, lcb="config"):
    return cfg.lcb[ply % len(cfg.lcb)] if lcb == "config" else lcb


def new_game(cfg, b, lcb="config"):
    bd = cfg.boards[b]
    g = Game(bd.make(), cfg.S, None, reuse=False, L=cfg.L, lam=1.0, solver=cfg.solver, c=2.0, learning=cfg.learning, mode=bd.mode, salt=bd.salt,
             fpu=cfg.fpu, cpuct=None, kld_stop=cfg.kld, lcb=lcb_of(cfg, 0, lcb))
    g.lcb_mode = lcb
    if cfg.endings is not None:
        g.set_endings(KR.PR.FU.ER.options(**cfg.endings), False)
    return g


def begin_ply(cfg, g, b, ply):
    """the setter calls and sz_search_begin of one ply on one board"""
    g.lcb = lcb_of(cfg, ply, g.lcb_mode)
    if cfg.temperature is not None:
        opts, temps = cfg.temperature[ply % len(cfg.temperature)]
        g.set_move_temperature(opts, temps[b])
    return g.begin(None if cfg.budgets is None else cfg.budgets[ply][b], None, False, cfg.forced_k)


def uniform_of(cfg, b, ply):
    return TM.uniform_of(b, ply) if cfg.temperature is not None else cfg.boards[b].u(ply)


def play(cfg, lcb="config"):
    """the restatement alone: every board of the configuration through its plies -> ([Game], per ply per board the record or None, per ply per
    board the Last (NO_LCB for a board that does not play))"""
    games = [new_game(cfg, b, lcb) for b in range(len(cfg.boards))]
    recs, lasts = [], []
    for ply in range(cfg.plies):
        row, lrow = [], []
        for b, g in enumerate(games):
            if not g.live:
                row.append(None), lrow.append(NO_LCB)
                continue
            begin_ply(cfg, g, b, ply)
            g.run()
            assert g.error is None, g.error
            row.append(g.play(uniform_of(cfg, b, ply)))
            lrow.append(g.last_lcb)
        recs.append(row), lasts.append(lrow)
    return games, recs, lasts


def coverage(games, hook=None):
    c = collections.Counter(hook or {})
    for g in games:
        c.update(g.cov)
    return c


# per configuration: a play the rule decided with another move than c*, and one with c*
CONFIG_COVERAGE = ("lcb_decided_differs", "lcb_decided_same")
# over the three together: a board without a candidate, the proving move of a root proven WIN, a greedy play by T = 0, pruned counts, a wide
# root, a play the option only observed
ENGINE_COVERAGE = ("lcb_no_candidate", "lcb_proving_move", "lcb_greedy_by_T", "lcb_on_pruned_counts", "lcb_wide_root", "lcb_observed_differs")
HOOK_COVERAGE = ("move_not_cstar", "no_candidate", "cstar_not_candidate", "lcb_tie", "lcb_tie_same_lane", "pruned_counts", "zero_spread", "wide_move",
                 "single_candidate", "p_one_ties_only")


def assert_coverage(cov, names):
    missing = [k for k in names if cov[k] < 1]
    assert not missing, "conditions not reached: %s of %s" % (missing, {k: cov[k] for k in names})


# ---------------------------------------------------------------------------------------------------------------- sz_debug_lcb cases
HookCases = collections.namedtuple("HookCases", "offsets n N W Q opts")
HOOK_K = (1, 2, 63, 64, 65, 127, 128, 129, 218)            # the 64-lane stride boundaries and the maximum
HOOK_Z = (0.0, 1.0, 5.0)
HOOK_P = (0.0, 0.15, 0.5, 1.0)
OPT_FIELDS = [("stdevs", np.float32), ("min_visit_prop", np.float32), ("select", np.int32)]      # sz_lcb_options as a numpy record
SHORT = np.array([-1.0, -0.75, -0.5, -0.125, 0.0, 0.25, 0.5, 0.625, 1.0])                        # values whose squares and sums stay exact


def moments(values):
    """W and Q of a child through which these values were backed up, in order: the engine's two sums"""
    w = q = 0.0
    for v in values:
        v = float(v)
        w, q = w + v, q + v * v
    return w, q


def hook_cases(n_cases=1440, seed=71):
    """Seeded cases for sz_debug_lcb, the stand-alone host program and the accuracy test.  Every K of HOOK_K, z of HOOK_Z and p of HOOK_P.  A
    child's W and Q are the sums of N values a search could have backed up: f32 values in [-1, 1] around the child's own mean, or N equal
    short values (spread exactly 0).  Kinds: a search's worth of visits with unvisited and once-visited children; every child below two
    visits (no candidate); counts at most 1 with tree counts above (c* is no candidate); copies of one child 64 apart and next to each other
    (ties in lcb); pruned counts below the tree's; all spreads zero -> HookCases of flat arrays"""
    rng = np.random.default_rng(seed)
    ns, Ns, Ws, Qs, off = [], [], [], [], [0]
    opts = np.zeros(n_cases, np.dtype(OPT_FIELDS))
    for i in range(n_cases):
        k = HOOK_K[i % len(HOOK_K)]
        kind = (i // len(HOOK_K)) % 8
        total = int(rng.choice([24, 48, 200, 800]))
        N = rng.multinomial(total, rng.dirichlet(np.full(k, 0.3 if k > 2 else 1.0)))
        if kind == 1:
            N = rng.integers(0, 2, size=k)                                       # no child with two visits
            N[int(rng.integers(0, k))] = 1
        if kind == 5:
            N = np.maximum(N, rng.integers(0, 5, size=k))                        # few children unvisited
        if N.max() < 1:
            N[int(rng.integers(0, k))] = 1
        centre = rng.uniform(-0.9, 0.9, size=k)
        vals = []
        for c in range(k):
            if kind == 4 or (kind == 0 and rng.random() < 0.2):
                vals.append(np.full(N[c], SHORT[int(rng.integers(0, len(SHORT)))]))
            else:
                vals.append(np.clip(centre[c] + rng.normal(0.0, 0.3, size=N[c]), -1.0, 1.0).astype(np.float32).astype(np.float64))
        if kind == 3 and k > 1:                                                  # ties: copies of one well-visited child
            src = int(np.argmax(N))
            for dst in ([src + 64] if src + 64 < k else []) + [(src + 1) % k]:
                N[dst], vals[dst] = N[src], vals[src].copy()
        n = N.copy()
        if kind == 2:                                                            # counts at most 1: c* has N_c* = 1, others N >= 2 pruned to 1
            n = np.minimum(N, 1)
            cs = first_max(n)
            N[cs], vals[cs] = 1, vals[cs][:1] if len(vals[cs]) else np.array([0.25])
            n[cs] = 1
        if kind in (6, 7) and k > 1:                                             # pruning: c* keeps its count
            cs = first_max(n)
            cut = rng.integers(0, 4, size=k)
            cut[cs] = 0
            n = np.maximum(N - cut, 0)
        WQ = [moments(v) for v in vals]
        opts[i] = (HOOK_Z[int(rng.integers(0, 3))], HOOK_P[int(rng.integers(0, 4))], int(rng.integers(0, 2)))
        ns.append(n), Ns.append(N), Ws.append([w for w, _ in WQ]), Qs.append([q for _, q in WQ]), off.append(off[-1] + k)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x) for x in xs]), dt)
    return HookCases(np.array(off, np.int32), cat(ns, np.int32), cat(Ns, np.int32), cat(Ws, np.float64), cat(Qs, np.float64), opts)


def hook_case(hc, i):
    lo, hi = int(hc.offsets[i]), int(hc.offsets[i + 1])
    o = Lcb(float(hc.opts[i]["stdevs"]), float(hc.opts[i]["min_visit_prop"]), int(hc.opts[i]["select"]))
    return hc.n[lo:hi], hc.N[lo:hi], hc.W[lo:hi], hc.Q[lo:hi], o


def hook_reference(hc):
    """the restatement's answers to the cases -> (move, cstar, n_candidates, bad [n] int32 each, lcb flat f64, Counter)"""
    n_cases = len(hc.opts)
    move, cstar, ncand, bad = (np.zeros(n_cases, np.int32) for _ in range(4))
    lcb = np.full(len(hc.n), NAN)
    cov = collections.Counter()
    for i in range(n_cases):
        n, N, W, Q, o = hook_case(hc, i)
        fd = choose(n, N, W, Q, o)
        lo = int(hc.offsets[i])
        move[i], cstar[i], ncand[i], bad[i] = fd.move, fd.cstar, fd.n_candidates, fd.bad
        lcb[lo:lo + len(n)] = fd.lcb
        cands = [c for c in range(len(n)) if candidate(N[c], n[c], n[fd.cstar], o.min_visit_prop)]
        top = [c for c in cands if fd.lcb[c] == fd.lcb[fd.move]]
        cov["move_not_cstar"] += fd.move != fd.cstar
        cov["no_candidate"] += not cands
        cov["cstar_not_candidate"] += bool(cands) and fd.cstar not in cands
        cov["lcb_tie"] += len(top) >= 2
        cov["lcb_tie_same_lane"] += len(top) >= 2 and any(c - top[0] >= 64 for c in top)
        cov["pruned_counts"] += bool((n != N).any())
        cov["zero_spread"] += any(N[c] >= 2 and fd.lcb[c] == mean(W[c], N[c]) and o.stdevs > 0 for c in range(len(n)))
        cov["wide_move"] += fd.move >= 64
        cov["single_candidate"] += len(cands) == 1
        cov["p_one_ties_only"] += o.min_visit_prop == 1.0 and bool(cands) and all(n[c] == n[fd.cstar] for c in cands)
    return move, cstar, ncand, bad, lcb, cov


def ssqrt_arguments(n=4000, seed=73):
    """arguments for the device's ssqrt: seeded normal numbers over 2^+-200, exact squares, the ends of the normal range, 0.0, and the ones the
    rule treats as 0.0 (negative, subnormal, infinite, NaN)"""
    rng = np.random.default_rng(seed)
    x = list(2.0 ** rng.uniform(-200.0, 200.0, size=n))
    x += [float(k * k) for k in range(1, 200)] + [1.0, 2.0, 4.0, float(np.nextafter(4.0, 0.0)), float(np.nextafter(1.0, 2.0)), 0.25, 0.5]
    x += [2.2250738585072014e-308, 1.7976931348623157e308, 0.0, -0.0, -1.0, 5e-324, 1e-310, math.inf, -math.inf, NAN]
    return np.array(x, np.float64)


same_bits = SR.same_bits
