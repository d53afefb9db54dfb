"""Plain-Python restatement of the visit-dependent exploration rate (sz_set_cpuct / sz_debug_cpuct, args["cpuct"], a NON-REFERENCE option;
include/sigmazero.h is the specification).  It is what puct_c (csrc/sz_engine.hip) and sz_cpuct (csrc/sz_cpuct.h), the selection of
k_search_step<.., PuctOpts> (the descent-only launch of sz_search_begin included) and the pruning of k_play<.., ForcedOpts, PuctOpts> are held
to, bit for bit (tests/test_gpu_cpuct.py).  Built on fullref through tempref (Game: fullref's with the move temperature as one more setting,
fullref itself while that is off), which stay as they are:

  * c_of(opts, n_p, is_root) is the rule, operator for operator, with slog from gumbelref;
  * Search._descend hands that c to every selection: fpuref.select (which is the plain arg-max at a REFERENCE site) at the parent's count
    n_p = N_p + k_p, the root's triple at the root and the tree's below, after forcedref's forced child at the root of a forced board, which
    takes the same c;
  * Game.cpuct is sz_set_cpuct for this board (a Cpuct, or None = off); begin() is sz_search_begin and takes it up for the whole search;
    play() hands pruning the root triple's c at the root's counted N;
  * the tree is never modified by the option: changing Game.cpuct between plies keeps the subtree kept for the next ply.

With Game.cpuct None it is fullref (tests/test_cpuct_ref.py pins it); with (C, b, 0) at both sites it is fullref with c = C.  CONFIGS and
hook_cases() are the inputs both test modules use; cov counts, on the restatement alone, the conditions the GPU cases must reach (COVERAGE)."""
import collections
import math

import numpy as np

import forcedref as FR
import fpuref as FP
import fullref as FU
import tempref as TM
from forcedref import WIDE_FEN, gammas, position_record, worst_case                # noqa: F401 (re-exported)
from gumbelref import slog
from vlref import F32

Cpuct = collections.namedtuple("Cpuct", "tree_init tree_base tree_factor root_init root_base root_factor")    # sz_cpuct_options
ALPHAZERO = Cpuct(1.25, 19652.0, 1.0, 1.25, 19652.0, 1.0)
NO_FPU = FP.Fpu(FP.REFERENCE, 0.0, FP.REFERENCE, 0.0)       # fpuref.select at a REFERENCE site is the plain arg-max


def site(opts, is_root):
    return (opts.root_init, opts.root_base, opts.root_factor) if is_root else (opts.tree_init, opts.tree_base, opts.tree_factor)


def c_of(opts, n_p, is_root):
    """sz_cpuct: the f32 that takes c_puct's place at a parent with n_p visits.  Python floats are IEEE f64: every operator one rounding"""
    init, base, factor = (float(np.float32(x)) for x in site(opts, is_root))
    x = ((float(int(n_p)) + base) + 1.0) / base
    return F32(init + factor * slog(x))


def checked(o):
    """sz_set_cpuct's refusals (SZ_ERR_INVALID) -> the Cpuct with f32 values"""
    o = Cpuct(*[float(np.float32(x)) for x in o])
    for init, base, factor in (site(o, False), site(o, True)):
        assert all(math.isfinite(x) for x in (init, base, factor)), "SZ_ERR_INVALID"
        assert 0.0 <= init <= 100.0 and 0.0 <= factor <= 100.0 and 1.0 <= base <= 1e9, "SZ_ERR_INVALID"
    return o


class Search(FP.Search):
    """fpuref.Search (and with it forcedref's) whose every selection takes c_of() at its parent's count in the place of the constant c.
    Game.begin() turns the ply's search into one: a search runs under one setting for its whole length."""
    cpuct = None

    def _pick(self, e, c):
        """the selection at parent e with the rate c: fpuref's arg-max, after forcedref's forced child at the root of a forced board"""
        f, k = int(self.first[e]), int(self.n[e])
        R = self.R[f:f + k] if self.solver else None
        n_p = int(self.N[e] + self.K[e])
        i, _, info = FP.select(self.N[f:f + k], self.K[f:f + k], self.W[f:f + k], self.P[f:f + k], R, n_p, int(self.N[e]), self.W[e], c, self.lam, e == 0,
                               self.fpu if self.fpu is not None else NO_FPU)
        forced = False
        if e == 0 and self.forced_k:
            j, forced, _ = FR.select_root(self.N[f:f + k], self.K[f:f + k], self.W[f:f + k], self.P[f:f + k], R, n_p, c, self.lam, self.forced_k)
            if forced:
                info["forced_overruled_fpu"] += self.fpu is not None and j != i
                i = j
        return i, forced, info

    def _descend(self):
        if self.cpuct is None:
            return super()._descend()
        path, e = [0], 0
        while self.n[e] > 0 and not (self.solver and self.R[e]):
            n_p = int(self.N[e] + self.K[e])
            i, forced, info = self._pick(e, c_of(self.cpuct, n_p, e == 0))
            self.forced_selections += forced
            if self.fpu is not None:
                self.cov.update(info)
            i0 = self._pick(e, F32(site(self.cpuct, e == 0)[0]))[0]      # what the constant `init` would have selected here
            self.cov["cpuct_changed_root" if e == 0 else "cpuct_changed_tree"] += i != i0
            self.cov["cpuct_parent_in_flight"] += self.L > 1 and int(self.K[e]) > 0
            self.cov["cpuct_wide_parent"] += int(self.n[e]) > 64
            e = int(self.first[e]) + i
            path.append(e)
        return path


class Game(TM.Game):
    """tempref.Game (fullref's while the temperature is off) with the option as a setting of the board: g.cpuct = Cpuct(...) or None between
    plies is sz_set_cpuct"""

    def __init__(self, *a, cpuct=None, **kw):
        super().__init__(*a, **kw)
        self.cpuct = cpuct
        self.cpuct_plies = []                            # per ply: the setting the search ran with

    def begin(self, target=None, gamma=None, quiet=False, forced_k=0.0):
        s = super().begin(target, gamma, quiet, forced_k)
        cp = None if self.cpuct is None else checked(self.cpuct)
        self.cpuct_plies.append(cp)
        if cp is not None:
            fk, fp = getattr(s, "forced_k", 0.0), getattr(s, "fpu", None)
            s.__class__, s.cpuct, s.forced_k, s.fpu = Search, cp, fk, fp
            self.cov["cpuct_kept_root_above_num_searches"] += bool(s.continued) and int(s.N[0]) > s.cap
        return s

    def play(self, u):
        s = self.search
        cp = getattr(s, "cpuct", None)
        if cp is None:
            return super().play(u)
        n_root = int(s.N[0])
        acts, vis = s.root_children()
        f, k = int(s.first[0]), len(acts)
        W, P = s.W[f:f + k].copy(), s.P[f:f + k].copy()
        c_const, s.c = s.c, c_of(cp, n_root, True)       # pruning reads the root triple's c at the root's counted N
        try:
            rec = super().play(u)
        finally:
            s.c = c_const
        if getattr(s, "forced_k", 0.0) and getattr(s, "pruned", None) is not None:
            flat = FR.prune(vis, W, P, n_root, F32(cp.root_init), s.forced_k)[0]
            self.cov["cpuct_changed_pruning"] += not np.array_equal(flat, s.pruned)
        return rec


# ---------------------------------------------------------------------------------------------------------------- the engine configurations
Config = collections.namedtuple("Config", "name S plies boards L solver reuse forced_k endings fpu noise targets temperature cpuct learning")
# one engine each; targets: per ply per board the visit target (a reuse engine) or None; temperature: per ply (Temp, T) or None; cpuct: per ply
Board = collections.namedtuple("Board", "name make mode salt u")

A = Cpuct(1.0, 8.0, 2.0, 2.5, 4.0, 1.0)                     # small bases: the rate moves within 32 simulations; root and tree differ
B_ = Cpuct(0.5, 16.0, 3.0, 1.5, 6.0, 2.0)
ENDINGS = dict(resign_value=-0.3, resign_patience=2, resign_min_ply=2, draw_value=0.0, draw_patience=0, draw_min_ply=0, proven=0)


def _u(b):
    return lambda ply: ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0


def _boards(names):
    import sigma_zero_amd as sz
    start = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    greedy = lambda ply: -1.0
    all_ = {"wide": Board("moves_218/rational/sampled", lambda: sz.ChessTensor(fen=WIDE_FEN), "rational", 1, _u(3)),
            "sp518": Board("sp518/rational/greedy", start(518), "rational", 518, greedy),
            "sp77": Board("sp77/peaked/greedy", start(77), "peaked", 77, greedy),
            "sp333": Board("sp333/peaked/sampled", start(333), "peaked", 333, _u(333)),
            "sp0": Board("sp0/dyadic/greedy", start(0), "dyadic", 0, greedy),
            # without noise and without the solver the mates a move away keep this root's subtree small while its visits grow
            "wide_greedy": Board("moves_218/dyadic/greedy", lambda: sz.ChessTensor(fen=WIDE_FEN), "dyadic", 3, greedy),
            "sp959": Board("sp959/dyadic/sampled", start(959), "dyadic", 959, _u(959))}
    return [all_[n] for n in names]


def configs():
    T = TM.options
    out = [
        Config("plain", 32, 4, _boards(["wide", "sp518", "sp77", "sp333"]), 1, False, False, 0.0, None, None, False, None, None, [A] * 4, True),
        # combine_options: leaf batching, the solver and reuse_subtree in one search
        Config("L4_solver_reuse", 32, 5, _boards(["sp518", "sp77", "sp0", "sp333"]), 4, True, True, 0.0, None, None, False, None, None, [A] * 5, False),
        Config("forced_fpu_endings_noise", 32, 4, _boards(["wide", "sp518", "sp77", "sp959"]), 1, False, False, 2.0, ENDINGS, FP.CONFIGS["red_tree_abs1_root"], True, None,
               None, [B_] * 4, True),
        # visit targets as a playout cap sets them: full and fast plies by board and ply
        Config("visit_targets_playout_cap", 32, 5, _boards(["sp518", "sp77", "sp0"]), 1, False, True, 0.0, None, None, False,
               [[32, 32, 32], [8, 32, 32], [32, 8, 32], [32, 32, 8], [8, 32, 32]], None, [A, A, B_, B_, A], True),
        Config("temperature", 24, 4, _boards(["sp518", "sp77", "sp333", "sp959"]), 1, False, False, 0.0, None, None, False, None,
               [(T(), 1.0), (T(-0.8, 0.1), 0.5), (T(-1.0), 0.25), (T(2.0, 0.0), 4.0)], [B_] * 4, True),
        # reuse_subtree alone, no noise: a kept root carries more than num_searches visits into its search
        Config("reuse_kept_root", 32, 4, _boards(["wide_greedy", "sp518", "sp77"]), 1, False, True, 0.0, None, None, False, None, None, [A] * 4, False),
    ]
    assert all(3 <= len(c.boards) <= 8 and 24 <= c.S <= 48 and 4 <= c.plies <= 6 and all(site(o, True) != site(o, False) for o in c.cpuct) for c in out)
    return out


def engine_args(cfg):
    """the args of the SelfPlayEngine of a configuration; the option itself is set through set_cpuct, ply by ply"""
    args = {"C": 2, "num_searches": cfg.S}
    if cfg.L != 1 or cfg.solver:
        args.update(combine_options=True, leaves_per_step=cfg.L, virtual_loss=1.0, solver=cfg.solver)
    if cfg.reuse:
        args["reuse_subtree"] = True
    if cfg.fpu is not None:
        args["fpu"] = FU.fpu_args(cfg.fpu)
    return args


def new_game(cfg, b, cpuct="config", c=2.0):
    bd = cfg.boards[b]
    g = Game(bd.make(), cfg.S, worst_case(cfg.S) if cfg.reuse else None, reuse=cfg.reuse, L=cfg.L, lam=1.0, solver=cfg.solver, c=c, learning=cfg.learning,
             mode=bd.mode, salt=bd.salt, fpu=cfg.fpu, cpuct=cfg.cpuct[0] if cpuct == "config" else cpuct)
    g.follow_config = cpuct == "config"
    if cfg.endings is not None:
        g.set_endings(FU.ER.options(**cfg.endings), False)
    return g


def begin_ply(cfg, g, b, ply, gam):
    """the setter calls and sz_search_begin of one ply on one board"""
    if g.follow_config:
        g.cpuct = cfg.cpuct[ply % len(cfg.cpuct)]
    if cfg.temperature is not None:
        g.set_move_temperature(*cfg.temperature[ply % len(cfg.temperature)])
    g.set_root_noise(cfg.noise)
    return g.begin(None if cfg.targets is None else cfg.targets[ply][b], gam[ply][b] if cfg.noise else None, False, cfg.forced_k)


def play(cfg, cpuct="config", c=2.0, plies=None):
    """the restatement alone: every board of the configuration through its plies -> ([Game], per ply per board the record or None)"""
    games, gam = [new_game(cfg, b, cpuct, c) for b in range(len(cfg.boards))], gammas(cfg) if cfg.noise else None
    recs = []
    for ply in range(cfg.plies if plies is None else plies):
        row = []
        for b, (g, bd) in enumerate(zip(games, cfg.boards)):
            if not g.live:
                row.append(None)
                continue
            begin_ply(cfg, g, b, ply, gam)
            g.run()
            assert g.error is None, g.error
            row.append(g.play(bd.u(ply)))
        recs.append(row)
    return games, recs


def coverage(played):
    """played: [[Game]] -> Counter of the conditions of COVERAGE"""
    c = collections.Counter()
    for games in played:
        for g in games:
            c.update(g.cov)
    return c


# the rate changed a selection at the root and below it; a parent had descents in flight (n_p = N_p + k_p); a kept root carried more than
# num_searches visits into its search; pruning under the rate left other counts than pruning under the constant `init`; a wide parent
COVERAGE = ("cpuct_changed_root", "cpuct_changed_tree", "cpuct_parent_in_flight", "cpuct_kept_root_above_num_searches", "cpuct_changed_pruning",
            "cpuct_wide_parent")


def assert_coverage(cov, names=COVERAGE):
    missing = [k for k in names if cov[k] < 1]
    assert not missing, "conditions not reached: %s of %s" % (missing, {k: cov[k] for k in COVERAGE})


# ---------------------------------------------------------------------------------------------------------------- sz_debug_cpuct cases
HookCases = collections.namedtuple("HookCases", "n_p is_root opts")
OPT_FIELDS = [(k, np.float32) for k in Cpuct._fields]      # sz_cpuct_options as a numpy record
HOOK_OPTS = (ALPHAZERO, A, B_, Cpuct(2.0, 7.0, 0.0, 3.0, 1e9, 0.0), Cpuct(0.0, 1.0, 100.0, 100.0, 1e9, 0.5), Cpuct(1.745, 38739.0, 3.894, 1.745, 38739.0, 3.894),
             Cpuct(0.1, 1.5, 0.3, 99.9, 3.0, 99.9))


def hook_cases(n_random=11632, seed=47):
    """Cases for sz_debug_cpuct and the stand-alone host program: every n_p of 0..300, the powers of two to 2^30 with both neighbours, 2^31 - 1
    and seeded draws (log-uniform to 2^31), each with every triple of HOOK_OPTS' root and tree side in turn -> HookCases"""
    rng = np.random.default_rng(seed)
    ns = list(range(0, 301))
    for k in range(9, 31):
        ns += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    ns.append(2 ** 31 - 1)
    ns += [int(x) for x in np.minimum(2.0 ** rng.uniform(0.0, 31.0, size=n_random), 2 ** 31 - 1)]
    n = len(ns)
    opts = np.zeros(n, np.dtype(OPT_FIELDS))
    for i in range(n):
        opts[i] = tuple(HOOK_OPTS[i % len(HOOK_OPTS)])
    return HookCases(np.array(ns, np.int32), np.array([(i // len(HOOK_OPTS)) % 2 for i in range(n)], np.uint8), opts)


def hook_reference(hc):
    """the restatement's answers to the cases -> c f32 [n]"""
    return np.array([c_of(Cpuct(*[x.item() for x in hc.opts[i]]), int(hc.n_p[i]), bool(hc.is_root[i])) for i in range(len(hc.n_p))], np.float32)
