"""Plain-Python restatement of KLD-gain early stopping of a board's search (sz_set_kld_stop / sz_search_check_stop / sz_debug_kld_gain,
args["kld_stop"], a NON-REFERENCE option; include/sigmazero.h is the specification).  It is what wave_kld_gain and k_kld_check
(csrc/sz_engine.hip) and sz_kld_term (csrc/sz_kldgain.h) are held to, bit for bit (tests/test_gpu_kld_stop.py).  Built on puctref, which stays
as it is:

  * term(prev_c, prev_total, now_c, new_total) and gain(prev, now) are the rule, operator for operator, with slog from gumbelref, the sum in the
    lane-partial and butterfly order;
  * Stepwise is composeref.Search._run with a point after sz_search_begin and after every sz_search_step where a check can be made; Game.begin()
    turns the ply's search, whatever puctref made of it, into one (test_kld_ref pins it to puctref's while the option is off);
  * Game.kld_stop is sz_set_kld_stop for this board (a KldStop, or None = off), Game.kld_chunk the driver's schedule: a check after every
    kld_chunk-th step, SelfPlayEngine.search()'s ceil(interval / L) by default; Search.check_stop() / Game.check_stop() is the check, goal
    lowering included: a stop sets the search's goal S to what is made and in flight, and the gather that follows starts no descent;
  * the tree is never modified by the option: changing Game.kld_stop between plies keeps the subtree kept for the next ply.

configs() and gain_cases() are the inputs both test modules use; cov counts, on the restatement alone, the conditions the GPU cases must
reach (COVERAGE)."""
import collections
import math
import struct

import numpy as np

import puctref as PR
from composeref import DRAW, LOSS
from forcedref import WIDE_FEN, gammas, position_record, worst_case                # noqa: F401 (re-exported)
from gumbelref import slog
from hashmodel import evaluate_packed

MAX_MOVES = 218
KldStop = collections.namedtuple("KldStop", "min_gain interval min_simulations")   # sz_kld_stop_options


def bits(x):
    """an f64 as its 64 bits; every NaN as one value (the device's is all ones, Python's the quiet NaN)"""
    return -1 if x != x else struct.unpack("<q", struct.pack("<d", float(x)))[0]


def term(prev_c, prev_total, now_c, new_total):
    """sz_kld_term.  Python floats are IEEE f64: every operator one rounding"""
    if int(prev_c) == 0:
        return 0.0
    o = float(int(prev_c)) / float(int(prev_total))
    n = float(int(now_c)) / float(int(new_total))
    return o * slog(o / n)


def terms(prev, now):
    pt, nt = int(np.sum(prev, dtype=np.int64)), int(np.sum(now, dtype=np.int64))
    return [term(p, pt, q, nt) for p, q in zip(prev, now)]


def lane_sum(ts):
    """the project's fixed order: lane l adds t_l, t_{l+64}, ... ascending from 0.0, then the xor butterfly"""
    lanes = np.zeros(64, np.float64)
    for c, t in enumerate(ts):
        lanes[c % 64] = lanes[c % 64] + t                # ascending within a lane: c runs upwards
    off = 32
    while off >= 1:
        lanes = lanes + lanes[np.arange(64) ^ off]
        off >>= 1
    return float(lanes[0])


def gain(prev, now):
    """wave_kld_gain: the summed gain of the K = len(prev) children, before the division by the new visits"""
    return lane_sum(terms(prev, now))


def gain_exact(prev, now):
    """the same quantity by math.log and math.fsum -> (gain, sum of |term|)"""
    pt, nt = int(np.sum(prev, dtype=np.int64)), int(np.sum(now, dtype=np.int64))
    ts = [(int(p) / pt) * math.log((int(p) / pt) / (int(q) / nt)) for p, q in zip(prev, now) if int(p) != 0]
    return math.fsum(ts), math.fsum(abs(t) for t in ts)


def checked(o, num_searches):
    """sz_set_kld_stop's refusals (SZ_ERR_INVALID) -> the KldStop"""
    o = KldStop(float(o.min_gain), int(o.interval), int(o.min_simulations))
    assert math.isfinite(o.min_gain) and 0.0 < o.min_gain <= 1.0, "SZ_ERR_INVALID"
    assert 1 <= o.interval <= num_searches and 0 <= o.min_simulations <= num_searches, "SZ_ERR_INVALID"
    return o


# ---------------------------------------------------------------------------------------------------------------- the search, step by step
class Stepwise:
    """Mixed in front of the class a ply's search has (Game.begin): composeref.Search._run as a sequence of points, "begin" when sz_search_begin
    returns and "step" after every sz_search_step, with the check of sz_search_check_stop after every kld_chunk-th step."""
    kld = None                                           # the KldStop the search runs under, None = off
    kld_chunk = 0

    def kld_reset(self, kld, chunk):
        """sz_search_begin's part: clean stop state"""
        self.kld, self.kld_chunk = kld, int(chunk)
        self.prev, self.prev_total, self.has_prev = None, 0, False
        self.stopped_at, self.checks, self.last_gain = -1, 0, float("nan")
        self.goal0 = int(self.S)                         # sz_search_goals
        self.pending = []
        self.n_steps = 0
        self.kld_log = []                                # per check the board took part in: (steps made, stopped_at, checks, bits(last_gain), tree)
        self.kld_evals = []                              # per evaluated gain: (prev, now, g, stopped)

    def _points(self):
        pending, descent_only = [], self.continued
        if not self.continued:
            root = self.games[0]
            tv, term_ = root.get_value_and_terminated()
            if term_ or self.S <= 0:                     # a terminal root: every simulation re-visits it (mcts.py:104-109)
                S = max(self.S, 0)
                self.W[0], self.N[0], self.sims, self.terminal_hits = float(tv) * S, 1 + S, S, S
                if self.solver and term_:
                    self.R[0] = LOSS if tv == -1 else DRAW
                self.begin_tree, self.begin_proven = self.tree(), self.tree_proven()
                return
            pending = [([0], self._planes(0))]
            self.K[0] = 1                                # the root's own evaluation is in flight
            self.begin_tree, self.begin_proven, self.begin_rows = self.tree(), self.tree_proven(), 1
            self.pending = pending
            yield "begin"
        while pending or descent_only:
            if pending:                                  # the network call of this step, then expand + back up in gather order
                self.steps.append(np.stack([p for _, p in pending]))
                for path, planes in pending:
                    pol, val = evaluate_packed(planes, self.mode, self.salt)
                    self._expand(path[-1], pol)
                    self.K[path] -= 1
                    self._backprop(path, float(val))
                    self.expansions += 1
                    self.sum_depth += len(path) - 1
            stepped = bool(pending)
            pending = self.pending = self._gather()
            if descent_only:                             # sz_search_begin's descent-only launch
                descent_only = False
                self.begin_tree, self.begin_proven, self.begin_rows = self.tree(), self.tree_proven(), len(pending)
                if len(pending) > 1:
                    self.cov["continued_gathers_several"] += 1
                if not pending and self.solver and self.R[0]:
                    self.cov["kept_root_proven_done_at_begin"] += 1
                yield "begin"
            elif stepped:
                self.n_steps += 1
                yield "step"

    def _run(self):
        for point in self._points():
            if point == "step" and self.kld is not None and self.kld_chunk and self.n_steps % self.kld_chunk == 0:
                self.check_stop()

    def check_stop(self):
        """sz_search_check_stop for this board"""
        kld = self.kld
        if kld is None or not self.pending or self.stopped_at >= 0:      # off; done (a gather that leaves nothing in flight ran out of goal); stopped
            return False
        K = int(self.n[0])
        if K == 0:
            return False
        f = int(self.first[0])
        now = self.N[f:f + K].astype(np.int64).copy()
        new_total = int(now.sum())
        stop = False
        if new_total < self.prev_total + kld.interval:
            self.cov["kld_check_skipped_below_interval"] += 1
        else:
            if self.has_prev and self.prev_total > 0:
                g = gain(self.prev, now) / float(new_total - self.prev_total)
                self.last_gain, self.checks = g, self.checks + 1
                below = g < kld.min_gain
                stop = below and self.sims >= kld.min_simulations
                self.cov["kld_stop_withheld_by_min_simulations"] += below and not stop
                self.kld_evals.append((self.prev.copy(), now.copy(), g, stop))
            if stop:
                s = self.sims + len(self.pending)
                self.stopped_at = self.S = s             # the goal: the gather that follows starts no descent
                self.cov["kld_stop_at_second_check" if self.checks == 1 else "kld_stop_at_later_check"] += 1
                self.cov["kld_stop_with_several_in_flight"] += self.L > 1 and len(self.pending) >= 2
                self.cov["kld_stop_on_continued_search"] += bool(self.continued) and self.n_kept > 1
                self.cov["kld_stop_below_num_searches_goal"] += self.goal0 < self.cap
            else:
                self.prev, self.prev_total, self.has_prev = now, new_total, True
        self.kld_log.append((self.n_steps, self.stopped_at, self.checks, bits(self.last_gain), self.tree()))
        return stop


_classes = {}


def stepwise(cls):
    if cls not in _classes:
        _classes[cls] = type("Stepwise" + cls.__name__, (Stepwise, cls), {})
    return _classes[cls]


class Game(PR.Game):
    """puctref.Game with the option as a setting of the board: g.kld_stop = KldStop(...) or None between plies is sz_set_kld_stop; g.kld_chunk
    the steps between two checks (None: ceil(interval / L), SelfPlayEngine.search()'s)"""

    def __init__(self, *a, kld_stop=None, kld_chunk=None, **kw):
        super().__init__(*a, **kw)
        self.kld_stop, self.kld_chunk = kld_stop, kld_chunk
        self.kld_plies = []                              # per ply: the setting the search ran with
        self.kld_stats = [0, 0, 0]                       # sz_kld_stop_stats of this board: stopped early, checks evaluated, simulations not made

    def begin(self, target=None, gamma=None, quiet=False, forced_k=0.0):
        s = super().begin(target, gamma, quiet, forced_k)
        ks = None if self.kld_stop is None else checked(self.kld_stop, s.cap)
        self.kld_plies.append(ks)
        s.__class__ = stepwise(s.__class__)
        s.kld_reset(ks, 0 if ks is None else (self.kld_chunk or -(-ks.interval // s.L)))
        return s

    def check_stop(self):
        return self.search.check_stop()

    def run(self):
        s = super().run()
        if s.kld is not None:
            self.kld_stats[1] += s.checks
            if s.stopped_at >= 0:
                self.kld_stats[0] += 1
                self.kld_stats[2] += s.goal0 - s.stopped_at
            else:
                self.cov["kld_ran_whole_goal"] += s.goal0 > 0 and s.sims == s.goal0 and s.has_prev
                self.cov["kld_proven_root_done_before_any_check"] += bool(s.solver and s.R[0]) and not s.has_prev and s.checks == 0
        return s


# ---------------------------------------------------------------------------------------------------------------- the engine configurations
Config = collections.namedtuple("Config", "name S plies boards L solver reuse forced_k endings fpu noise targets budgets cpuct learning kld")
# one engine each; targets: per ply per board the visit target (a reuse engine) or None; budgets: per ply per board (an engine without reuse) or
# None; kld: the KldStop of every ply
Board = PR.Board
MATE_IN_1_FEN = "k7/2P5/1K6/8/8/8/8/8 w - - 0 1"            # nine legal moves, c8=Q and c8=R mate: the solver proves the root within a few visits
ENDINGS = dict(resign_value=-0.9, resign_patience=3, resign_min_ply=2, draw_value=0.0, draw_patience=0, draw_min_ply=0, proven=0)


def _boards(names):
    import sigma_zero_amd as sz
    start = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    greedy = lambda ply: -1.0
    all_ = {"wide": Board("moves_218/rational/sampled", lambda: sz.ChessTensor(fen=WIDE_FEN), "rational", 1, PR._u(3)),
            "mate1": Board("mate_in_1/rational/greedy", lambda: sz.ChessTensor(fen=MATE_IN_1_FEN), "rational", 2, greedy),
            "sp518": Board("sp518/rational/greedy", start(518), "rational", 518, greedy),
            "sp77": Board("sp77/peaked/greedy", start(77), "peaked", 77, greedy),
            "sp333": Board("sp333/peaked/sampled", start(333), "peaked", 333, PR._u(333)),
            "sp0": Board("sp0/dyadic/greedy", start(0), "dyadic", 0, greedy),
            "sp400": Board("sp400/rational/sampled", start(400), "rational", 400, PR._u(400)),
            "sp959": Board("sp959/dyadic/sampled", start(959), "dyadic", 959, PR._u(959))}
    return [all_[n] for n in names]


def configs():
    import fpuref as FP
    out = [
        Config("plain", 48, 3, _boards(["wide", "sp518", "sp77", "sp333", "sp0", "sp959"]), 1, False, False, 0.0, None, None, False, None, None, None, True,
               KldStop(GAINS["plain"], 6, 0)),
        # combine_options: leaf batching, the solver and reuse_subtree in one search; interval 8 at L = 4 is a check every second step
        Config("L4_solver_reuse", 48, 4, _boards(["sp518", "sp77", "sp0", "sp333", "mate1", "sp400"]), 4, True, True, 0.0, None, None, False, None, None, None, False,
               KldStop(GAINS["L4_solver_reuse"], 8, 0)),
        Config("forced_fpu_endings_noise_cpuct", 48, 3, _boards(["wide", "sp518", "sp77", "sp959"]), 1, False, False, 2.0, ENDINGS, FP.CONFIGS["red_tree_abs1_root"], True,
               None, None, PR.B_, True, KldStop(GAINS["forced_fpu_endings_noise_cpuct"], 6, 30)),
        # visit targets as a playout cap sets them: full and fast plies by board and ply
        Config("visit_targets", 48, 4, _boards(["sp518", "sp77", "sp0", "sp400"]), 1, False, True, 0.0, None, None, False,
               [[48, 48, 48, 48], [16, 48, 48, 48], [48, 16, 48, 48], [48, 48, 16, 48]], None, None, True, KldStop(GAINS["visit_targets"], 4, 0)),
        Config("budgets", 64, 3, _boards(["sp518", "sp77", "sp0", "sp333", "sp959"]), 1, False, False, 0.0, None, None, False, None,
               [[64, 40, 64, 24, 64], [40, 64, 24, 64, 8], [64, 64, 40, 40, 24]], None, True, KldStop(GAINS["budgets"], 8, 16)),
    ]
    assert all(4 <= len(c.boards) <= 8 and 32 <= c.S <= 64 and 4 <= c.kld.interval <= 8 and c.plies >= 3 for c in out)
    return out


def all_configs():
    """configs() and the one more the invariant is tested on: visit targets under leaf batching (interval 8 at L = 4: a check every second step)"""
    vt = next(c for c in configs() if c.name == "visit_targets")
    return configs() + [vt._replace(name="visit_targets_L4", L=4, kld=KldStop(GAINS["visit_targets_L4"], 8, 0))]


# min_gain per configuration, chosen on the gains the configurations form (tests/test_kld_ref.py prints them) so that every outcome of COVERAGE
# occurs and no gain of any check lies within a relative 1e-9 of it, which that test asserts with math.fsum / math.log
GAINS = {"plain": 7e-3, "L4_solver_reuse": 4e-3, "forced_fpu_endings_noise_cpuct": 2e-2, "visit_targets": 7e-3, "budgets": 6e-3, "visit_targets_L4": 7e-3}


def engine_args(cfg):
    """the args of the SelfPlayEngine of a configuration; the option itself is set through set_kld_stop, ply by ply"""
    args = {"C": 2, "num_searches": cfg.S}
    if cfg.L != 1 or cfg.solver:
        args.update(combine_options=True, leaves_per_step=cfg.L, virtual_loss=1.0, solver=cfg.solver)
    if cfg.reuse:
        args["reuse_subtree"] = True
    if cfg.fpu is not None:
        args["fpu"] = PR.FU.fpu_args(cfg.fpu)
    return args


def new_game(cfg, b, kld="config", chunk=None):
    bd = cfg.boards[b]
    g = Game(bd.make(), cfg.S, worst_case(cfg.S) if cfg.reuse else None, reuse=cfg.reuse, L=cfg.L, lam=1.0, solver=cfg.solver, c=2.0, learning=cfg.learning,
             mode=bd.mode, salt=bd.salt, fpu=cfg.fpu, cpuct=cfg.cpuct, kld_stop=cfg.kld if kld == "config" else kld, kld_chunk=chunk)
    if cfg.endings is not None:
        g.set_endings(PR.FU.ER.options(**cfg.endings), False)
    return g


def goal_of(cfg, ply, b):
    """the board's target or budget of a ply, None = neither is set"""
    if cfg.targets is not None:
        return cfg.targets[ply][b]
    return None if cfg.budgets is None else cfg.budgets[ply][b]


def begin_ply(cfg, g, b, ply, gam):
    """the setter calls and sz_search_begin of one ply on one board"""
    g.set_root_noise(cfg.noise)
    return g.begin(goal_of(cfg, ply, b), gam[ply][b] if cfg.noise else None, False, cfg.forced_k)


def play(cfg, kld="config", plies=None, goals=None):
    """the restatement alone: every board of the configuration through its plies -> ([Game], per ply per board the record or None).
    goals: per ply per board a target / budget in the configuration's place"""
    games, gam = [new_game(cfg, b, kld) for b in range(len(cfg.boards))], gammas(cfg) if cfg.noise else None
    recs = []
    for ply in range(cfg.plies if plies is None else plies):
        row = []
        for b, (g, bd) in enumerate(zip(games, cfg.boards)):
            if not g.live:
                row.append(None)
                continue
            if goals is not None:
                g.set_root_noise(cfg.noise)
                g.begin(goals[ply][b], gam[ply][b] if cfg.noise else None, False, cfg.forced_k)
            else:
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


# a board stops at its second evaluated check, the earliest possible; at a later one; runs its whole goal; a check is skipped because fewer than
# `interval` visits were gained; a stop is withheld by min_simulations; a stop with two or more leaves in flight; a stop on a continued search
# whose kept root carried its visits into the first snapshot; a stop on a board whose goal was below num_searches; a board done by a proven
# root before any check
COVERAGE = ("kld_stop_at_second_check", "kld_stop_at_later_check", "kld_ran_whole_goal", "kld_check_skipped_below_interval",
            "kld_stop_withheld_by_min_simulations", "kld_stop_with_several_in_flight", "kld_stop_on_continued_search",
            "kld_stop_below_num_searches_goal", "kld_proven_root_done_before_any_check")


def assert_coverage(cov, names=COVERAGE):
    missing = [k for k in names if cov[k] < 1]
    assert not missing, "conditions not reached: %s of %s" % (missing, {k: cov[k] for k in COVERAGE})


# ---------------------------------------------------------------------------------------------------------------- sz_debug_kld_gain cases
GainCases = collections.namedtuple("GainCases", "prev now n_child")       # [n, MAX_MOVES] int32 each (zeros beyond n_child), [n] int32
WIDTHS = (1, 2, 63, 64, 65, 128, 218)


def gain_cases(n_random=19400, seed=53):
    """Cases for sz_debug_kld_gain, the stand-alone host program and the accuracy test: every width of WIDTHS and seeded ones; snapshots with
    children at 0 visits; now == prev (every term exactly 0); one visit more at totals up to 1e5; searches' worth of new visits"""
    rng = np.random.default_rng(seed)
    rows = []

    def add(prev, more):
        prev, more = np.asarray(prev, np.int64), np.asarray(more, np.int64)
        if prev.sum() > 0:
            rows.append((prev, prev + more))

    for K in WIDTHS:
        for total in (1, 7, 100, 801, 10 ** 5):
            base = rng.multinomial(total, rng.dirichlet(np.full(K, 0.3)))
            zero = np.zeros(K, np.int64)
            add(base, zero)                                            # now == prev
            for _ in range(4):                                         # a single visit, to a visited and to any child
                one = zero.copy()
                one[rng.integers(K)] = 1
                add(base, one)
            add(base, rng.multinomial(max(1, total // 4), rng.dirichlet(np.full(K, 0.3))))
            add(base + 1, rng.multinomial(100, np.full(K, 1.0 / K)))   # no child at 0
    widths = np.concatenate([rng.integers(1, 40, size=n_random * 9 // 10), rng.integers(40, MAX_MOVES + 1, size=n_random - n_random * 9 // 10)])
    for K in widths:
        K = int(K)
        total = int(2.0 ** rng.uniform(0.0, 16.6))
        alpha = float(rng.choice([0.05, 0.3, 1.0, 10.0]))
        base = rng.multinomial(total, rng.dirichlet(np.full(K, alpha)))
        new = int(rng.choice([1, 1, 4, 8, 100, max(1, total // 2)]))
        add(base, rng.multinomial(new, rng.dirichlet(np.full(K, alpha))))
    n = len(rows)
    prev, now, nc = np.zeros((n, MAX_MOVES), np.int32), np.zeros((n, MAX_MOVES), np.int32), np.zeros(n, np.int32)
    for i, (p, q) in enumerate(rows):
        prev[i, :len(p)], now[i, :len(p)], nc[i] = p, q, len(p)
    return GainCases(prev, now, nc)


def gain_reference(gc):
    """the restatement's answers to the cases -> gain f64 [n]"""
    return np.array([gain(gc.prev[i, :k], gc.now[i, :k]) for i, k in enumerate(gc.n_child)], np.float64)
