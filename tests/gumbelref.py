"""Plain-Python restatement of the Gumbel root search (sz_set_gumbel / sz_fetch_gumbel / sz_gumbel_stats / sz_debug_gumbel, args["gumbel"], a
NON-REFERENCE option; include/sigmazero.h is the specification).  It is what wave_select_root_gumbel (the depth-0 selection of
k_search_step<false, false, GumbelOpts[, FpuOpts]>), wave_gumbel_play (k_play<false, GumbelOpts>) and csrc/sz_gumbel.h (sz_slog, sz_sexp,
sz_gumbel_level) are held to, bit for bit (tests/test_gpu_gumbel.py).  Built on fpuref (Search / Game), which stays as it is:

  * slog() and sexp() repeat csrc/sz_gumbel.h operator for operator on Python floats (IEEE f64, one rounding per operator);
  * level() is the literal phase loop that builds the whole schedule of a search; the device's closed walk is held to it;
  * select_root(), final_move() and improved_policy() are the three rules on plain arrays; Search._descend uses the first at the root (below
    it fpuref's selection with the tree's setting, or composeref's), Game.play the other two, and hook_reference() all three;
  * Game.gumbel is sz_set_gumbel for this board (a Gumbel, or None = off); begin(budget, g) is sz_search_begin and takes it up for the search.

Accuracy of slog / sexp against math.log / math.exp, measured by tests/test_gumbel_ref.py on the CPU (every f32 power of two, 10^5 seeded f32
priors with denormals, a grid of 20001 y over [-700, 0]): largest relative error MEASURED_REL_ERR = 3.66e-16 (slog 3.654e-16, sexp 2.176e-16);
the test bound is four times
that (platform libm differences in the comparison value), far below the 2^-40 the rule needs.

scenarios() and hook_cases() are the inputs both test modules use; cov counts, on the restatement alone, the conditions the GPU cases must
reach (COVERAGE, HOOK_COVERAGE, assert_coverage)."""
import collections
import functools
import math
import struct

import numpy as np

import fpuref as FP
from fpuref import MAX_MOVES, WIDE_FEN, position_record      # noqa: F401 (re-exported)
from hashmodel import evaluate_packed
from vlref import F32, ucb

F64 = np.float64
Gumbel = collections.namedtuple("Gumbel", "m c_visit c_scale")       # sz_gumbel_options: max_considered, c_visit, c_scale
MEASURED_REL_ERR = 3.66e-16
REL_ERR_BOUND = 4 * MEASURED_REL_ERR

SQRT2 = 1.4142135623730951
LN2 = 0.6931471805599453
INV_LN2 = 1.4426950408889634
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
EXP_CUTOFF = -700.0


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _f64(u):
    return struct.unpack("<d", struct.pack("<Q", u & 0xFFFFFFFFFFFFFFFF))[0]


def slog(x):
    """sz_slog: x > 0 a normal f64"""
    u = _bits(float(x))
    e = ((u >> 52) & 0x7FF) - 1023
    m = _f64((u & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000)
    if m >= SQRT2:
        m = m * 0.5
        e = e + 1
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    p = 1.0 / 19.0
    p = p * s2 + 1.0 / 17.0
    p = p * s2 + 1.0 / 15.0
    p = p * s2 + 1.0 / 13.0
    p = p * s2 + 1.0 / 11.0
    p = p * s2 + 1.0 / 9.0
    p = p * s2 + 1.0 / 7.0
    p = p * s2 + 1.0 / 5.0
    p = p * s2 + 1.0 / 3.0
    p = p * s2 + 1.0
    return (2.0 * s) * p + float(e) * LN2


def sexp(y):
    """sz_sexp: y <= 0; 0 below the cutoff"""
    y = float(y)
    if not (y >= EXP_CUTOFF):
        return 0.0
    k = float(math.floor(y * INV_LN2 + 0.5))
    r = (y - k * LN2_HI) - k * LN2_LO
    p = 1.0 / 6227020800.0
    p = p * r + 1.0 / 479001600.0
    p = p * r + 1.0 / 39916800.0
    p = p * r + 1.0 / 3628800.0
    p = p * r + 1.0 / 362880.0
    p = p * r + 1.0 / 40320.0
    p = p * r + 1.0 / 5040.0
    p = p * r + 1.0 / 720.0
    p = p * r + 1.0 / 120.0
    p = p * r + 1.0 / 24.0
    p = p * r + 1.0 / 6.0
    p = p * r + 1.0 / 2.0
    p = p * r + 1.0
    p = p * r + 1.0
    return _f64(_bits(p) + (int(k) << 52))


# ---------------------------------------------------------------------------------------------------------------- the schedule
@functools.lru_cache(maxsize=None)
def schedule(n, m_eff):
    """the levels of the n root-child visits of a search, by the literal phase loop -> (tuple of levels, info)"""
    L = max(1, int(math.ceil(math.log2(m_eff)))) if m_eff > 1 else 1
    assert 2 ** L >= m_eff and (L == 1 or 2 ** (L - 1) < m_eff)
    seq, level, c = [], 0, m_eff
    info = collections.Counter()
    phases_at_2 = 0
    while len(seq) < n:
        r = max(1, n // (L * c))
        phases_at_2 += c == 2 and m_eff > 2
        for _ in range(r):
            if len(seq) == n:
                break
            for j in range(c):
                if len(seq) == n:
                    info["cut_mid_round"] += 1       # the last phase ends inside a round
                    break
                seq.append(level)
            level += 1
        c = max(2, c // 2)
    info["c_stays_2"] += phases_at_2 >= 2
    info["ends_in_level_0"] += n < m_eff
    return tuple(seq), info


def level(t, n, m_eff):
    return schedule(int(n), int(m_eff))[0][t]


# ---------------------------------------------------------------------------------------------------------------- the three rules
def _q(W, N):
    return 0.5 - 0.5 * (float(W) / float(int(N)))


def _sigma_factor(opts, maxN):
    return (float(F32(opts.c_visit)) + float(int(maxN))) * float(F32(opts.c_scale))


def logits(P):
    return [slog(float(F32(p))) for p in P]


def scores(N, W, g, lg, sf):
    """s_c = (g_c + logit_c) + sigma(q_c), the sigma term 0.0 at N_c = 0"""
    out = []
    for c in range(len(N)):
        gl = (0.0 if g is None else float(g[c])) + lg[c]
        out.append(gl + (sf * _q(W[c], N[c]) if N[c] >= 1 else 0.0))
    return out


def _first_max(s, idx):
    bi, best = -1, 0.0
    for c in idx:                                        # wave_select_child's loop: first maximum
        if bi < 0 or s[c] > best:
            bi, best = c, s[c]
    return bi


def select_root(N, W, P, g, t, goal, opts, lg=None):
    """the root selection at root-child visit t of a search of `goal` simulations -> (child, fallback, info)"""
    K = len(N)
    m_eff = min(int(opts.m), K)
    lv = level(t, goal - 1, m_eff)
    lg = logits(P) if lg is None else lg
    s = scores(N, W, g, lg, _sigma_factor(opts, max(int(x) for x in N)))
    idx = [c for c in range(K) if int(N[c]) == lv]
    info = collections.Counter()
    fallback = not idx
    if fallback:
        idx = list(range(K))
    i = _first_max(s, idx)
    info["tie_by_index"] += g is None and sum(1 for c in idx if s[c] == s[i]) >= 2
    info["wide_root"] += K > 64
    return i, fallback, info


def final_move(N, W, P, g, opts, lg=None):
    """sz_play's move: the best child among the most visited"""
    maxN = max(int(x) for x in N)
    lg = logits(P) if lg is None else lg
    s = scores(N, W, g, lg, _sigma_factor(opts, maxN))
    return _first_max(s, [c for c in range(len(N)) if int(N[c]) == maxN])


def improved_policy(N, W, P, vhat, opts, lg=None):
    """the completed-Q improved policy -> (pi f32 [K], v_mix f64, info)"""
    K = len(N)
    lg = logits(P) if lg is None else lg
    sf = _sigma_factor(opts, max(int(x) for x in N))
    v01 = 0.5 + 0.5 * float(F32(vhat))
    sumN, pq, pm = 0, 0.0, 0.0
    for c in range(K):
        sumN += int(N[c])
        if N[c] >= 1:
            pq = pq + float(F32(P[c])) * _q(W[c], N[c])
            pm = pm + float(F32(P[c]))
    v_mix = v01 if sumN == 0 else (v01 + float(sumN) * (pq / pm)) / (1.0 + float(sumN))
    z = [lg[c] + sf * (_q(W[c], N[c]) if N[c] >= 1 else v_mix) for c in range(K)]
    zmax = max(z)
    e = [sexp(zc - zmax) for zc in z]
    se = 0.0
    for c in range(K):
        se = se + e[c]
    info = collections.Counter()
    info["e_exactly_0"] += any(x == 0.0 for x in e)
    info["denormal_prior"] += any(0.0 < float(F32(p)) < 2.0 ** -126 for p in P)
    return np.array([F32(e[c] / se) for c in range(K)], np.float32), v_mix, info


def checked(gb):
    """sz_set_gumbel's refusals of the options (SZ_ERR_INVALID) -> the Gumbel with f32 constants"""
    gb = Gumbel(int(gb[0]), float(np.float32(gb[1])), float(np.float32(gb[2])))
    assert 1 <= gb.m <= MAX_MOVES and math.isfinite(gb.c_visit) and gb.c_visit >= 0.0 and math.isfinite(gb.c_scale) and gb.c_scale >= 0.0, "SZ_ERR_INVALID"
    return gb


# ---------------------------------------------------------------------------------------------------------------- Search / Game
class Search(FP.Search):
    """fpuref.Search whose selection at the root is select_root().  Game.begin() turns the ply's search into one."""
    gumbel = None
    g = None
    vhat = F32(0.0)
    gumbel_selections = gumbel_fallbacks = 0
    _lg = None
    step_trees = None                                    # tree() after every search step (an expansion and the descents that follow it)

    def _gather(self):
        pending = super()._gather()
        if self.gumbel is not None:
            if self.step_trees is None:
                self.step_trees = []
            self.step_trees.append(self.tree())
        return pending

    def _descend(self):
        if self.gumbel is None:
            return super()._descend()
        path, e = [0], 0
        if self.n[0] > 0:
            f, k = int(self.first[0]), int(self.n[0])
            if self._lg is None:
                self._lg = logits(self.P[f:f + k])           # cached per search: the priors of a root do not change
            i, fb, info = select_root(self.N[f:f + k], self.W[f:f + k], self.P[f:f + k], self.g, self.sims - 1, self.S, self.gumbel, self._lg)
            self.cov.update(info)
            self.gumbel_selections += 1
            self.gumbel_fallbacks += fb
            e = f + i
            path.append(e)
            self.cov["terminal_child_considered"] += bool(self.term[e])
        while self.n[e] > 0:                                  # below the root nothing changes
            f, k = int(self.first[e]), int(self.n[e])
            zero = np.zeros(k, np.int64)
            if self.fpu is not None:
                i, _, _ = FP.select(self.N[f:f + k], zero, self.W[f:f + k], self.P[f:f + k], None, int(self.N[e]), int(self.N[e]), self.W[e], self.c, self.lam, False, self.fpu)
            else:
                i = int(np.argmax(ucb(self.N[f:f + k], self.W[f:f + k], self.P[f:f + k], F32(math.sqrt(float(self.N[e]))), self.c)))
            e = f + i
            path.append(e)
        return path


class Game(FP.Game):
    """fpuref.Game with the option as a setting of the board: g.gumbel = Gumbel(...) or None between plies is sz_set_gumbel"""

    def __init__(self, *a, gumbel=None, **kw):
        super().__init__(*a, **kw)
        self.gumbel = gumbel
        self.gumbel_plies = []
        self.gumbel_selections = self.gumbel_fallbacks = 0

    def begin(self, budget=None, g=None):
        s = super().begin(budget)
        gb = None if self.gumbel is None else checked(self.gumbel)
        self.gumbel_plies.append(gb)
        if gb is not None:
            assert not self.reuse and s.L == 1 and not s.solver, "SZ_ERR_INVALID"
            fp = getattr(s, "fpu", None)
            s.__class__ = Search
            s.fpu, s.gumbel, s.g = fp, gb, (None if g is None else np.asarray(g, np.float64))
            root = s.games[0]
            term = root.get_value_and_terminated()[1]
            self.cov["terminal_root"] += bool(term)
            self.cov["goal_1"] += s.S == 1 and not term
            self.cov["goal_2"] += s.S == 2 and not term
            if not term and s.S > 0:
                s.vhat = F32(evaluate_packed(s._planes(0), s.mode, s.salt)[1])      # the value sz_search_step reads when it expands the root
                k = len(root.legal_action_indices())
                self.cov["K_lt_m"] += k < gb.m
                self.cov["m_1"] += gb.m == 1
                if s.S >= 2:
                    self.cov.update(schedule(s.S - 1, min(gb.m, k))[1])      # k: before zero priors are dropped; exact for the coverage's purpose
        return s

    def run(self):
        s = super().run()
        self.gumbel_selections += getattr(s, "gumbel_selections", 0)
        self.gumbel_fallbacks += getattr(s, "gumbel_fallbacks", 0)
        return s

    def play(self, u):
        s = self.search
        if getattr(s, "gumbel", None) is None:
            return super().play(u)
        acts, vis = s.root_children()
        k = len(acts)
        assert k > 0 and vis.sum() > 0, "SZ_ERR_ZERO_VISITS"
        f = int(s.first[0])
        W, P = s.W[f:f + k], s.P[f:f + k]
        lg = logits(P)
        i = final_move(vis, W, P, s.g, s.gumbel, lg)
        pi, v_mix, info = improved_policy(vis, W, P, s.vhat, s.gumbel, lg)
        self.cov.update(info)
        s.choose = lambda _u, i=i: i                         # the board's uniform is not read
        rec = super().play(u)
        rec["policy"] = np.zeros(MAX_MOVES, np.float32)
        rec["policy"][:k] = pi
        rec["v_mix"], rec["root_value"] = v_mix, F32(s.vhat)
        return rec


# ---------------------------------------------------------------------------------------------------------------- scenarios
Scenario = collections.namedtuple("Scenario", "name S learning plies boards gumbel fpu seeded compact")
# gumbel: the Gumbel every ply runs with; fpu: an fpuref.Fpu or None; seeded: g drawn from a seeded generator, else g = NULL; compact: the
# engine runs with sz_compact and shrinks the batch during the search (sz_compact_searching)
Board = collections.namedtuple("Board", "name make mode salt budgets")

MATE_IN_1_FEN = "kbK5/p7/1P6/8/8/8/8/8 w - - 0 1"         # four legal moves, b7 mates: K < m and a terminal child among the considered
MATED_FEN = "7k/6Q1/6K1/8/8/8/8/8 b - - 0 1"              # a terminal root
BUDGETS = (1, 2, 3, 9, 33, 64)


def _boards():
    import sigma_zero_amd as sz
    start = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    fen = lambda f: (lambda: sz.ChessTensor(fen=f))
    return [Board("sp518", start(518), "dyadic", 518, [64, 33, 9]),
            Board("sp0", start(0), "dyadic", 0, [33, 64, 2]),
            Board("sp77/peaked", start(77), "peaked", 77, [9, 3, 64]),
            Board("sp959/rational", start(959), "rational", 959, [3, 9, 33]),
            Board("moves_218", fen(WIDE_FEN), "dyadic", 1, [64, 2, 1]),
            Board("mate_in_1", fen(MATE_IN_1_FEN), "dyadic", 3, [33, 64, 3]),
            Board("mated", fen(MATED_FEN), "dyadic", 4, [64, 64, 64]),
            Board("sp333", start(333), "dyadic", 333, [2, 64, 1])]


def scenarios():
    bs = _boards()
    assert len(bs) == 8 and {x for b in bs for x in b.budgets} == set(BUDGETS)
    tree_fpu = FP.Fpu(FP.REDUCTION, 0.33, FP.ABSOLUTE, 1.0)            # the root's setting is not consulted
    return [Scenario("m16_seeded", 64, True, 3, bs, Gumbel(16, 50.0, 1.0), None, True, False),
            Scenario("m4_seeded_fpu", 64, True, 3, bs, Gumbel(4, 50.0, 1.0), tree_fpu, True, False),
            Scenario("m2_null", 64, False, 3, bs, Gumbel(2, 50.0, 1.0), None, False, False),
            Scenario("m1_null_fpu", 64, False, 3, bs, Gumbel(1, 50.0, 1.0), tree_fpu, False, False),
            Scenario("m16_null_scale100", 64, False, 3, bs, Gumbel(16, 50.0, 100.0), None, False, False),
            Scenario("m16_seeded_compact", 64, True, 3, bs, Gumbel(16, 50.0, 1.0), None, True, True)]


def gumbels(sc):
    """the Gumbel(0,1) draws of a scenario, [plies][boards][218] f64 from a seeded generator (g = -log(-log(u))), or None"""
    if not sc.seeded:
        return None
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(sc.name))
    u = np.random.default_rng(seed).random(size=(sc.plies, len(sc.boards), MAX_MOVES))
    return -np.log(-np.log(u))


def new_game(sc, bd, gumbel="scenario"):
    return Game(bd.make(), sc.S, None, reuse=False, L=1, lam=1.0, solver=False, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt, fpu=sc.fpu,
                gumbel=sc.gumbel if gumbel == "scenario" else gumbel)


def play(sc, gumbel="scenario"):
    """the restatement alone: every board of the scenario through its plies; a board that has nothing to play (zero visits) ends in an error"""
    games, gs = [new_game(sc, bd, gumbel) for bd in sc.boards], gumbels(sc)
    for ply in range(sc.plies):
        for b, (g, bd) in enumerate(zip(games, sc.boards)):
            if g.live:
                g.begin(bd.budgets[ply], None if gs is None else gs[ply][b])
                g.run()
                play_or_flag(g, 0.5)
    return games


def play_or_flag(g, u):
    """sz_play on one board: the record, or None and the board's error when the root has no visited child (SZ_ERR_ZERO_VISITS)"""
    acts, vis = g.search.root_children()
    if len(acts) == 0 or vis.sum() == 0:
        g.error = "zero_visits"
        return None
    return g.play(u)


def coverage(played, hook=None):
    c = collections.Counter(hook or {})
    for games in played:
        for g in games:
            c.update(g.cov)
            c["selections"] += g.gumbel_selections
            c["fallbacks"] += g.gumbel_fallbacks
            c["zero_visits"] += g.error == "zero_visits"
    return c


# K < m; the budget ends inside level 0; a last phase cut mid-round; c reaching 2 and staying there; a score tie broken by index; a terminal
# child among the considered; goal 1 (zero visits) and goal 2; a terminal root; m = 1; some e_c exactly 0; a root with more than 64 children
COVERAGE = ("K_lt_m", "ends_in_level_0", "cut_mid_round", "c_stays_2", "tie_by_index", "terminal_child_considered", "goal_1", "goal_2", "terminal_root",
            "m_1", "e_exactly_0", "wide_root", "zero_visits", "selections")
HOOK_COVERAGE = ("tie_by_index", "e_exactly_0", "denormal_prior", "wide_root", "all_unvisited", "hook_fallback")


def assert_coverage(cov, names=COVERAGE):
    missing = [k for k in names if cov[k] < 1]
    assert not missing, "conditions not reached: %s of %s" % (missing, dict(cov))
    assert cov["fallbacks"] == 0, "a fresh root found no child at the level"


# ---------------------------------------------------------------------------------------------------------------- sz_debug_gumbel cases
def powers_of_two_f32():
    return np.array([2.0 ** e for e in range(-149, 128)], np.float64)


def random_priors(n, seed=5):
    """seeded f32 priors as f64: uniform bit patterns of positive finite f32 (all magnitudes, denormals included) and Dirichlet-like values"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(1, 0x7F800000, size=n // 2, dtype=np.uint32)
    a = bits.view(np.float32).astype(np.float64)
    b = rng.random(n - n // 2).astype(np.float32)
    b = b[b > 0].astype(np.float64)
    d = (rng.integers(1, 1 << 23, size=64, dtype=np.uint32)).view(np.float32).astype(np.float64)      # f32 denormals
    return np.concatenate([a, b, d])


def exp_grid(n=20001):
    return np.concatenate([np.linspace(EXP_CUTOFF, 0.0, n), np.array([-0.0, -1e-300, -1e-17, -700.0000001, -1e4])])


def level_cases(n_max=70, m_max=20):
    return np.array([(t, n, m) for n in range(1, n_max + 1) for m in range(1, m_max + 1) for t in range(n)], np.int32)


HookCases = collections.namedtuple("HookCases", "offsets N W P g visit goal vhat opts")
HOOK_K = (1, 2, 63, 64, 65, 128, 218)
HOOK_OPTS = (Gumbel(16, 50.0, 1.0), Gumbel(1, 50.0, 1.0), Gumbel(2, 0.0, 0.1), Gumbel(4, 50.0, 100.0), Gumbel(32, 10.0, 1.0), Gumbel(218, 50.0, 0.0))


def hook_cases(n_cases=500, seed=77):
    """Seeded child sets for sz_debug_gumbel: K of 1, 2, 63, 64, 65, 128, 218 and random widths; visit counts at and around the level of a
    random visit t of a random goal, all children unvisited, no child at the level (the fall-back), equal priors, f32-denormal priors, a
    c_scale that drives some e_c to exactly 0 -> HookCases of flat arrays (g: seeded draws; the tests also run them with g = NULL)"""
    rng = np.random.default_rng(seed)
    Ns, Ws, Ps, Gs, off, visit, goal, vhat, opts = [], [], [], [], [0], [], [], [], []
    for i in range(n_cases):
        k = HOOK_K[i % 10] if i % 10 < len(HOOK_K) else int(rng.integers(2, 219))
        kind = (i // 10) % 6
        ob = HOOK_OPTS[int(rng.integers(0, len(HOOK_OPTS)))]
        gl = int(rng.integers(2, 131))
        t = int(rng.integers(0, gl - 1))
        lv = level(t, gl - 1, min(ob.m, k))
        N = np.maximum(lv + rng.integers(-1, 2, size=k), 0)
        if kind == 0:
            N[:] = 0                                                             # all children unvisited (t = 0 is the matching visit; others fall back)
        if kind == 1:
            N[:] = lv + 1                                                        # no child at the level: the fall-back over all children
        P = rng.dirichlet(np.full(k, 0.3)).astype(np.float32) if k > 1 else np.ones(1, np.float32)
        P = np.maximum(P, np.float32(2.0 ** -140))                               # a prior that is exactly 0 is dropped at expansion
        if kind == 2:
            P[:] = np.float32(1.0 / 256)                                         # equal priors: with g = NULL and equal q the first child wins
        if kind == 3:
            P[rng.random(k) < 0.3] = np.float32(1e-42)                           # denormal in f32
        W = (rng.uniform(-1.0, 1.0, size=k) * N).astype(np.float64)
        if kind == 2:
            W[:] = -0.25 * N
        Ns.append(N); Ws.append(W); Ps.append(P); Gs.append(-np.log(-np.log(rng.random(k))))
        off.append(off[-1] + k); visit.append(t); goal.append(gl); vhat.append(rng.uniform(-1.0, 1.0)); opts.append(ob)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dt)
    o = np.zeros(n_cases, np.dtype([("max_considered", np.int32), ("c_visit", np.float32), ("c_scale", np.float32)]))
    for i, ob in enumerate(opts):
        o[i] = tuple(ob)
    return HookCases(np.array(off, np.int32), cat(Ns, np.int32), cat(Ws, np.float64), cat(Ps, np.float32), cat(Gs, np.float64),
                     np.array(visit, np.int32), np.array(goal, np.int32), np.array(vhat, np.float32), o)


def hook_reference(hc, with_g=True):
    """the restatement's answers to the cases -> (selected, fallback, final, policy f32 flat, v_mix f64, Counter)"""
    n = len(hc.visit)
    sel, fbk, fin = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    pol, vmix, cov = np.zeros(len(hc.N), np.float32), np.zeros(n, np.float64), collections.Counter()
    for i in range(n):
        lo, hi = int(hc.offsets[i]), int(hc.offsets[i + 1])
        ob = Gumbel(*[x.item() for x in hc.opts[i]])
        N, W, P = hc.N[lo:hi], hc.W[lo:hi], hc.P[lo:hi]
        g = hc.g[lo:hi] if with_g else None
        lg = logits(P)
        sel[i], fb, info = select_root(N, W, P, g, int(hc.visit[i]), int(hc.goal[i]), ob, lg)
        fbk[i] = int(fb)
        cov.update(info)
        fin[i] = final_move(N, W, P, g, ob, lg)
        pol[lo:hi], vmix[i], info = improved_policy(N, W, P, hc.vhat[i], ob, lg)
        cov.update(info)
        cov["hook_fallback"] += int(fb)
        cov["all_unvisited"] += not (N >= 1).any()
    return sel, fbk, fin, pol, vmix, cov
