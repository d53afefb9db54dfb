"""Plain-Python restatement of first-play urgency for unvisited children (sz_set_fpu / sz_debug_select_fpu, args["fpu"], a NON-REFERENCE
option; include/sigmazero.h is the specification).  It is what wave_select_child<.., true>, the selection of k_search_step<.., FpuOpts> (the
descent-only launch of sz_search_begin included) in csrc/sz_engine.hip, is held to, bit for bit (tests/test_gpu_fpu.py).  Built on forcedref
(Search / Game), which stays as it is:

  * select() is the rule on plain arrays, the lane-strided sum of the visited children's priors written out; Search._descend uses it at
    every node, after forcedref's forced child at the root of a forced board, and hook_reference() for the cases of sz_debug_select_fpu;
  * Game.fpu is sz_set_fpu for this board (an Fpu, or None = off); begin() is sz_search_begin and takes it up for the whole search.  Only
    _descend is overridden, so leaf batching, the solver, reuse, visit targets, root noise and forced playouts compose as they do in forcedref;
  * the tree is never modified by the option: changing Game.fpu between plies keeps the subtree kept for the next ply.

With Game.fpu None it is forcedref (tests/test_fpu_ref.py pins it); with ABSOLUTE 0 at both sites it builds the same trees as with None.
scenarios() and hook_cases() are the inputs both test modules use; cov counts, on the restatement alone, the conditions the GPU cases must
reach (COVERAGE, assert_coverage)."""
import collections
import math

import numpy as np

import forcedref as FR
from composeref import WIN
from forcedref import FULL, MAX_MOVES, WIDE_FEN, gammas, position_record, worst_case      # noqa: F401 (re-exported)
from vlref import F32, ucb

F64 = np.float64
REFERENCE, ABSOLUTE, REDUCTION = 0, 1, 2                   # SZ_FPU_*
MODE_NAMES = {REFERENCE: "reference", ABSOLUTE: "absolute", REDUCTION: "reduction"}
Fpu = collections.namedtuple("Fpu", "tree_mode tree_value root_mode root_value")


def visited_mass(P, visited):
    """the kernel's sum of the visited children's priors: lane l adds children l, l+64, ... ascending and skips unvisited ones, then the xor
    butterfly of wave_sum_butterfly (targetref.gamma_sum's scheme)"""
    lanes = np.zeros(64, np.float32)
    for c in range(len(P)):
        if visited[c]:
            lanes[c % 64] = lanes[c % 64] + P[c]
    off = 32
    while off >= 1:
        lanes = lanes + lanes[np.arange(64) ^ off]
        off >>= 1
    return lanes[0]


def first_play_q(mode, value, P, visited, N_p, W_p):
    """q0 = (v0 + 1) / 2 of a parent, every operator one f32 rounding -> (q0, clamped: -1 / 0 / +1)"""
    with np.errstate(all="ignore"):
        if mode == ABSOLUTE:
            v0 = F32(value)
        else:
            mass = visited_mass(P, visited)
            vp = F32(F64(W_p)) / (F32(int(N_p)) + F32(1e-6))         # the parent's own stored edge: no in-flight terms
            v0 = vp - (F32(value) * F32(math.sqrt(float(mass))))
        clamped = 0
        if not (v0 >= F32(-1.0)):
            v0, clamped = F32(-1.0), -1
        if v0 > F32(1.0):
            v0, clamped = F32(1.0), 1
        return (v0 + F32(1.0)) / F32(2.0), clamped


def select(N, K, W, P, R, n_p, N_p, W_p, c, lam, is_root, opts):
    """Selection under the option over a parent's children (K: in-flight counts, R: proven codes or None = no solver; n_p = N_p + k_p, what
    selection takes as the parent's count; N_p, W_p: the parent's stored edge).  -> (child, scores f32 of every child, info): info counts
    what the coverage asks about"""
    N, K = np.asarray(N, np.int64), np.asarray(K, np.int64)
    P, c = np.asarray(P, np.float32), F32(c)
    nc = N + K
    visited = nc >= 1
    sq = F32(math.sqrt(float(n_p)))
    with np.errstate(all="ignore"):
        ref = ucb(nc, np.asarray(W, F64) + F64(lam) * K.astype(F64), P, sq, c)        # a visited child, and every child under REFERENCE
    mode, value = (opts.root_mode, opts.root_value) if is_root else (opts.tree_mode, opts.tree_value)
    scores, info = ref, collections.Counter()
    if mode != REFERENCE:
        q0, clamped = first_play_q(mode, value, P, visited, N_p, W_p)
        with np.errstate(all="ignore"):
            first = q0 + ((((F32(1.0) / F32(1)) * sq) * c) * P)
        scores = np.where(visited, ref, first).astype(np.float32)
        info["clamp_low"] += clamped < 0 and not visited.all()
        info["clamp_high"] += clamped > 0 and not visited.all()
        info["wide_unvisited"] += len(N) > 64 and not visited.all()
        info["inflight_only_visited"] += bool(((N == 0) & (K > 0)).any())
    idx = np.arange(len(N))
    if R is not None:
        cand = np.nonzero(np.asarray(R) != WIN)[0]
        if len(cand):                                    # every child WIN: all children, as without the solver
            idx = cand
    i = int(idx[np.argmax(scores[idx])])
    if mode != REFERENCE:
        site = "root" if is_root else "tree"
        info["changed_%s_%s" % (MODE_NAMES[mode], site)] += i != int(idx[np.argmax(ref[idx])])
        info["win_skipped"] += len(idx) < len(N) and R[int(np.argmax(scores))] == WIN
        info["tie_first_maximum"] += int((scores[idx] == scores[i]).sum()) >= 2
    return i, scores, info


class Search(FR.Search):
    """forcedref.Search whose selection is select() at every node.  Game.begin() turns the ply's search into one (a search runs under one
    setting for its whole length), so reroot() and the fresh starts stay targetref's."""
    fpu = None

    def _descend(self):
        if self.fpu is None:
            return super()._descend()
        path, e = [0], 0
        while self.n[e] > 0 and not (self.solver and self.R[e]):
            f, k = int(self.first[e]), int(self.n[e])
            R = self.R[f:f + k] if self.solver else None
            n_p = int(self.N[e] + self.K[e])
            i, _, info = select(self.N[f:f + k], self.K[f:f + k], self.W[f:f + k], self.P[f:f + k], R, n_p, int(self.N[e]), self.W[e], self.c, self.lam, e == 0, self.fpu)
            self.cov.update(info)
            if e == 0 and self.forced_k:                 # the forced child decides first, as without the option
                j, forced, finfo = FR.select_root(self.N[f:f + k], self.K[f:f + k], self.W[f:f + k], self.P[f:f + k], R, n_p, self.c, self.lam, self.forced_k)
                if forced:
                    self.forced_selections += 1
                    self.cov["forced_overruled_fpu"] += j != i
                    i = j
            e = f + i
            path.append(e)
        return path


class Game(FR.Game):
    """forcedref.Game with the option as a setting of the board: g.fpu = Fpu(...) or None between plies is sz_set_fpu"""

    def __init__(self, *a, fpu=None, **kw):
        super().__init__(*a, **kw)
        self.fpu = fpu
        self.fpu_plies = []                              # per ply: the setting the search ran with

    def begin(self, target=None, gamma=None, quiet=False, forced_k=0.0):
        s = super().begin(target, gamma, quiet, forced_k)
        fp = None if self.fpu is None else checked(self.fpu)
        if fp is not None and fp.tree_mode == REFERENCE and fp.root_mode == REFERENCE:
            fp = None                                    # both sites REFERENCE: off, the kernels that run without the option run
        self.fpu_plies.append(fp)
        if fp is not None:
            fk = getattr(s, "forced_k", 0.0)
            s.__class__, s.fpu, s.forced_k = Search, fp, fk
        return s


def checked(fp):
    """sz_set_fpu's refusals (SZ_ERR_INVALID) -> the Fpu with f32 values"""
    fp = Fpu(int(fp[0]), float(np.float32(fp[1])), int(fp[2]), float(np.float32(fp[3])))
    for mode, value in ((fp.tree_mode, fp.tree_value), (fp.root_mode, fp.root_value)):
        assert mode in (REFERENCE, ABSOLUTE, REDUCTION), "SZ_ERR_INVALID"
        if mode == ABSOLUTE:
            assert math.isfinite(value) and -1.0 <= value <= 1.0, "SZ_ERR_INVALID"
        if mode == REDUCTION:
            assert math.isfinite(value) and 0.0 <= value <= 2.0, "SZ_ERR_INVALID"
    return fp


# ---------------------------------------------------------------------------------------------------------------- scenarios
Scenario = collections.namedtuple("Scenario", "name S c960 learning plies boards fpu extras")
# fpu: the Fpu every ply runs with; extras: visit targets + root noise + forced playouts on top (a reuse engine; targets / k per ply)
Board = collections.namedtuple("Board", "name make mode salt u")
Extras = collections.namedtuple("Extras", "targets k")

CONFIGS = {
    "red_tree_abs1_root": Fpu(REDUCTION, 0.33, ABSOLUTE, 1.0),       # lc0's self-play shape: every root move looks won until tried
    "red_both": Fpu(REDUCTION, 1.5, REDUCTION, 0.44),                # a large reduction in the tree: the clamp at -1 fires
    "ref_root_absm1_tree": Fpu(ABSOLUTE, -1.0, REFERENCE, 0.0),      # an untried move below the root counts as lost
}
KQK_FEN = "8/8/8/8/8/2k5/8/K2q4 w - - 0 1"
OPTIONS = [(L, solver, reuse) for L in (1, 4) for solver in (False, True) for reuse in (False, True)]


def _u(b):
    return lambda ply: ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0


def _boards():
    import sigma_zero_amd as sz
    start = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    fen = lambda f: (lambda: sz.ChessTensor(fen=f))
    greedy = lambda ply: -1.0
    return [Board("moves_218/rational/sampled", fen(WIDE_FEN), "rational", 1, _u(3)),
            Board("sp518/rational/greedy", start(518), "rational", 518, greedy),
            Board("sp77/peaked/greedy", start(77), "peaked", 77, greedy),
            Board("sp333/peaked/sampled", start(333), "peaked", 333, _u(333)),
            # king against king and queen, the lone king to move: with the solver most of its moves are soon proven WIN for the other side
            Board("kqk/peaked/greedy", fen(KQK_FEN), "peaked", 2, greedy)]


def scenarios():
    bs = _boards()
    out = [Scenario(name, 48, True, name != "red_both", 3, bs, fp, None) for name, fp in CONFIGS.items()]
    # visit targets + root noise + forced playouts on top of the option, on a reuse engine: the forced child decides before FPU does
    out.append(Scenario("extras", 48, True, True, 3, bs, CONFIGS["red_tree_abs1_root"], Extras([48, 16, 48], [2.0, 2.0, 8.0])))
    assert all(4 <= len(sc.boards) <= 8 and 48 <= sc.S <= 64 and 3 <= sc.plies <= 4 for sc in out)
    return out


def runs():
    """(scenario, L, solver, reuse) of every whole-search comparison"""
    out = [(sc, L, solver, reuse) for sc in scenarios() if sc.extras is None for L, solver, reuse in OPTIONS]
    out += [(sc, 4, True, True) for sc in scenarios() if sc.extras is not None]
    return out


def new_game(sc, bd, L=1, solver=False, reuse=True, fpu="scenario"):
    return Game(bd.make(), sc.S, worst_case(sc.S) if reuse else None, reuse=reuse, L=L, lam=1.0, solver=solver, c=2.0, learning=sc.learning, mode=bd.mode,
                salt=bd.salt, fpu=sc.fpu if fpu == "scenario" else fpu)


def begin_ply(sc, g, b, ply, gam):
    """the setter calls and sz_search_begin of one ply on one board"""
    if sc.extras is None:
        return g.begin()
    g.set_root_noise(True)
    return g.begin(sc.extras.targets[ply], gam[ply][b], False, sc.extras.k[ply])


def play(sc, L=1, solver=False, reuse=True, fpu="scenario"):
    """the restatement alone: every board of the scenario through its plies"""
    games, gam = [new_game(sc, bd, L, solver, reuse, fpu) for bd in sc.boards], gammas(sc) if sc.extras is not None else None
    for ply in range(sc.plies):
        for b, (g, bd) in enumerate(zip(games, sc.boards)):
            if g.live:
                begin_ply(sc, g, b, ply, gam)
                g.run()
                if g.error is None:
                    g.play(bd.u(ply))
    return games


def coverage(played, hook=None):
    """played: [[Game]], hook: the Counter of hook_reference() summed over hook_cases() -> Counter of the conditions of COVERAGE"""
    c = collections.Counter(hook or {})
    for games in played:
        for g in games:
            c.update(g.cov)
    return c


# FPU changed the selected child in every mode and at both sites; a parent with more than 64 children had unvisited ones; the clamp fired;
# an in-flight-only child was treated as visited; a WIN child was skipped under FPU; a forced child overruled an FPU selection
COVERAGE = ("changed_absolute_root", "changed_absolute_tree", "changed_reduction_root", "changed_reduction_tree", "wide_unvisited", "clamp_low",
            "inflight_only_visited", "win_skipped", "forced_overruled_fpu")
HOOK_COVERAGE = COVERAGE[:-1] + ("clamp_high", "tie_first_maximum", "all_unvisited", "all_visited", "all_win")


def assert_coverage(cov, names=COVERAGE):
    missing = [k for k in names if cov[k] < 1]
    assert not missing, "conditions not reached: %s of %s" % (missing, dict(cov))


# ---------------------------------------------------------------------------------------------------------------- sz_debug_select_fpu cases
HookCases = collections.namedtuple("HookCases", "offsets N K W P R parent parent_n parent_w c is_root opts lam")
HOOK_K = (1, 63, 64, 65, 128, 129, 218)
HOOK_OPTS = (Fpu(REDUCTION, 0.33, ABSOLUTE, 1.0), Fpu(ABSOLUTE, -1.0, REDUCTION, 2.0), Fpu(REFERENCE, 0.0, REDUCTION, 0.5), Fpu(REDUCTION, 2.0, REFERENCE, 0.0),
             Fpu(ABSOLUTE, 0.0, ABSOLUTE, 0.25), Fpu(REDUCTION, 1.0, REDUCTION, 0.0))


def hook_cases(n_cases=3000, seed=31, solver=True):
    """Seeded cases for sz_debug_select_fpu: K of 1, 63, 64, 65, 128, 129, 218 and random widths; all children unvisited, all visited, children
    with N = 0 and k > 0, equal scores (equal priors among unvisited children, equal statistics among visited ones), every child proven WIN,
    a parent value and a mass that drive v0 past both ends of [-1, 1], both sites and all three modes -> HookCases of flat arrays"""
    rng = np.random.default_rng(seed + (1000 if solver else 0))
    Ns, Ks, Ws, Ps, Rs, off = [], [], [], [], [], [0]
    parent, parent_n, parent_w, cs, roots, opts = [], [], [], [], [], []
    for i in range(n_cases):
        k = HOOK_K[i % 10] if i % 10 < len(HOOK_K) else int(rng.integers(2, 219))
        kind = (i // 10) % 9
        N = rng.integers(0, 12, size=k) * (rng.random(k) < 0.5)
        K = rng.integers(0, 3, size=k) * (rng.random(k) < 0.2)
        P = rng.dirichlet(np.full(k, 0.3)).astype(np.float32) if k > 1 else np.ones(1, np.float32)
        if kind == 0:
            N[:], K[:] = 0, 0                                                    # all children unvisited
        if kind == 1:
            N[:] = rng.integers(1, 12, size=k)                                   # all children visited
        if kind == 2:
            N[:], K[:] = 0, rng.integers(0, 3, size=k)                           # only in-flight visits: N = 0, k > 0 counts as visited
        if kind == 3:
            P[:] = np.float32(1.0 / 256)                                         # equal priors: the unvisited children tie, the first one wins
            N[:] = np.where(N > 0, 3, 0)
        if kind == 4:
            P[:] = np.float32(2.0) ** -rng.integers(1, 4, size=k)                # a mass far above 1: sqrt(mass) drives v0 below -1 ...
        W = (rng.uniform(-1.0, 1.0, size=k) * N).astype(np.float64)
        if kind == 3:
            W[:] = -0.5 * N                                                      # ... and the visited ones tie too
        n_stored = int(N.sum()) + 1 + int(rng.integers(0, 3))
        w_stored = float(rng.uniform(-1.0, 1.0)) * n_stored
        if kind == 5:
            w_stored = 3.0 * n_stored                                            # ... and vp = 3 above +1 (no search has it: |vp| <= 1 there)
        if kind == 6:
            w_stored = -1.0 * n_stored
        R = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.int8), size=k)
        if kind == 7:
            R[:] = 1                                                             # every child WIN: nothing is skipped
        Ns.append(N); Ks.append(K); Ws.append(W); Ps.append(P); Rs.append(R)
        off.append(off[-1] + k)
        parent.append(n_stored + int(K.sum())); parent_n.append(n_stored); parent_w.append(w_stored)
        cs.append(rng.choice([1.0, 2.0, 4.0])); roots.append(int(rng.integers(0, 2))); opts.append(HOOK_OPTS[int(rng.integers(0, len(HOOK_OPTS)))])
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dt)
    o = np.zeros(n_cases, np.dtype([("tree_mode", np.int32), ("tree_value", np.float32), ("root_mode", np.int32), ("root_value", np.float32)]))
    for i, fp in enumerate(opts):
        o[i] = tuple(fp)
    return HookCases(np.array(off, np.int32), cat(Ns, np.int32), cat(Ks, np.int32), cat(Ws, np.float64), cat(Ps, np.float32),
                     cat(Rs, np.int8) if solver else None, np.array(parent, np.int32), np.array(parent_n, np.int32), np.array(parent_w, np.float64),
                     np.array(cs, np.float32), np.array(roots, np.int32), o, 1.0)


def hook_reference(hc):
    """the restatement's answers to the cases -> (scores f32 flat, selected, Counter)"""
    n = len(hc.parent)
    sel, scores, cov = np.zeros(n, np.int32), np.zeros(len(hc.N), np.float32), collections.Counter()
    for i in range(n):
        lo, hi = int(hc.offsets[i]), int(hc.offsets[i + 1])
        R = None if hc.R is None else hc.R[lo:hi]
        fp = Fpu(*[x.item() for x in hc.opts[i]])
        sel[i], scores[lo:hi], info = select(hc.N[lo:hi], hc.K[lo:hi], hc.W[lo:hi], hc.P[lo:hi], R, int(hc.parent[i]), int(hc.parent_n[i]), hc.parent_w[i],
                                             hc.c[i], hc.lam, bool(hc.is_root[i]), fp)
        cov.update(info)
        mode = fp.root_mode if hc.is_root[i] else fp.tree_mode
        nc = hc.N[lo:hi] + hc.K[lo:hi]
        cov["all_unvisited"] += mode != REFERENCE and not (nc >= 1).any()
        cov["all_visited"] += mode != REFERENCE and bool((nc >= 1).all())
        cov["all_win"] += mode != REFERENCE and R is not None and bool((R == WIN).all())
        cov["site_%s_%s" % ("root" if hc.is_root[i] else "tree", MODE_NAMES[mode])] += 1
    return scores, sel, cov
