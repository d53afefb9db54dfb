"""Plain-Python restatement of forced playouts and policy-target pruning (sz_set_forced_playouts / sz_forced_stats / sz_debug_forced,
args["forced_playouts"], a NON-REFERENCE option; include/sigmazero.h is the specification).  It is what wave_forced_child /
wave_select_root_forced (the depth-0 selection of k_search_step<.., ForcedOpts>, the descent-only launch of sz_search_begin included) and
wave_prune (k_play<.., ForcedOpts>) in csrc/sz_engine.hip are held to, bit for bit (tests/test_gpu_forced_playouts.py).  Built on
targetref (Search / Game), which stays as it is:

  * select_root() and prune() are the two rules on plain arrays; Search._descend uses the first at the root, Game.play the second, and
    hook_reference() both, for the cases of sz_debug_forced;
  * Game.begin(..., forced_k=k) is sz_set_forced_playouts for this board followed by sz_search_begin: k > 0 makes this ply's search a forced
    one (the status bit the kernel latches), 0 leaves it targetref's;
  * Game.play records and samples from the pruned counts; the tree, and the subtree kept for the next ply, keep the counted visits;
  * forced_selections and pruned_visits are cumulative like the engine's counters (sz_forced_stats).

With forced_k = 0 everywhere it is targetref (tests/test_forced_ref.py pins it).  scenarios() and hook_cases() are the inputs both test
modules use; cov counts, on the restatement alone, the conditions the GPU cases must reach (COVERAGE)."""
import collections
import math

import numpy as np

import targetref as TR
from composeref import LOSS, WIN
from hashmodel import pack_planes
from reuseref import choose
from targetref import FULL, MAX_MOVES, WIDE_FEN, gammas, position_record, worst_case      # noqa: F401 (re-exported)
from vlref import F32, ucb

F64 = np.float64


def forced_limit(P, T, fk):
    """sqrt(((double)k * (double)P_c) * (double)T), NaN where the product is negative or NaN"""
    with np.errstate(all="ignore"):
        return np.sqrt((F64(F32(fk)) * np.asarray(P, np.float32).astype(F64)) * F64(T))


def select_root(N, K, W, P, R, n_p, c, lam, fk):
    """The root selection of a forced board over its children's arrays (K: in-flight counts, R: proven codes or None = no solver; n_p =
    N_root + k_root).  -> (child, forced, info): forced = a forced child decided it; info counts what the coverage asks about"""
    N, K = np.asarray(N, np.int64), np.asarray(K, np.int64)
    nc = N + K
    sq = F32(math.sqrt(float(n_p)))
    u = ucb(nc, np.asarray(W, F64) + F64(lam) * K.astype(F64), np.asarray(P, np.float32), sq, F32(c))
    open_ = np.ones(len(N), bool)
    if R is not None:
        cand = np.asarray(R) != WIN
        if cand.any():                                   # every child WIN: all children, as without the solver
            open_ = cand
    idx = np.nonzero(open_)[0]
    puct = int(idx[np.argmax(u[idx])])
    would = (nc >= 1) & (nc.astype(F64) < forced_limit(P, n_p - 1, fk))
    forced = would & open_
    info = collections.Counter()
    info["forced_win_skipped"] += int((would & ~open_).any())
    if not forced.any():
        return puct, False, info
    i = int(np.nonzero(forced)[0][0])
    info["forced_overruled_puct"] += i != puct
    info["several_forced"] += int(forced.sum()) >= 2
    info["forced_in_flight"] += int(K[i]) > 0
    return i, True, info


def prune(N, W, P, n_root, c, fk):
    """Policy-target pruning of a finished search over the root children's arrays -> (pruned counts int64, c*, info)"""
    N = np.asarray(N, np.int64)
    W, P, c = np.asarray(W, F64), np.asarray(P, np.float32), F32(c)
    out = N.copy()
    cs = int(np.argmax(N))                               # the first maximum
    sq = F32(math.sqrt(float(n_root)))
    best = ucb(N[cs:cs + 1], W[cs:cs + 1], P[cs:cs + 1], sq, c)[0]
    lim = forced_limit(P, n_root - 1, fk)
    info = collections.Counter()
    with np.errstate(all="ignore"):
        for i in range(len(N)):
            n = int(N[i])
            if i == cs or n < 1:
                continue
            m = n if lim[i] >= n else (int(math.floor(lim[i])) if lim[i] >= 0.0 else 0)      # NaN: 0
            q = F32(1.0) - ((F32(W[i]) / (F32(n) + F32(1e-6))) + F32(1.0)) / F32(2.0)      # the q term at the counted N_c, W_c
            n1, stopped = n, False
            for _ in range(m):
                cand = n1 - 1
                u = (((F32(1.0) / F32(cand + 1)) * sq) * c) * P[i]
                if q + u < best:
                    n1 = cand
                else:
                    stopped = True
                    break
            info["stopped_at_bound"] += stopped and n1 < n
            info["m_capped_by_n"] += lim[i] >= n
            if n1 < n and n1 <= 1:
                info["last_visit_taken"] += n1 == 1      # the PUCT bound alone would have left this child one visit
                n1 = 0
            info["pruned_to_zero"] += n1 == 0
            info["tied_with_best_later"] += n == int(N[cs])
            out[i] = n1
    return out, cs, info


class Search(TR.Search):
    """targetref.Search whose root selection is select_root() while forced_k > 0.  Game.begin() turns a targetref.Search into one (the class
    is the status bit: a search is forced or not for its whole length), so reroot() and the fresh starts stay targetref's."""
    forced_k = 0.0
    forced_selections = 0
    pruned = None                                        # Game.play: the pruned counts of the root's children

    def _descend(self):
        if not self.forced_k or self.n[0] == 0 or (self.solver and self.R[0]):
            return super()._descend()
        f, k = int(self.first[0]), int(self.n[0])
        i, forced, info = select_root(self.N[f:f + k], self.K[f:f + k], self.W[f:f + k], self.P[f:f + k], self.R[f:f + k] if self.solver else None,
                                      int(self.N[0] + self.K[0]), self.c, self.lam, self.forced_k)
        self.cov.update(info)
        if forced:
            self.forced_selections += 1
            if self.continued and self.begin_tree is None:
                self.cov["forced_on_kept_root_at_begin"] += 1        # sz_search_begin's descent-only launch
        path, e = [0, f + i], f + i
        lam = F64(self.lam)
        while self.n[e] > 0 and not (self.solver and self.R[e]):     # below the root: composeref's descent (its `skips` diagnostic does not see the root step)
            f, k = self.first[e], self.n[e]
            kk = self.K[f:f + k]
            sq = F32(math.sqrt(float(self.N[e] + self.K[e])))
            u = ucb(self.N[f:f + k] + kk, self.W[f:f + k] + lam * kk.astype(F64), self.P[f:f + k], sq, self.c)
            i = int(np.argmax(u))
            if self.solver:
                cand = np.nonzero(self.R[f:f + k] != WIN)[0]
                if len(cand):
                    if self.R[f + i] == WIN:
                        self.skips += 1
                        self.cov["win_child_skipped"] += 1
                    i = int(cand[np.argmax(u[cand])])
            e = f + i
            path.append(e)
        return path

    def choose(self, u):
        if self.pruned is None:
            return super().choose(u)
        r, rc = self.root_proven()
        if self.solver and r == WIN:                     # the solver's WIN-root rule stays on top
            return int(np.nonzero(rc == LOSS)[0][0])
        return choose(self.pruned, u)


class Game(TR.Game):
    """targetref.Game with the forced constant per ply: begin(..., forced_k), and play() on the pruned counts"""
    COUNTERS = TR.Game.COUNTERS

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.forced_selections = self.pruned_visits = 0
        self.forced_plies = []                           # per ply: the constant the search ran with (0.0: not forced)

    def begin(self, target=None, gamma=None, quiet=False, forced_k=0.0):
        s = super().begin(target, gamma, quiet)
        fk = float(np.float32(forced_k))
        assert fk >= 0.0 and math.isfinite(fk) and (fk == 0.0 or s.learning), "SZ_ERR_INVALID"
        self.forced_plies.append(fk)
        if fk > 0.0:
            s.__class__, s.forced_k = Search, fk
        return s

    def run(self):
        s = super().run()
        self.forced_selections += getattr(s, "forced_selections", 0)
        return s

    def play(self, u):
        s = self.search
        if not getattr(s, "forced_k", 0.0):
            return super().play(u)
        acts, vis = s.root_children()
        k = len(acts)
        assert k > 0 and vis.sum() > 0, "SZ_ERR_ZERO_VISITS"     # on the counted visits
        f = int(s.first[0])
        s.pruned, _, info = prune(vis, s.W[f:f + k], s.P[f:f + k], int(s.N[0]), s.c, s.forced_k)
        cut = int((vis - s.pruned).sum())
        self.pruned_visits += cut
        self.cov.update(info)
        self.cov["pruned_on_continued_ply"] += cut > 0 and self.starts[-1] == "reused"
        if s.solver and s.R[0] == WIN:
            self.cov["win_root_played"] += 1
        chosen = int(acts[s.choose(u)])
        rec = dict(packed=pack_planes(self.game.get_representation().numpy()), action=np.full(MAX_MOVES, -1, np.int32),
                   visits=np.zeros(MAX_MOVES, np.int32), n_child=k, colour=int(bool(self.game.board.turn)), chosen=chosen)
        rec["action"][:k], rec["visits"][:k] = acts, s.pruned
        self.chosen.append(chosen)
        self.game.push_action(chosen)
        v, t = self.game.get_value_and_terminated()
        self.over = bool(t)
        self.result = 0 if not (t and v) else (-1 if self.game.board.turn else 1)
        rec["game_over"], rec["result"] = int(self.over), self.result
        if self.reuse:
            nxt = s.reroot(chosen, self.game)            # the counted visits: the kept subtree does not see the pruning
            if self.over:
                self.last_fallback = nxt[1]
            else:
                self.next = nxt
        return rec


# ---------------------------------------------------------------------------------------------------------------- scenarios
Scenario = collections.namedtuple("Scenario", "name S c960 learning edges_per_board plies boards noise k reuse")
# k: per ply the forced constant of sz_set_forced_playouts; reuse False: an engine without reuse_subtree, `targets` are budgets there
Board = collections.namedtuple("Board", "name make mode salt u targets quiet forced")
# forced: per ply 0 / 1, the board's entry of `boards`; the rest as targetref.Board


def _u(b):
    return lambda ply: ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0


def scenarios():
    import sigma_zero_amd as sz
    start = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    fen = lambda f: (lambda: sz.ChessTensor(fen=f))
    greedy = lambda ply: -1.0
    F = FULL
    on, off = [1] * 5, [0] * 5
    out = []
    # 1. visit targets + root noise at every ply on a reuse engine; greedy boards keep large subtrees (forced selections on kept roots in
    #    the descent-only launch, pruning on continued plies); one board never forced beside the others, one forced on full plies only
    out.append(Scenario("c960_forced", 64, True, True, worst_case(64), 5, [
        Board("sp0/greedy", start(0), "dyadic", 0, greedy, [F] * 5, off, on),
        Board("sp17/greedy/off", start(17), "dyadic", 17, greedy, [F] * 5, off, off),
        Board("sp518/sampled", start(518), "dyadic", 518, _u(518), [F, F, 16, F, F], off, [1, 1, 0, 1, 1]),
        Board("sp77/peaked", start(77), "peaked", 77, greedy, [F, 32, F, F, 8], off, on),
    ], [True] * 5, [2.0, 2.0, 2.0, 0.5, 8.0], True))
    # 2. the wide position: more than 64 children forced and pruned across the four lane passes; k changes between plies, subtrees stay
    out.append(Scenario("wide_forced", 64, True, True, worst_case(64), 3, [
        Board("moves_218/greedy", fen(WIDE_FEN), "dyadic", 1, greedy, [F] * 3, [0] * 3, [1] * 3),
        Board("moves_218/sampled", fen(WIDE_FEN), "dyadic", 2, _u(3), [F] * 3, [0] * 3, [1] * 3),
        Board("moves_218/off", fen(WIDE_FEN), "dyadic", 1, greedy, [F] * 3, [0] * 3, [0] * 3),
        Board("sp333/greedy", start(333), "dyadic", 333, greedy, [F] * 3, [0] * 3, [1] * 3),       # the wide root is soon proven with the solver: a board that searches on
    ], [True] * 3, [4.0, 2.0, 16.0], True))
    # 3. an engine without reuse_subtree: budgets, root noise, a quiet board
    out.append(Scenario("budgets_forced", 64, True, True, None, 4, [
        Board("sp5/greedy", start(5), "dyadic", 5, greedy, [F, 24, F, 9], [0] * 4, [1] * 4),
        Board("sp400/sampled/quiet", start(400), "dyadic", 400, _u(400), [F, F, 8, F], [1] * 4, [1] * 4),
        Board("sp811/off", start(811), "dyadic", 811, greedy, [F, 24, F, 9], [0] * 4, [0] * 4),
    ], [True] * 4, [2.0] * 4, False))
    assert all(3 <= len(sc.boards) <= 4 and sc.plies >= 3 and sc.S == 64 and any(not any(b.forced) for b in sc.boards) for sc in out)
    return out


OPTIONS = TR.OPTIONS                                       # (L, solver): the option combinations the comparison runs under


def new_game(sc, bd, L=1, solver=False):
    return Game(bd.make(), sc.S, sc.edges_per_board, reuse=sc.reuse, L=L, lam=1.0, solver=solver, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt)


def begin_ply(sc, g, bd, b, ply, gam):
    """the setter calls and sz_search_begin of one ply on one board"""
    g.set_root_noise(sc.noise[ply])
    return g.begin(bd.targets[ply], gam[ply][b] if sc.noise[ply] else None, bd.quiet[ply], sc.k[ply] if bd.forced[ply] else 0.0)


def play(sc, L=1, solver=False):
    """the restatement alone: every board of the scenario through its plies"""
    games, gam = [new_game(sc, bd, L, solver) for bd in sc.boards], gammas(sc)
    for ply in range(sc.plies):
        for b, (g, bd) in enumerate(zip(games, sc.boards)):
            if g.live:
                begin_ply(sc, g, bd, b, ply, gam)
                g.run()
                if g.error is None:
                    g.play(bd.u(ply))
    return games


def coverage(played, hook=None):
    """played: [(Scenario, [Game])], hook: the Counter of hook_reference() summed over hook_cases() -> Counter of the conditions of COVERAGE"""
    c = collections.Counter(hook or {})
    for sc, games in played:
        for g in games:
            c.update(g.cov)
            c["forced_selections"] += g.forced_selections
            c["pruned_visits"] += g.pruned_visits
        for ply in range(sc.plies):                        # a board with the bit off beside boards with it on, in the same lock-step search
            bits = [bool(g.forced_plies[ply]) for g in games if len(g.forced_plies) > ply]
            c["bit_off_beside_on"] += any(bits) and not all(bits)
    return c


COVERAGE = ("forced_overruled_puct", "several_forced", "forced_in_flight", "forced_win_skipped", "forced_on_kept_root_at_begin",
            "pruned_on_continued_ply", "last_visit_taken", "bit_off_beside_on", "wide_case", "stopped_at_bound", "m_capped_by_n",
            "pruned_to_zero", "tied_with_best_later", "forced_selections", "pruned_visits")


# ---------------------------------------------------------------------------------------------------------------- sz_debug_forced cases
HookCases = collections.namedtuple("HookCases", "offsets N K W P R parent c fk lam")
HOOK_K = (1, 63, 64, 65, 218)


def hook_cases(n_cases=3000, seed=20, solver=True):
    """Seeded cases for sz_debug_forced: K of 1, 63, 64, 65, 218 and random widths, visit counts with ties, n_p = 1, priors of exactly 0 and
    1, children in flight, proven codes (solver) -> HookCases of flat arrays"""
    rng = np.random.default_rng(seed + (1000 if solver else 0))
    Ns, Ks, Ws, Ps, Rs, off, parent, cs, fks = [], [], [], [], [], [0], [], [], []
    for i in range(n_cases):
        k = HOOK_K[i % 8] if i % 8 < len(HOOK_K) else int(rng.integers(2, 219))
        kind = i % 7
        N = rng.integers(0, 4 if kind == 0 else 40, size=k)                    # kind 0: small counts, many ties
        if kind == 1:
            N[:] = rng.integers(0, 3)                                            # every child tied
        if kind == 2 and k > 1:
            N[rng.integers(0, k)] = N.max()                                      # c* tied with another child
        K = rng.integers(0, 3, size=k) * (rng.random(k) < 0.2)
        P = rng.dirichlet(np.full(k, 0.3)).astype(np.float32) if k > 1 else np.ones(1, np.float32)
        if kind == 3:
            P[rng.random(k) < 0.3] = 0.0                                         # priors of exactly 0 ...
        if kind == 4:
            P[rng.integers(0, k)] = 1.0                                          # ... and exactly 1
        W = (rng.uniform(-1.0, 1.0, size=k) * N).astype(np.float64)
        n_p = 1 if kind == 5 else int(N.sum() + K.sum()) + 1 + int(rng.integers(0, 3))
        R = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.int8), size=k)
        if kind == 6:
            R[:] = 1                                                             # every child WIN: nothing is skipped
        Ns.append(N); Ks.append(K); Ws.append(W); Ps.append(P); Rs.append(R)
        off.append(off[-1] + k); parent.append(n_p); cs.append(rng.choice([1.0, 2.0, 4.0])); fks.append(rng.choice([0.5, 2.0, 8.0, 64.0]))
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dt)
    return HookCases(np.array(off, np.int32), cat(Ns, np.int32), cat(Ks, np.int32), cat(Ws, np.float64), cat(Ps, np.float32),
                     cat(Rs, np.int8) if solver else None, np.array(parent, np.int32), np.array(cs, np.float32), np.array(fks, np.float32), 1.0)


def hook_reference(hc):
    """the restatement's answers to the cases -> (selected, forced, pruned, cstar, Counter)"""
    n = len(hc.parent)
    sel, frc, cst, pruned, cov = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(len(hc.N), np.int32), collections.Counter()
    for i in range(n):
        lo, hi = int(hc.offsets[i]), int(hc.offsets[i + 1])
        R = None if hc.R is None else hc.R[lo:hi]
        sel[i], f, info = select_root(hc.N[lo:hi], hc.K[lo:hi], hc.W[lo:hi], hc.P[lo:hi], R, int(hc.parent[i]), hc.c[i], hc.lam, hc.fk[i])
        frc[i] = int(f)
        cov.update(info)
        cov["wide_case"] += f and hi - lo > 64
        pruned[lo:hi], cst[i], info = prune(hc.N[lo:hi], hc.W[lo:hi], hc.P[lo:hi], int(hc.parent[i]), hc.c[i], hc.fk[i])
        cov.update(info)
        cov["wide_pruned"] += hi - lo > 64 and int((hc.N[lo:hi] - pruned[lo:hi]).sum()) > 0
    return sel, frc, pruned, cst, cov
