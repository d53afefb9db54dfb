"""Plain-Python restatement of subtree reuse as a self-play configuration (sz_set_visit_targets / sz_search_goals / sz_set_search_root_noise,
args["visit_targets"], NON-REFERENCE options; include/sigmazero.h is the specification).  It is what k_search_begin's goal computation and
begin-time root mix and the d == 0 expansion site of k_search_step (csrc/sz_engine.hip) are held to, bit for bit, ply after ply
(tests/test_gpu_visit_targets.py).  Built on composeref (Search / Game), which stays as it is:

  * the capacity S (store sizes, the "nodes" fall-back) and the per-ply goal are separate: Search.cap is num_searches, Search.S, which
    composeref's loops read as the budget, is the goal of this search, set by begin();
  * begin(target, gamma, quiet): goal = target on a fresh root, max(0, target + 1 - N_kept) on a kept one (target None: num_searches); a
    kept root's children are mixed with the board's Gamma draws in place, P = (0.75*P) + (0.25*(g / gs)), unless the board is quiet;
  * a fresh root is mixed when it is expanded; under root noise (gamma given) no node gets the reference's constant;
  * gs is summed the kernel's way, vlref.masked_sum's scheme over the child index: lane c % 64 adds g[c] ascending, then an xor butterfly;
  * Game.set_root_noise(on): switching between the reference's noise and root noise drops the kept subtree ("dropped"), as
    sz_set_search_options does for a change of L or the solver.

With target None, gamma None it is composeref, and hence reuseref and vlref (tests/test_target_ref.py pins it).  scenarios() are the inputs
both test modules use; cov counts, on the restatement alone, the conditions the GPU cases must reach (COVERAGE)."""
import collections

import numpy as np

import composeref as CR
from composeref import FALLBACKS, MAX_MOVES, position_record, worst_case        # noqa: F401 (re-exported)
from vlref import F32


def gamma_sum(g, k):
    """the kernel's sum of the first k Gamma draws: lane-strided partial sums (lane l adds g[l], g[l+64], ... ascending), xor butterfly"""
    lanes = np.zeros(64, np.float32)
    for c in range(k):
        lanes[c % 64] = lanes[c % 64] + g[c]
    off = 32
    while off >= 1:
        lanes = lanes + lanes[np.arange(64) ^ off]
        off >>= 1
    return lanes[0]


def root_mix(p, g):
    """priors p[0..k) of a root's children mixed with the draws g: (0.75f * p) + (0.25f * (g / gs)), every operator one f32 rounding"""
    k = len(p)
    g = np.asarray(g, np.float32)
    gs = gamma_sum(g, k)
    with np.errstate(all="ignore"):
        return (F32(0.75) * p.astype(np.float32)) + (F32(0.25) * (g[:k] / gs))


class Search(CR.Search):
    def __init__(self, game, S, **kw):
        super().__init__(game, S, **kw)
        self.cap = self.S                                # num_searches: the capacity.  self.S becomes the goal at begin()
        self.goal = self.target = None
        self.gamma, self.quiet = None, False
        self.n_kept = 1                                  # root visit count at search begin (a fresh root: 1)
        self.noised_kept_children = 0                    # children of a kept root mixed at begin

    def begin(self, target=None, gamma=None, quiet=False):
        """sz_search_begin's part of the options: the goal, and the mix of a kept root.  gamma: this board's draws [218] f32 or None"""
        self.target, self.gamma, self.quiet = target, (None if gamma is None else np.asarray(gamma, np.float32)), bool(quiet)
        t = self.cap if target is None else int(target)
        assert 0 <= t <= self.cap
        self.n_kept = int(self.N[0])
        self.goal = max(0, t + 1 - self.n_kept) if self.continued and target is not None else t     # targets off: num_searches new simulations
        self.S = self.goal
        if self.continued and self._noisy():
            f, k = int(self.first[0]), int(self.n[0])
            self.P[f:f + k] = root_mix(self.P[f:f + k], self.gamma)
            self.noised_kept_children = k
        return self.goal

    def _noisy(self):
        return self.learning and self.gamma is not None and not self.quiet

    def _expand(self, e, pol):
        if self.gamma is None:
            return super()._expand(e, pol)
        learning, self.learning = self.learning, False   # root noise on: no node gets the reference's constant
        try:
            super()._expand(e, pol)
        finally:
            self.learning = learning
        if e == 0 and self._noisy() and self.n[0] > 0:
            f, k = int(self.first[0]), int(self.n[0])
            self.P[f:f + k] = root_mix(self.P[f:f + k], self.gamma)

    def run(self):
        if self.goal is None:
            self.begin()
        return super().run()

    def reroot(self, action, game):
        """composeref.Search.reroot with the capacity, not this search's goal, as num_searches: the fresh-start conditions are unchanged"""
        S = self.cap
        fresh = lambda reason: (Search(game, S, **self.settings()), reason)
        f, k = int(self.first[0]), int(self.n[0])
        c = f + [int(a) for a in self.action[f:f + k]].index(int(action))
        if c not in self.games:
            return fresh("unvisited")
        if self.n[c] == 0:
            return fresh("leaf")
        new = Search(game, S, room=self.n_edges, **self.settings())
        new.games = {}

        def copy(src, dst):
            for name in ("W", "N", "P", "action", "term", "tval", "R", "complete"):
                getattr(new, name)[dst] = getattr(self, name)[src]
            if src in self.games:
                new.games[dst] = self.games[src].copy()
            if self.first[src] >= 0:
                kk, span = int(self.n[src]), new.n_edges
                new.first[dst], new.n[dst] = span, kk
                new.n_edges += kk
                for j in range(kk):
                    copy(int(self.first[src]) + j, span + j)

        copy(c, 0)
        if len(new.games) > S:
            return fresh("nodes")
        if 2 * new.n_edges > new.e_cap:
            return fresh("edges")
        new.continued, new.kept_edges, new.kept_nodes = True, new.n_edges, len(new.games)
        return new, "reused"


class Game(CR.Game):
    """composeref.Game with a target, Gamma draws and a quiet flag per ply, and the noise mode as a setting"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.noise_on = False                            # sz_set_search_root_noise with gamma_dev != NULL is in force
        self.goals, self.kept_visits, self.targets = [], [], []     # per ply

    def _fresh(self):
        return Search(self.game, self.S, **self.opts)

    def set_options(self, L, lam, solver):
        changed = int(L) != self.opts["L"] or bool(solver) != self.opts["solver"]
        self.opts.update(L=int(L), lam=lam, solver=bool(solver))
        if self.next is not None:
            if changed:
                self.next = (self._fresh(), "dropped")
            else:
                self.next[0].lam = float(np.float32(lam))

    def set_root_noise(self, on):
        """a call of sz_set_search_root_noise: switching between gamma_dev == NULL and non-NULL drops the kept subtree"""
        if bool(on) != self.noise_on and self.reuse and self.next is not None:
            self.next = (self._fresh(), "dropped")
            self.cov["noise_switch_dropped"] += 1
        self.noise_on = bool(on)

    def begin(self, target=None, gamma=None, quiet=False):
        assert (gamma is not None) == self.noise_on, "set_root_noise() first"
        self.search, start = self.next if self.next is not None else (self._fresh(), "new")
        self.next = None
        self.starts.append(start)
        self.searches.append(self.search)
        self.roots.append(self.game.copy())
        s = self.search
        goal = s.begin(target, gamma, quiet)
        self.goals.append(goal)
        self.kept_visits.append(s.n_kept)
        if target is not None:
            t = int(target)
            if start == "reused":
                self.cov["continued_goal_0"] += goal == 0
                self.cov["continued_goal_between"] += 0 < goal < t
                run = 1
                while run < len(self.starts) and self.starts[-1 - run] == "reused":
                    run += 1
                self.cov["three_continued_in_a_row"] += run >= 3
                if self.targets and self.targets[-1] == s.cap and t < s.cap:
                    self.cov["fast_after_full"] += 1
            if start in FALLBACKS and t == s.cap and goal == t:
                self.cov["fresh_fallback_full_goal"] += 1
        if start == "reused" and s.noised_kept_children > 64:
            self.cov["noised_kept_root_wide"] += 1
        self.targets.append(None if target is None else int(target))
        return s


# ---------------------------------------------------------------------------------------------------------------- scenarios
Scenario = collections.namedtuple("Scenario", "name S c960 learning edges_per_board plies boards noise")
# noise: per ply True / False = root noise on / off for that ply's search (a switch drops the kept subtrees); boards: [Board]
Board = collections.namedtuple("Board", "name make mode salt u targets quiet")
# targets: per ply the visit target (None: targets off for the whole scenario); quiet: per ply 0 / 1

FULL = 64
WIDE_FEN = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"       # 218 legal moves (tests/reuseref.py scenario 2, tests/solver_cases.py)


def _u(b):
    return lambda ply: ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0


def gammas(sc):
    """the Gamma(0.3, 1) draws of a scenario, [plies][boards][218] f32 from a seeded generator: arbitrary f32 values, not dyadic ones"""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(sc.name))
    return np.random.default_rng(seed).standard_gamma(0.3, size=(sc.plies, len(sc.boards), MAX_MOVES)).astype(np.float32)


def scenarios():
    import sigma_zero_amd as sz
    start = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    fen = lambda f: (lambda: sz.ChessTensor(fen=f))
    greedy = lambda ply: -1.0
    last = lambda ply: 1.0 if ply % 2 == 0 else 0.5       # u = 1.0 samples the last child whether it was visited or not: a fresh fall-back
    F, on8, q0 = FULL, [True] * 8, [0] * 8
    cap = [F, 8, 8, F, 16, 8, F, 8]                        # playout-cap style: full plies with fast ones between
    out = []
    # 1. root noise at every ply, targets full / fast; greedy boards keep large subtrees (goal 0 and 0 < goal < t), one board is quiet on its
    #    fast plies next to noisy ones, one falls back to a fresh root at full target
    out.append(Scenario("c960_noise", 64, True, True, worst_case(64), 8, [
        Board("sp0/greedy", start(0), "dyadic", 0, greedy, cap, q0),
        Board("sp17/greedy/quiet_fast", start(17), "dyadic", 17, greedy, cap, [int(t < F) for t in cap]),
        Board("sp518/sampled", start(518), "dyadic", 518, _u(518), cap, q0),
        Board("sp959/all_full", start(959), "dyadic", 959, greedy, [F] * 8, q0),
        Board("sp333/quiet", start(333), "dyadic", 333, greedy, [F, 24, 24, 24, F, 4, 4, 2], [1] * 8),
        Board("sp702/last_child", start(702), "dyadic", 702, last, [F] * 8, q0),
        Board("sp77/peaked", start(77), "peaked", 77, greedy, [F, 8, F, 8, F, 32, 8, F], q0),
    ], on8))
    # 2. the wide position: ply 2's kept root has far more than 64 children and is noised at begin
    out.append(Scenario("wide_noise", 64, False, True, worst_case(64), 4, [
        Board("moves_218/greedy", fen(WIDE_FEN), "dyadic", 1, greedy, [F, F, F, 8], [0] * 4),
        Board("moves_218/sampled", fen(WIDE_FEN), "dyadic", 2, _u(3), [F, F, F, 16], [0] * 4),
        Board("moves_218/quiet", fen(WIDE_FEN), "dyadic", 1, greedy, [F, F, 32, 8], [1] * 4),
    ], [True] * 4))
    # 3. the noise mode switches on at ply 3 and off at ply 6: both drop the kept subtrees; the reference's constant noise before and after
    out.append(Scenario("noise_switch", 64, True, True, worst_case(64), 8, [
        Board("sp5/greedy", start(5), "dyadic", 5, greedy, [F, 8, F, 8, 8, F, 8, 16], q0),
        Board("sp400/sampled", start(400), "dyadic", 400, _u(400), [F, F, 8, F, 8, 8, F, 8], q0),
    ], [False, False, False, True, True, True, False, False]))
    # 4. targets without root noise and without `learning`
    out.append(Scenario("plain_targets", 64, True, False, worst_case(64), 8, [
        Board("sp811/greedy", start(811), "dyadic", 811, greedy, cap, q0),
        Board("sp100/sampled", start(100), "dyadic", 100, _u(100), cap, q0),
    ], [False] * 8))
    assert all(len(sc.boards) <= 8 and sc.plies <= 8 and sc.S == 64 for sc in out)
    return out


OPTIONS = [(1, False), (4, True)]                          # (L, solver): the option combinations the comparison runs under


def new_game(sc, bd, L=1, solver=False, reuse=True):
    return Game(bd.make(), sc.S, sc.edges_per_board, reuse=reuse, L=L, lam=1.0, solver=solver, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt)


def begin_ply(sc, g, bd, b, ply, gam):
    """the setter calls and sz_search_begin of one ply on one board"""
    g.set_root_noise(sc.noise[ply])
    return g.begin(bd.targets[ply] if bd.targets is not None else None, gam[ply][b] if sc.noise[ply] else None, bd.quiet[ply])


def play(sc, L=1, solver=False, reuse=True):
    """the restatement alone: every board of the scenario through its plies"""
    games, gam = [new_game(sc, bd, L, solver, reuse) for bd in sc.boards], gammas(sc)
    for ply in range(sc.plies):
        for b, (g, bd) in enumerate(zip(games, sc.boards)):
            if g.live:
                begin_ply(sc, g, bd, b, ply, gam)
                g.run()
                if g.error is None:
                    g.play(bd.u(ply))
    return games


def coverage(played):
    """played: [(Scenario, [Game])] -> Counter of the conditions of COVERAGE"""
    c = collections.Counter()
    for sc, games in played:
        for g in games:
            c.update(g.cov)
        for ply in range(sc.plies):                        # a quiet board next to a noisy one in the same lock-step search
            if sc.noise[ply]:
                live = [b for b, g in enumerate(games) if len(g.starts) > ply]
                q = [sc.boards[b].quiet[ply] for b in live]
                c["quiet_next_to_noisy"] += any(q) and not all(q)
    return c


COVERAGE = ("continued_goal_0", "continued_goal_between", "fresh_fallback_full_goal", "fast_after_full", "three_continued_in_a_row",
            "noised_kept_root_wide", "quiet_next_to_noisy", "noise_switch_dropped")
