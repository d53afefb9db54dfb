"""Plain-Python restatement of the completed-Q selection below the root of a Gumbel search (sz_set_gumbel_tree / sz_gumbel_tree_stats /
sz_debug_gumbel_tree / sz_debug_tree_values, args["gumbel_tree"], a NON-REFERENCE option on top of sz_set_gumbel; include/sigmazero.h is the
specification).  It is what wave_select_tree_gumbel, the selection at depth >= 1 of k_search_step<false, false, GumbelTreeOpts>, is held to,
bit for bit (tests/test_gpu_gumbel_tree.py).  Built on gumbelref, which stays as it is:

  * wsum() is the rule's sum written as the device forms it: 64 per-lane partial sums, then the six xor stages; every lane ends with the same
    bits (tests/test_gumbel_tree_ref.py asserts it), lane 0 is the result;
  * select_tree() is the rule on plain arrays, with gumbelref's slog, sexp, _q and _sigma_factor;
  * Search is a gumbelref.Search that keeps every node's network value where _run expands it (value[edge], f32) and whose _descend uses
    select_tree() below the root; the root's selection, Game.play and the policy target are gumbelref's;
  * Game.gumbel_tree is sz_set_gumbel_tree for this board; begin() takes it up for the search.  With the flag off it IS gumbelref: no class of
    this module touches the search.

scenarios() and hook_cases() are the inputs both test modules use; cov counts, on the restatement alone, the conditions the GPU cases must
reach (COVERAGE, HOOK_COVERAGE, assert_coverage).  A "board" of the whole-search conditions is one board's game over its plies."""
import collections

import numpy as np

import gumbelref as GB
from gumbelref import Gumbel, MAX_MOVES, WIDE_FEN, position_record      # noqa: F401 (re-exported)
from hashmodel import evaluate_packed
from vlref import F32

NAN32 = np.float32("nan")


# ---------------------------------------------------------------------------------------------------------------- the rule
def wsum_lanes(t):
    """the 64 lanes after the butterfly: lane l starts from 0.0 and adds t_c for c = l, l + 64, ... ascending, then v_l = v_l + v_(l xor off) for
    off = 32, 16, 8, 4, 2, 1"""
    lanes = []
    for lane in range(64):
        v = 0.0
        for c in range(lane, len(t), 64):
            v = v + float(t[c])
        lanes.append(v)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[lane] + lanes[lane ^ off] for lane in range(64)]
    return lanes


def wsum(t):
    return wsum_lanes(t)[0]


def select_tree(N, W, P, vhat, opts, lg=None):
    """the selection at an inner node with children N, W, P and the node's own network value vhat -> (child, scores, v_mix, info)"""
    K = len(N)
    N = [int(x) for x in N]
    lg = GB.logits(P) if lg is None else lg
    p = [float(F32(x)) for x in P]
    q = [GB._q(W[c], N[c]) if N[c] >= 1 else None for c in range(K)]
    sf = GB._sigma_factor(opts, max(N))
    sumN = sum(N)
    v01 = 0.5 + 0.5 * float(F32(vhat))
    pq = wsum([p[c] * q[c] if N[c] >= 1 else 0.0 for c in range(K)])
    pm = wsum([p[c] if N[c] >= 1 else 0.0 for c in range(K)])
    v_mix = v01 if sumN == 0 else (v01 + float(sumN) * (pq / pm)) / (1.0 + float(sumN))
    z = [lg[c] + sf * (q[c] if N[c] >= 1 else v_mix) for c in range(K)]
    zmax = max(z)
    e = [GB.sexp(zc - zmax) for zc in z]
    se = wsum(e)
    dn = 1.0 + float(sumN)
    score = [(e[c] / se) - (float(N[c]) / dn) for c in range(K)]
    i = GB._first_max(score, range(K))
    info = collections.Counter()
    info["sumN_0"] += sumN == 0
    info["tree_tie_by_index"] += sum(1 for s in score if s == score[i]) >= 2
    info["wide_inner"] += K > 64
    info["e_exactly_0"] += any(x == 0.0 for x in e)
    return i, score, v_mix, info


# ---------------------------------------------------------------------------------------------------------------- Search / Game
class Search(GB.Search):
    """gumbelref.Search with every expanded node's network value kept and select_tree() below the root.  Game.begin() turns the ply's search
    into one."""
    tree_rule = False
    value = None                                         # edge -> f32 network value of the node behind it, set where it is expanded
    tree_selections = 0
    step_values = None                                   # tree_values() after every search step, beside gumbelref's step_trees
    _tlg = None                                          # parent edge -> its children's logits: the priors of a node do not change

    def _expand(self, e, pol):
        super()._expand(e, pol)
        if self.tree_rule:                               # the value sz_search_step reads from value_dev when it expands the node
            self.value[e] = F32(evaluate_packed(self._planes(e), self.mode, self.salt)[1])

    def _gather(self):
        pending = super()._gather()
        if self.tree_rule:
            if self.step_values is None:
                self.step_values = []
            self.step_values.append(self.tree_values())
        return pending

    def _descend(self):
        if not self.tree_rule:
            return super()._descend()
        path, e = [0], 0
        if self.n[0] > 0:                                # the root: gumbelref's selection, unchanged
            f, k = int(self.first[0]), int(self.n[0])
            if self._lg is None:
                self._lg = GB.logits(self.P[f:f + k])
            i, fb, info = GB.select_root(self.N[f:f + k], self.W[f:f + k], self.P[f:f + k], self.g, self.sims - 1, self.S, self.gumbel, self._lg)
            self.cov.update(info)
            self.gumbel_selections += 1
            self.gumbel_fallbacks += fb
            e = f + i
            path.append(e)
            self.cov["terminal_child_considered"] += bool(self.term[e])
        while self.n[e] > 0:                             # below the root: the completed-Q rule; neither c nor fpu is consulted
            f, k = int(self.first[e]), int(self.n[e])
            if e not in self._tlg:
                self._tlg[e] = GB.logits(self.P[f:f + k])
            i, _, _, info = select_tree(self.N[f:f + k], self.W[f:f + k], self.P[f:f + k], self.value[e], self.gumbel, self._tlg[e])
            self.cov.update(info)
            self.tree_selections += 1
            self.cov["depth_ge_3"] += len(path) - 1 >= 3
            self.cov["terminal_child_scored"] += any(self.term[c] and self.N[c] >= 1 for c in range(f, f + k))
            e = f + i
            path.append(e)
        return path

    def tree_values(self):
        """the kept value of every node, f32, NaN where the node was never expanded, in tree()'s row order (sz_debug_tree_values)"""
        rows = [self.value.get(0, NAN32)]
        stack = [int(self.first[0]) + k for k in range(int(self.n[0]) - 1, -1, -1)] if self.first[0] >= 0 else []
        while stack:
            e = stack.pop()
            rows.append(self.value.get(e, NAN32))
            if self.first[e] >= 0:
                stack += [int(self.first[e]) + k for k in range(int(self.n[e]) - 1, -1, -1)]
        return np.array(rows, np.float32)


class Game(GB.Game):
    """gumbelref.Game with the flag as a setting of the board: g.gumbel_tree = True / False between plies is sz_set_gumbel_tree"""

    def __init__(self, *a, gumbel_tree=False, **kw):
        super().__init__(*a, **kw)
        self.gumbel_tree = bool(gumbel_tree)
        self.tree_plies = []                             # per ply: whether the search ran under the rule
        self.tree_selections = 0
        self.board_tree_selections = []                  # per ply

    def begin(self, budget=None, g=None):
        s = super().begin(budget, g)
        on = self.gumbel_tree
        assert not on or self.gumbel is not None, "SZ_ERR_STATE"
        self.tree_plies.append(on)
        if on:
            assert type(s) is GB.Search
            s.__class__ = Search
            s.tree_rule, s.value, s._tlg = True, {}, {}
            self.cov["budget_2"] += s.S == 2
            self.cov["budget_3"] += s.S == 3
        return s

    def run(self):
        s = super().run()
        n = getattr(s, "tree_selections", 0)
        self.tree_selections += n
        self.board_tree_selections.append(n)
        if getattr(s, "tree_rule", False) and s.S <= 3:
            assert n == 0, "a search of %d simulations selected below the root" % s.S
        return s


# ---------------------------------------------------------------------------------------------------------------- scenarios
Scenario = collections.namedtuple("Scenario", GB.Scenario._fields + ("tree",))


def scenarios():
    """gumbelref's eight boards, budgets and plies under the rule: the five scenarios that differ in m, the draws, FPU (on and ignored below the
    root), c_scale and compaction"""
    keep = ("m16_seeded", "m4_seeded_fpu", "m2_null", "m16_null_scale100", "m16_seeded_compact")
    out = [Scenario(*sc, True) for sc in GB.scenarios() if sc.name in keep]
    assert [sc.name for sc in out] == list(keep)
    return out


def gumbels(sc):
    return GB.gumbels(sc)


def new_game(sc, bd, tree="scenario"):
    return Game(bd.make(), sc.S, None, reuse=False, L=1, lam=1.0, solver=False, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt, fpu=sc.fpu,
                gumbel=sc.gumbel, gumbel_tree=sc.tree if tree == "scenario" else tree)


def play(sc, tree="scenario"):
    """the restatement alone: every board of the scenario through its plies (gumbelref.play's loop)"""
    games, gs = [new_game(sc, bd, tree) for bd in sc.boards], gumbels(sc)
    for ply in range(sc.plies):
        for b, (g, bd) in enumerate(zip(games, sc.boards)):
            if g.live:
                g.begin(bd.budgets[ply], None if gs is None else gs[ply][b])
                g.run()
                GB.play_or_flag(g, 0.5)
    return games


def coverage(played, hook=None):
    c = GB.coverage(played, hook)
    for games in played:
        for g in games:
            c["tree_selections"] += g.tree_selections
    return c


# a selection at a node whose children are all unvisited; a selection at depth >= 3; a visited terminal child among the scored children; a
# score tie broken by index; an inner node with more than 64 children where a selection is made; budgets 2 and 3 (no selection below the root,
# asserted by Game.run); selections made at all
COVERAGE = ("sumN_0", "depth_ge_3", "terminal_child_scored", "tree_tie_by_index", "wide_inner", "budget_2", "budget_3", "tree_selections")
HOOK_COVERAGE = ("K_1", "K_gt_64", "K_218", "all_unvisited", "e_exactly_0", "denormal_prior", "W_plus_N", "W_minus_N", "N_800", "vhat_plus_1",
                 "vhat_minus_1", "tree_tie_by_index")
NO_SELECTION_BOARDS = ("mated",)                         # a terminal root: nothing is ever selected
# nearly every move of the 218-move position mates or stalemates: with m of 2 and 4 all considered children are terminal and nothing is selected
# below them; with m = 16 one or two are not, and theirs are the grandchildren with more than 64 moves
SOME_SCENARIOS_BOARDS = ("moves_218",)


def assert_coverage(cov, names=COVERAGE):
    missing = [k for k in names if cov[k] < 1]
    assert not missing, "conditions not reached: %s of %s" % (missing, dict(cov))


def assert_every_board_selects(scs, played):
    """tree-rule selections > 0 on every board over its plies: in every scenario, but for the 218-move board over the scenarios together and
    for the terminal root never"""
    total = collections.Counter()
    for sc, games in zip(scs, played):
        for bd, g in zip(sc.boards, games):
            total[bd.name] += g.tree_selections
            if bd.name in NO_SELECTION_BOARDS:
                assert g.tree_selections == 0, (sc.name, bd.name)
            elif bd.name not in SOME_SCENARIOS_BOARDS:
                assert g.tree_selections > 0, "%s board %s: no selection below the root" % (sc.name, bd.name)
    for name in SOME_SCENARIOS_BOARDS:
        assert total[name] > 0, "board %s: no selection below the root in any scenario" % name


# ---------------------------------------------------------------------------------------------------------------- sz_debug_gumbel_tree cases
HookCases = collections.namedtuple("HookCases", "offsets N W P vhat opts")
HOOK_K = GB.HOOK_K
HOOK_OPTS = GB.HOOK_OPTS
HOOK_NMAX = (1, 4, 30, 800)


def hook_cases(n_cases=500, seed=91):
    """Seeded child sets for sz_debug_gumbel_tree: K of 1, 2, 63, 64, 65, 128, 218 and random widths; visit counts up to 1, 4, 30 or 800; all
    children unvisited; equal children (a tie the index breaks); f32-denormal priors; W_c = +N_c and W_c = -N_c (q of 0 and 1); a child with
    800 visits; vhat of +1 and -1; a c_scale that drives some e_c to exactly 0 -> HookCases of flat arrays"""
    rng = np.random.default_rng(seed)
    Ns, Ws, Ps, off, vhat, opts = [], [], [], [0], [], []
    for i in range(n_cases):
        k = HOOK_K[i % 10] if i % 10 < len(HOOK_K) else int(rng.integers(2, 219))
        kind = (i // 10) % 8
        ob = HOOK_OPTS[int(rng.integers(0, len(HOOK_OPTS)))]
        N = rng.integers(0, HOOK_NMAX[int(rng.integers(0, len(HOOK_NMAX)))] + 1, size=k)
        if kind == 0:
            N[:] = 0                                                             # all children unvisited: v_mix = v01, the softmax of the logits
        P = rng.dirichlet(np.full(k, 0.3)).astype(np.float32) if k > 1 else np.ones(1, np.float32)
        P = np.maximum(P, np.float32(2.0 ** -140))                               # a prior that is exactly 0 is dropped at expansion
        if kind == 2:
            P[:] = np.float32(1.0 / 256)                                         # equal children: every score is the same, the first child wins
            N[:] = int(rng.integers(0, 5))
        if kind == 3:
            P[rng.random(k) < 0.3] = np.float32(1e-42)                           # denormal in f32
        W = (rng.uniform(-1.0, 1.0, size=k) * N).astype(np.float64)
        if kind == 2:
            W[:] = -0.25 * N
        if kind == 4:
            W = np.where(rng.random(k) < 0.5, 1.0, -1.0) * N                     # q of exactly 0 and exactly 1
        if kind == 5:
            N[int(rng.integers(0, k))] = 800
            W = (rng.uniform(-1.0, 1.0, size=k) * N).astype(np.float64)
        v = (1.0, -1.0)[kind - 6] if kind >= 6 else rng.uniform(-1.0, 1.0)
        Ns.append(N); Ws.append(np.asarray(W, np.float64)); Ps.append(P)
        off.append(off[-1] + k); vhat.append(v); opts.append(ob)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dt)
    o = np.zeros(n_cases, np.dtype([("max_considered", np.int32), ("c_visit", np.float32), ("c_scale", np.float32)]))
    for i, ob in enumerate(opts):
        o[i] = tuple(ob)
    return HookCases(np.array(off, np.int32), cat(Ns, np.int32), cat(Ws, np.float64), cat(Ps, np.float32), np.array(vhat, np.float32), o)


def hook_reference(hc):
    """the restatement's answers to the cases -> (selected, scores f64 flat, v_mix f64, Counter)"""
    n = len(hc.vhat)
    sel, score, vmix, cov = np.zeros(n, np.int32), np.zeros(len(hc.N), np.float64), np.zeros(n, np.float64), collections.Counter()
    for i in range(n):
        lo, hi = int(hc.offsets[i]), int(hc.offsets[i + 1])
        ob = Gumbel(*[x.item() for x in hc.opts[i]])
        N, W, P = hc.N[lo:hi], hc.W[lo:hi], hc.P[lo:hi]
        sel[i], score[lo:hi], vmix[i], info = select_tree(N, W, P, hc.vhat[i], ob)
        cov.update(info)
        k = hi - lo
        cov["K_1"] += k == 1
        cov["K_gt_64"] += k > 64
        cov["K_218"] += k == 218
        cov["all_unvisited"] += not (N >= 1).any()
        cov["denormal_prior"] += bool(((P > 0) & (P < np.float32(2.0 ** -126))).any())
        cov["W_plus_N"] += bool(((N >= 1) & (W == N)).any())
        cov["W_minus_N"] += bool(((N >= 1) & (W == -N)).any())
        cov["N_800"] += int(N.max()) == 800
        cov["vhat_plus_1"] += hc.vhat[i] == 1.0
        cov["vhat_minus_1"] += hc.vhat[i] == -1.0
    return sel, score, vmix, cov
