"""Plain-Python restatement of the engine's search with leaf batching, the solver and subtree reuse TOGETHER (sz_set_search_options /
args["combine_options"], NON-REFERENCE options; include/sigmazero.h is the specification).  It is what k_search_begin<VL, SOLVE>,
k_search_step<true, true>, the descent-only launch of sz_search_begin and k_play's compaction (csrc/sz_engine.hip) are held to, bit for bit
(tests/test_gpu_compose.py).  Built on the three single-option restatements, which stay as they are:

  * Search derives from solverref.Search (labels R, `complete`, the update walk, the readouts) and takes L and lam back from vlref.Search;
    with solver=False, reuse off it is vlref's search, with L = 1 it is solverref's, with L = 1, solver=False and a carried tree reuseref's
    (tests/test_compose_ref.py pins all three);
  * one step = expand and back up every pending leaf in gather order (k taken back along its path), then gather: descend with virtual loss
    over the children that are not WIN; a descent that meets a proven node is backed up there and the gather goes on; a new terminal leaf
    is labelled, backed up and its labels are carried up; a new non-terminal leaf becomes pending (k + 1 along its path); a descent that
    ends on a leaf pending in this step ends the gather;
  * reroot(): the next ply's tree is a recursive copy of the chosen child's subtree, labels and `complete` bits included; a continued
    search has nothing pending and gathers first (sz_search_begin's descent-only launch);
  * at the end of every search every in-flight count is 0 (asserted in run()).

Game plays one board ply after ply; set_options() is the rule for a setting change on a reuse engine.  cov counts, on the restatement
alone, the events the GPU cases must reach (COVERAGE)."""
import collections
import math

import numpy as np

import solverref
from hashmodel import evaluate_packed, pack_planes
from reuseref import CapacityError, E_CAP_FLOOR, FALLBACKS, MAX_MOVES, choose, position_record, worst_case    # noqa: F401 (re-exported)
from solverref import UNKNOWN, WIN, DRAW, LOSS, VALUE
from vlref import F32, ucb

_ARRAYS = ("W", "N", "P", "K", "first", "n", "action", "term", "tval", "R", "complete")


class Search(solverref.Search):
    def __init__(self, game, S, L=1, lam=1.0, solver=False, edges_per_board=None, room=0, **kw):
        super().__init__(game, S, solver=solver, **kw)
        self.L, self.lam = int(L), float(np.float32(lam))               # solverref.Search fixes L = 1
        self.kw = dict(kw)
        self.edges_per_board = None if edges_per_board is None else int(edges_per_board)
        self.e_cap = None if edges_per_board is None else max(self.edges_per_board, E_CAP_FLOOR)       # None: the default store, no search overflows
        if room:                                         # a carried tree: room for its edges on top of the S expansions of this search
            cap = room + max(self.S, 1) * MAX_MOVES + 2
            for name in _ARRAYS:
                a = getattr(self, name)
                setattr(self, name, np.full(cap, -1, a.dtype) if name == "first" else np.zeros(cap, a.dtype))
        self.continued = False                           # the search goes on on a kept subtree
        self.kept_edges = self.kept_nodes = 0
        self.begin_tree = self.begin_proven = None       # tree() / tree_proven() when sz_search_begin returns
        self.begin_rows = 0                              # network rows asked for by sz_search_begin (a continued search: leaves of the descent-only launch)
        self.error = None
        self.cov = collections.Counter()

    def settings(self):
        return dict(L=self.L, lam=self.lam, solver=self.solver, edges_per_board=self.edges_per_board, **self.kw)

    # -- tree operations
    def _expand(self, e, pol):
        super()._expand(e, pol)
        if self.e_cap is not None and self.n_edges > self.e_cap:
            raise CapacityError()

    def _descend(self):
        path, e = [0], 0
        lam = np.float64(self.lam)
        while self.n[e] > 0 and not (self.solver and self.R[e]):
            f, k = self.first[e], self.n[e]
            kk = self.K[f:f + k]
            sq = F32(math.sqrt(float(self.N[e] + self.K[e])))
            u = ucb(self.N[f:f + k] + kk, self.W[f:f + k] + lam * kk.astype(np.float64), self.P[f:f + k], sq, self.c)
            i = int(np.argmax(u))
            if self.solver:
                cand = np.nonzero(self.R[f:f + k] != WIN)[0]
                if len(cand):                            # every child WIN: all children, as without the solver
                    if self.R[f + i] == WIN:
                        self.skips += 1
                        self.cov["win_child_skipped"] += 1
                    i = int(cand[np.argmax(u[cand])])
            e = f + i
            path.append(e)
        return path

    def _gather(self):
        pending = []
        while self.sims + len(pending) < self.S and len(pending) < self.L:
            path = self._descend()
            e = path[-1]
            if self.solver and self.R[e]:                # the first proven node on the way: backed up on the spot, nothing goes in flight
                self._end(path, VALUE[int(self.R[e])])
                self.proven_stops += 0 if self.term[e] else 1
                if pending and e == 0:
                    self.cov["root_stop_while_pending"] += 1
                if pending and e != 0 and not self.term[e]:
                    self.cov["inner_stop_with_k_elsewhere"] += 1
                continue
            if e in self.games:
                if not self.term[e] and self.first[e] < 0:      # pending in this step: a collision ends the gather
                    self.collisions += 1
                    break
                self._end(path, float(self.tval[e]))            # visited leaf without children
                continue
            g = self.games[path[-2]].copy()
            g.push_action(int(self.action[e]))
            self.games[e] = g
            v, t = g.get_value_and_terminated()
            self.term[e], self.tval[e] = int(t), int(v) if t else 0
            if t:
                if self.solver:
                    self.R[e] = LOSS if v == -1 else DRAW
                self._end(path, float(v))
                if self.solver:
                    was = int(self.R[0])
                    self._update(path)
                    if pending and not was and self.R[0]:
                        self.cov["root_proven_mid_gather"] += 1
                continue
            self.K[path] += 1
            pending.append((path, self._planes(e)))
        return pending

    def _run(self):
        pending, descent_only = [], self.continued
        if not self.continued:
            root = self.games[0]
            tv, term = root.get_value_and_terminated()
            if term or self.S <= 0:                      # a terminal root: every simulation re-visits it (mcts.py:104-109)
                S = max(self.S, 0)
                self.W[0], self.N[0], self.sims, self.terminal_hits = float(tv) * S, 1 + S, S, S
                if self.solver and term:
                    self.R[0] = LOSS if tv == -1 else DRAW
                self.begin_tree, self.begin_proven = self.tree(), self.tree_proven()
                return
            pending = [([0], self._planes(0))]
            self.K[0] = 1                                # the root's own evaluation is in flight
            self.begin_tree, self.begin_proven, self.begin_rows = self.tree(), self.tree_proven(), 1
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
            pending = self._gather()
            if descent_only:                             # sz_search_begin's descent-only launch
                descent_only = False
                self.begin_tree, self.begin_proven, self.begin_rows = self.tree(), self.tree_proven(), len(pending)
                if len(pending) > 1:
                    self.cov["continued_gathers_several"] += 1
                if not pending and self.solver and self.R[0]:
                    self.cov["kept_root_proven_done_at_begin"] += 1

    def run(self):
        try:
            self._run()
            assert not self.K[:self.n_edges].any(), "a descent is still in flight at the end of the search"
            assert self.sims == max(self.S, 0)
        except CapacityError:
            self.error = "capacity"
        return self

    # -- subtree reuse
    def reroot(self, action, game):
        """-> (the next ply's Search, "reused" or the name of the fall-back).  `game` is the board's game after the move"""
        fresh = lambda reason: (Search(game, self.S, **self.settings()), reason)
        f, k = int(self.first[0]), int(self.n[0])
        c = f + [int(a) for a in self.action[f:f + k]].index(int(action))
        if c not in self.games:
            return fresh("unvisited")
        if self.n[c] == 0:
            return fresh("leaf")
        new = Search(game, self.S, room=self.n_edges, **self.settings())
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
        if len(new.games) > self.S:
            return fresh("nodes")
        if 2 * new.n_edges > new.e_cap:
            return fresh("edges")
        new.continued, new.kept_edges, new.kept_nodes = True, new.n_edges, len(new.games)
        return new, "reused"


def search(game, S, **kw):
    return Search(game, S, **kw).run()


class Game:
    """One board, ply after ply: begin() -> run() -> play(u).  starts[p] says how ply p's search began: "new" (first ply), "reused", a
    fall-back's name, or "dropped" (set_options() changed L or the solver); counters are cumulative like the engine's."""
    COUNTERS = ("simulations", "expansions", "terminal_hits", "sum_depth", "proven_stops", "proved")

    def __init__(self, game, S, edges_per_board=None, reuse=True, L=1, lam=1.0, solver=False, **kw):
        self.game, self.S, self.reuse = game.copy(), int(S), bool(reuse)
        self.opts = dict(L=int(L), lam=lam, solver=bool(solver), edges_per_board=edges_per_board if reuse else None, **kw)
        if reuse:
            assert edges_per_board is not None, "a reuse engine's child slots decide the 'edges' fall-back"
        self.next = self.search = None
        self.starts, self.searches, self.roots, self.chosen = [], [], [], []
        self.over, self.result, self.error, self.last_fallback = False, 0, None, None
        for k in self.COUNTERS:
            setattr(self, k, 0)
        self.cov = collections.Counter()

    @property
    def live(self):
        return not self.over and self.error is None

    def set_options(self, L, lam, solver):
        """sz_set_search_options between two plies: a change of L or of the solver drops the kept subtree, anything else keeps it"""
        changed = int(L) != self.opts["L"] or bool(solver) != self.opts["solver"]
        self.opts.update(L=int(L), lam=lam, solver=bool(solver))
        if self.next is not None:
            if changed:
                self.next = (Search(self.game, self.S, **self.opts), "dropped")
            else:
                self.next[0].lam = float(np.float32(lam))

    def begin(self):
        self.search, start = self.next if self.next is not None else (Search(self.game, self.S, **self.opts), "new")
        self.next = None
        self.starts.append(start)
        self.searches.append(self.search)
        self.roots.append(self.game.copy())
        return self.search

    def run(self):
        s = self.search.run()
        self.error = s.error
        for k, attr in zip(self.COUNTERS, ("sims", "expansions", "terminal_hits", "sum_depth", "proven_stops", "proved")):
            setattr(self, k, getattr(self, k) + getattr(s, attr))
        self.cov.update(s.cov)
        return s

    def play(self, u):
        """sz_play: the training record of this ply (sz_fetch_ply's fields), the move, the game-over test, the subtree kept"""
        s = self.search
        acts, vis = s.root_children()
        k = len(acts)
        assert k > 0 and vis.sum() > 0, "SZ_ERR_ZERO_VISITS"
        if s.solver and s.R[0] == WIN:
            self.cov["win_root_played"] += 1
        chosen = int(acts[s.choose(u)])
        rec = dict(packed=pack_planes(self.game.get_representation().numpy()), action=np.full(MAX_MOVES, -1, np.int32),
                   visits=np.zeros(MAX_MOVES, np.int32), n_child=k, colour=int(bool(self.game.board.turn)), chosen=chosen)
        rec["action"][:k], rec["visits"][:k] = acts, vis
        self.chosen.append(chosen)
        self.game.push_action(chosen)
        v, t = self.game.get_value_and_terminated()
        self.over = bool(t)
        self.result = 0 if not (t and v) else (-1 if self.game.board.turn else 1)       # the side to move is mated
        rec["game_over"], rec["result"] = int(self.over), self.result
        if self.reuse:
            nxt = s.reroot(chosen, self.game)
            if self.over:
                self.last_fallback = nxt[1]
            else:
                self.next = nxt
        return rec

    def fallbacks(self):
        c = collections.Counter(x for x in self.starts if x in FALLBACKS)
        if self.last_fallback in FALLBACKS:
            c[self.last_fallback] += 1
        return c


# ---------------------------------------------------------------------------------------------------------------- the GPU case sets
L_VALUES = (2, 7, 32)
EXTRA_FENS = {"kqk_stalemates": "k7/8/1Q6/8/8/8/8/7K w - - 0 1"}


def solver_items():
    """(S, chess960) -> [(name, position, salt)]: solver_cases.CASES plus the standard start and two Chess960 starts (test_gpu_solver's groups)"""
    import sigma_zero_amd as sz
    import solver_cases as SC
    out = {}
    for name, S, salt in SC.CASES:
        out.setdefault((S, False), []).append((name, SC.game(name), salt))
    out[(64, False)].append(("endgame_6_men", SC.game("endgame_6_men"), 1))
    # none of solver_cases.FENS stops a descent at a proven INNER node within 200 simulations (salts 0..7 tried): a proven child is WIN (skipped)
    # or LOSS (then its parent is WIN and stops the descent first), so only a non-terminal DRAW node can.  King and queen against a bare king
    # with stalemates one move away has them
    out[(64, False)].append(("kqk_stalemates", sz.ChessTensor(fen=EXTRA_FENS["kqk_stalemates"]), 5))
    out[(64, False)].append(("start", sz.ChessTensor(), 3))
    out[(200, False)].append(("start", sz.ChessTensor(), 5))
    out[(64, True)] = [("sp0", sz.ChessTensor(chess960=True, scharnagl=0), 4), ("sp959", sz.ChessTensor(chess960=True, scharnagl=959), 7)]
    assert all(len(v) <= 8 for v in out.values())
    return out


def solver_refs(S, c960, L, learning, lam=1.0):
    return [search(ct, S, L=L, lam=lam, solver=True, learning=learning, mode="dyadic", salt=salt) for _, ct, salt in solver_items()[(S, c960)]]


GameCase = collections.namedtuple("GameCase", "name S c960 learning edges_per_board plies boards")
GameBoard = collections.namedtuple("GameBoard", "name make mode salt u")


def _u(b):
    return lambda ply: ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0


def game_cases():
    """whole games with reuse (run at every (L, solver) of GAME_OPTIONS): endgame_6_men and a Chess960 start; a peaked evaluator for the
    'nodes' fall-back, few child slots for 'edges'"""
    import sigma_zero_amd as sz
    import solver_cases as SC
    greedy = lambda ply: -1.0
    last = lambda ply: 1.0 if ply % 2 == 0 else 0.5       # u = 1.0 samples the last child whether it was visited or not
    end = lambda: SC.game("endgame_6_men")
    sp = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    return [
        GameCase("endgame", 64, False, True, worst_case(64), 60, [GameBoard("6men/%d" % s, end, "dyadic", s, _u(s)) for s in (1, 2, 3)] +
                 [GameBoard("6men/greedy%d" % s, end, "dyadic", s, greedy) for s in (1, 4)]),
        GameCase("endgame_plain", 64, False, False, worst_case(64), 40, [GameBoard("6men/%d" % s, end, "dyadic", s, greedy if s % 2 else _u(s)) for s in (0, 5, 6, 7)]),
        GameCase("c960", 64, True, False, worst_case(64), 12, [GameBoard("sp518/%d" % s, sp(518), "dyadic", s, greedy if s % 2 else _u(s)) for s in (0, 1)] +
                 [GameBoard("sp518/peaked", sp(518), "peaked", 518, greedy), GameBoard("sp518/last_child", sp(518), "dyadic", 0, last)]),
        # few child slots: the "edges" fall-back; where a search does not fit, SZ_ERR_CAPACITY on both sides ends that board
        GameCase("c960_2300_slots", 64, True, False, 2300, 6, [GameBoard("sp518/peaked", sp(518), "peaked", 518, greedy)]),
        GameCase("c960_2600_slots", 64, True, False, 2600, 8, [GameBoard("sp518/peaked77", sp(518), "peaked", 77, greedy)]),
    ]


GAME_OPTIONS = [(1, False), (4, False), (1, True), (4, True)]           # (L, solver), all with reuse


def new_game(gc, bd, L, solver, reuse=True, lam=1.0):
    return Game(bd.make(), gc.S, gc.edges_per_board, reuse=reuse, L=L, lam=lam, solver=solver, c=2.0, learning=gc.learning, mode=bd.mode, salt=bd.salt)


def play(gc, L, solver, reuse=True):
    """the restatement alone: every board of the case through its plies"""
    games = [new_game(gc, bd, L, solver, reuse) for bd in gc.boards]
    for ply in range(gc.plies):
        for g, bd in zip(games, gc.boards):
            if g.live:
                g.begin()
                g.run()
                if g.error is None:
                    g.play(bd.u(ply))
    return games


# the events the issue lists; counted by Search.cov / Game.cov, summed over a case set
SOLVER_COVERAGE = ("root_proven_mid_gather", "root_stop_while_pending", "inner_stop_with_k_elsewhere", "win_child_skipped")
GAME_COVERAGE = ("continued_gathers_several", "kept_root_proven_done_at_begin", "win_root_played")
