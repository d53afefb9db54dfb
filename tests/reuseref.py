"""Plain-Python restatement of the engine's subtree reuse (sz_config.reuse_subtree / args["reuse_subtree"], a NON-REFERENCE option;
include/sigmazero.h): sz_play keeps the subtree below the move it plays and the next search continues on it.  It is what k_play's
in-place compaction and k_search_begin's reuse branch (csrc/sz_engine.hip) are held to, bit for bit, ply after ply
(tests/test_gpu_subtree_reuse.py).  Written the obvious way, not the kernel's way:

  * Search.reroot(action, game): the next search's tree is a recursive copy of the chosen child's subtree into a NEW store (edges, games,
    term / tval, W, N, P; children in order, each node's children in one contiguous span).  No compaction in place, no node map.  The
    chosen child becomes edge 0 with its own N, W and P.
  * the fall-backs to a fresh root (N = 1, no children), each reported by name (FALLBACKS):
      "unvisited"  the chosen child was never visited (k_play: node < 0),
      "leaf"       it was visited and has no children (k_play: n == 0).  A visited node without children is a terminal position (an expansion
                   keeps NaN priors, so it never leaves a live node childless): the game is over and no search follows,
      "nodes"      the kept subtree has more than S visited nodes (k_search_begin: n_nodes <= S fails),
      "edges"      twice its edge count, edge 0 included, exceeds the engine's child slots per board (2 * n_edges <= e_cap fails;
                   e_cap = max(edges_per_board, E_CAP_FLOOR) as sz_create sizes it);
  * a continued search: sims = 0, nothing pending, descend first (sz_search_begin's descent-only launch), then S simulations as the
    reference makes them.  A search on a fresh root is vlref.Search.run() itself, untouched;
  * an expansion that does not fit in e_cap ends the search with error = "capacity" (SZ_ERR_CAPACITY on the device);
  * choose(): the move choice of k_play (np.random.choice semantics), so host and device are driven by the same uniforms.

Game plays one board ply after ply (begin / run / play).  scenarios() at the end are the inputs both test modules use; coverage() counts,
on the restatement alone, what they must reach.  S = 0 (nothing to search) is not restated."""
import collections

import numpy as np

import vlref
from hashmodel import evaluate_packed, pack_planes

E_CAP_FLOOR = 220                                       # sz_create: never fewer than SZ_MAX_CHILDREN + 2 child slots per board
FALLBACKS = ("unvisited", "leaf", "nodes", "edges")
MAX_MOVES = 218


class CapacityError(Exception):
    pass


def choose(visits, u):
    """k_play's move choice = np.random.choice(p = visits / sum) given the uniform it draws: cumulative f64 sums, divided by the last,
    searchsorted(..., 'right'), clamped; u < 0: the first most visited child (eval.py:92-94)"""
    vis = np.asarray(visits, np.int64)
    if u < 0.0:
        return int(np.argmax(vis))
    cdf = np.cumsum(vis.astype(np.float64) / np.float64(vis.sum()))
    cdf = cdf / cdf[-1]
    return min(int(np.searchsorted(cdf, u, side="right")), len(vis) - 1)


def position_record(game):
    """the 80-byte record of the game's current position (szh_export: the ring entry of its ply)"""
    ring, ply, _ = game.export_ring()
    raw = bytes(ring)
    k = ply & 255
    return raw[k * 80:(k + 1) * 80]


class Search(vlref.Search):
    """vlref.Search (L = 1) with a store that can start from a carried tree"""

    def __init__(self, game, S, edges_per_board, room=0, **kw):
        super().__init__(game, S, L=1, **kw)
        self.kw, self.edges_per_board = dict(kw), int(edges_per_board)
        self.e_cap = max(self.edges_per_board, E_CAP_FLOOR)
        if room:                                         # a carried tree: room for its edges on top of the S expansions of this search
            cap = room + max(self.S, 1) * MAX_MOVES + 2
            for name in ("W", "N", "P", "K", "first", "n", "action", "term", "tval"):
                a = getattr(self, name)
                b = np.full(cap, -1, a.dtype) if name == "first" else np.zeros(cap, a.dtype)
                setattr(self, name, b)
        self.continued = False                           # the search goes on on a kept subtree
        self.kept_edges = self.kept_nodes = 0            # its size at search begin (edge 0 / the root included)
        self.kept_terminal_revisits = 0                  # simulations of this search that ended on a terminal node of the kept subtree
        self.error = None
        self.begin_tree = None                           # tree() when the first network call is due (what sz_debug_tree shows after sz_search_begin)

    def _expand(self, e, pol):
        super()._expand(e, pol)
        if self.n_edges > self.e_cap:
            raise CapacityError()

    @property
    def expansions(self):
        return sum(len(st) for st in self.steps)        # every network row is one expansion

    @property
    def terminal_hits(self):
        return self.sims - self.expansions

    def run(self):
        try:
            if not self.continued:
                self.begin_tree = self.tree()            # a bare root: N = 1
                super().run()
                if not self.steps:                       # a terminal root is finished at search begin
                    self.begin_tree = self.tree()
            else:
                self._run_continued()
        except CapacityError:
            self.error = "capacity"
        return self

    def _run_continued(self):
        pending = None
        while True:
            if pending is not None:
                path, planes = pending
                pol, val = evaluate_packed(planes, self.mode, self.salt)
                self._expand(path[-1], pol)
                self._backprop(path, float(val))
                pending = None
            while self.sims < self.S and pending is None:
                path = self._descend()
                e = path[-1]
                if e in self.games:                      # visited and without children: a terminal position
                    self._backprop(path, float(self.tval[e]))
                    self.kept_terminal_revisits += 1 if e < self.kept_edges else 0
                    continue
                g = self.games[path[-2]].copy()
                g.push_action(int(self.action[e]))
                self.games[e] = g
                v, t = g.get_value_and_terminated()
                self.term[e], self.tval[e] = int(t), int(v) if t else 0
                if t:
                    self._backprop(path, float(v))
                    continue
                pending = (path, self._planes(e))
            if self.begin_tree is None:
                self.begin_tree = self.tree()
            if pending is None:
                return
            self.steps.append(pending[1][None])

    def reroot(self, action, game):
        """-> (the next ply's Search, "reused" or the name of the fall-back).  `game` is the board's game after the move (the root of a fresh search)"""
        fresh = lambda reason: (Search(game, self.S, self.edges_per_board, **self.kw), reason)
        f, k = int(self.first[0]), int(self.n[0])
        c = f + [int(a) for a in self.action[f:f + k]].index(int(action))
        if c not in self.games:
            return fresh("unvisited")
        if self.n[c] == 0:
            return fresh("leaf")
        new = Search(game, self.S, self.edges_per_board, room=self.n_edges, **self.kw)
        new.games = {}

        def copy(src, dst):
            new.W[dst], new.N[dst], new.P[dst] = self.W[src], self.N[src], self.P[src]
            new.action[dst], new.term[dst], new.tval[dst] = self.action[src], self.term[src], self.tval[src]
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
        if 2 * new.n_edges > self.e_cap:
            return fresh("edges")
        new.continued, new.kept_edges, new.kept_nodes = True, new.n_edges, len(new.games)
        return new, "reused"


class Game:
    """One board, ply after ply: begin() -> run() -> play(u).  starts[p] says how ply p's search began: "new" (first ply), "reused" or
    a fall-back's name; counters are cumulative like the engine's (sz_get_stats)."""

    def __init__(self, game, S, edges_per_board, reuse=True, **kw):
        self.game, self.S, self.edges_per_board, self.reuse, self.kw = game.copy(), int(S), int(edges_per_board), bool(reuse), dict(kw)
        self.next = None
        self.search = None
        self.starts, self.searches, self.roots, self.chosen = [], [], [], []      # per ply; roots: the game at search begin
        self.over, self.result, self.error = False, 0, None
        self.last_fallback = None                        # of the move that ended the game (no search follows it)
        self.simulations = self.expansions = self.terminal_hits = 0

    @property
    def live(self):
        return not self.over and self.error is None

    def begin(self):
        self.search, start = self.next if self.next is not None else (Search(self.game, self.S, self.edges_per_board, **self.kw), "new")
        self.next = None
        self.starts.append(start)
        self.searches.append(self.search)
        self.roots.append(self.game.copy())
        return self.search

    def run(self):
        s = self.search.run()
        self.error = s.error
        self.simulations += s.sims
        self.expansions += s.expansions
        self.terminal_hits += s.terminal_hits
        return s

    def play(self, u):
        """sz_play: the training record of this ply (sz_fetch_ply's fields), the move, the game-over test, the subtree kept"""
        acts, vis = self.search.root_children()
        k = len(acts)
        assert k > 0 and vis.sum() > 0, "SZ_ERR_ZERO_VISITS"
        chosen = int(acts[choose(vis, u)])
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
            nxt = self.search.reroot(chosen, self.game)
            if self.over:
                self.last_fallback = nxt[1]
            else:
                self.next = nxt
        return rec


# ---------------------------------------------------------------------------------------------------------------- scenarios
Scenario = collections.namedtuple("Scenario", "name S learning c960 edges_per_board plies boards counted")
Board = collections.namedtuple("Board", "name make mode salt u")
# counted: the scenario's (board, ply) pairs count towards "reuse on at least half of all pairs after ply 0" (scenarios 1 and 2 of the issue)


def _u(b):
    return lambda ply: ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0


def worst_case(S):
    return 2 * S * MAX_MOVES + 2                         # sz_create's default with reuse: no search can overflow


def scenarios():
    import sigma_zero_amd as sz
    import rule_endings as RE
    from test_gpu_parity import FENS
    start = lambda n=None: (lambda: sz.ChessTensor(chess960=n is not None, scharnagl=n))
    fen = lambda i: (lambda: sz.ChessTensor(fen=FENS[i]))
    ending = lambda name: (lambda: RE.build(next(c for c in RE.CASES if c[0] == name))[0])
    greedy = lambda ply: -1.0
    out = []
    # 1. starts, 8 plies: trees compacted up to seven times; sampled moves keep small subtrees, the most visited move keeps large ones
    out.append(Scenario("c960_starts_learning", 64, True, True, worst_case(64), 8,
                        [Board("sp%d" % n, start(n), "dyadic", n, greedy if n % 2 else _u(n)) for n in (0, 17, 518, 959, 333, 702)], True))
    out.append(Scenario("classical_starts", 64, False, False, worst_case(64), 8,
                        [Board("start/%d" % s, start(), "dyadic", s, _u(s) if s % 3 == 0 else greedy) for s in (1, 2, 3, 4, 5, 6)], True))
    # 2. terminal nodes, wide spans, the 75-move rule and ring history inside the kept subtree
    names = {4: "mate_or_stalemate_kqk", 5: "pawn_endgame_e2", 6: "back_rank_mate", 9: "clock_140", 10: "moves_218", 11: "en_passant_root"}
    for learning in (False, True):
        boards = [Board(names[i], fen(i), "dyadic", 10 * i + learning, greedy if learning and i != 10 else _u(i)) for i in sorted(names)]
        boards += [Board(n, ending(n), "dyadic", j, greedy if j % 2 else _u(j)) for j, n in
                   enumerate(("ring_wrap_260_plies", "fivefold_next_move", "threefold_next_move", "clock_148", "window_84_plies"))]
        out.append(Scenario("positions_learning%d" % learning, 48, learning, False, worst_case(48), 6, boards, True))
    # 3. a peaked evaluator: the kept subtree outgrows S nodes ("nodes")
    out.append(Scenario("peaked", 32, False, True, worst_case(32), 7,
                        [Board("sp%d" % n, start(n), "peaked", n, greedy) for n in (5, 77, 400, 811)], False))
    # 4. few child slots: "edges" fires, every search still fits (no error on either side) ...
    out.append(Scenario("few_edges", 32, False, True, 1350, 6,
                        [Board("peaked/sp%d" % n, start(n), "peaked", n, greedy) for n in (5, 77)] +
                        [Board("dyadic/sp%d" % n, start(n), "dyadic", n, _u(n)) for n in (5, 77, 400)], False))
    # ... and searches that do not fit, SZ_ERR_CAPACITY on both sides: a first search on the floor of 220 slots, a continued one on 1350
    out.append(Scenario("overflow_fresh", 24, False, False, 1, 2, [Board("start", start(), "dyadic", 0, greedy)], False))
    out.append(Scenario("overflow_continued", 32, False, True, 1350, 3, [Board("peaked/sp400", start(400), "peaked", 400, greedy)], False))
    # 5. u = 1.0 samples the last child whether it was visited or not ("unvisited"); the mates of scenario 2 end on a visited leaf ("leaf")
    out.append(Scenario("last_child", 12, True, True, worst_case(12), 5,
                        [Board("sp%d" % n, start(n), "dyadic", n, (lambda ply: 1.0 if ply % 2 == 0 else 0.5)) for n in (100, 200, 300)], False))
    return out


def new_game(sc, bd, reuse=True):
    return Game(bd.make(), sc.S, sc.edges_per_board, reuse=reuse, c=2.0, learning=sc.learning, mode=bd.mode, salt=bd.salt)


def play(sc, reuse=True):
    """the restatement alone: every board of the scenario through all its plies; -> the Game objects"""
    games = [new_game(sc, bd, reuse) for bd in sc.boards]
    for ply in range(sc.plies):
        for g, bd in zip(games, sc.boards):
            if g.live:
                g.begin()
                g.run()
                if g.error is None:
                    g.play(bd.u(ply))
    return games


def coverage(played):
    """played: [(Scenario, [Game])] -> the figures of the coverage conditions, counted on the restatement"""
    c = dict(fallbacks=collections.Counter(), pairs=0, reused_pairs=0, widest_kept_span=0, kept_terminal_revisits=0, longest_reused_run=0,
             capacity_errors=0, largest_kept_nodes=0)
    for sc, games in played:
        for g in games:
            run = 0
            for ply, (start, s) in enumerate(zip(g.starts, g.searches)):
                if start in FALLBACKS:
                    c["fallbacks"][start] += 1
                if sc.counted and ply > 0:
                    c["pairs"] += 1
                    c["reused_pairs"] += start == "reused"
                run = run + 1 if start == "reused" else 0
                c["longest_reused_run"] = max(c["longest_reused_run"], run)
                if start == "reused":
                    c["widest_kept_span"] = max(c["widest_kept_span"], int(s.n[:s.kept_edges].max()))
                    c["largest_kept_nodes"] = max(c["largest_kept_nodes"], s.kept_nodes)
                    c["kept_terminal_revisits"] += s.kept_terminal_revisits
            if g.last_fallback in FALLBACKS:
                c["fallbacks"][g.last_fallback] += 1
            c["capacity_errors"] += g.error == "capacity"
    return c


def assert_coverage(c):
    assert all(c["fallbacks"][r] >= 1 for r in FALLBACKS), "every fall-back at least once: %r" % dict(c["fallbacks"])
    assert 2 * c["reused_pairs"] >= c["pairs"] > 0, "reuse on at least half of the (board, ply) pairs after ply 0: %d of %d" % (c["reused_pairs"], c["pairs"])
    assert c["widest_kept_span"] > 64, "a kept node with more than 64 children: widest %d" % c["widest_kept_span"]
    assert c["kept_terminal_revisits"] >= 1, "a terminal node of a kept subtree revisited by the continued search"
    assert c["longest_reused_run"] >= 3, "three consecutive reused plies on one board: longest %d" % c["longest_reused_run"]
    assert c["capacity_errors"] == 2, "the two overflow scenarios overflow, nothing else: %d" % c["capacity_errors"]
