"""Plain-Python restatement of sz_play_moves (include/sigmazero.h): a GIVEN move played on a board, and the re-rooting of the board's tree
that goes with it on a reuse_subtree engine.  It is what k_play_moves (csrc/sz_engine.hip) is held to, bit for bit, ply after ply
(tests/test_gpu_play_moves.py).  Built on tests/reuseref.py, which it imports and does not change:

  * Search.keep(action, game): reuseref.Search.reroot's recursive copy of a root child's subtree into a new store, WITHOUT the "nodes" and
    "edges" conditions.  The device evaluates those two in k_search_begin, on whatever is kept after the LAST re-rooting: a subtree too
    large after sz_play can fit again after the sz_play_moves that follows.  Game.begin() applies them there.  (Where reroot answers
    "reused", keep gives the same store: tests/test_play_moves_ref.py.)  keep does not assume that the action is among the root's
    children: expansion drops legal moves whose renormalised prior is exactly 0 ("dropped_move").
  * Game.play_move(action): legality with the host mirror (an illegal move is the sticky error "invalid" and changes nothing), the move,
    the game-over test, and the tree: the board has one when a search has finished on it and no move was played since (Game.done), or
    when an earlier play() / play_move() kept a subtree no search has continued yet (Game.kept).  The fall-backs to a fresh root, by name:
      "no_tree"       nothing to re-root (no search yet, or the last re-rooting kept nothing),
      "dropped_move"  the move is legal and not among the root's children,
      "unvisited"     its child was never visited,
      "leaf"          it was visited and has no children: a terminal position, the game is over,
      "over"          the game has ended and the board had no tree to name another reason by;
    Game.play(u) re-roots the same way, so a play() followed by a play_move() is a two-ply re-rooting (Game.rerooted == 2) and the next
    search continues on the grandchild's subtree.
  * a given move is no search of the mover: no counter moves, no record is made.

scenarios() are the inputs of both test modules: boards of reuseref.scenarios(), each tracked by two Games, sides A and B, with networks
of their own (salts), each searching only when it is to move (or, with ponder, also on the opponent's time) and taking the other's move
through play_move.  A Script can replace the mover's choice by a move picked on the restatement (a dropped move, an unvisited child, a move
that ends the game); both sides then take it through play_move, the mover on its finished search.  coverage() counts what they reach."""
import collections

import numpy as np

import reuseref as R
from hashmodel import evaluate_packed, pack_planes

FALLBACKS = ("no_tree", "dropped_move", "unvisited", "leaf", "over")


class Search(R.Search):
    def keep(self, action, game):
        """-> (the Search that holds the subtree below the root child `action`, "kept"), or (None, the fall-back's name)"""
        f, k = int(self.first[0]), int(self.n[0])
        acts = [int(a) for a in self.action[f:f + k]] if f >= 0 else []
        if int(action) not in acts:
            return None, "dropped_move"
        c = f + acts.index(int(action))
        if c not in self.games:
            return None, "unvisited"
        if self.n[c] == 0:
            return None, "leaf"
        new = Search(game, self.S, self.edges_per_board, room=self.n_edges, **self.kw)
        new.games = {}

        def copy(src, dst):                                  # reuseref.Search.reroot's copy: children in order, each node's in one contiguous span
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
        new.continued, new.kept_edges, new.kept_nodes = True, new.n_edges, len(new.games)
        return new, "kept"

    def fits(self):
        """k_search_begin's conditions on a kept subtree: None, or the fall-back's name (reuseref: "nodes", "edges")"""
        if len(self.games) > self.S:
            return "nodes"
        if 2 * self.n_edges > self.e_cap:
            return "edges"
        return None


class Game(R.Game):
    """reuseref.Game with play_move().  done: the finished search no move has consumed; kept: the subtree the last re-rooting kept;
    rerooted: re-rootings behind `kept` since the last search.  begins[i] describes search i: (start, rerooted, had_kept)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.done = self.kept = None
        self.rerooted = 0
        self.reason = "new"
        self.fallbacks = collections.Counter()
        self.moves = []                                      # per play_move: (action, outcome, a finished search was re-rooted)
        self.begins = []

    def begin(self):
        start, s = self.reason, None
        if self.kept is not None:
            start = self.kept.fits() or "reused"
            if start == "reused":
                s = self.kept
            else:
                self.fallbacks[start] += 1
        self.begins.append((start, self.rerooted if self.kept is not None else 0, self.kept is not None))
        self.search = s if s is not None else Search(self.game, self.S, self.edges_per_board, **self.kw)
        self.kept = self.done = None
        self.rerooted = 0
        self.starts.append(start)
        self.searches.append(self.search)
        self.roots.append(self.game.copy())
        return self.search

    def run(self):
        s = super().run()
        self.done = s if s.error is None else None
        return s

    def _reroot(self, action):
        tree, self.done = (self.done if self.done is not None else self.kept), None
        if not self.reuse:
            self.kept = None
            return None
        if tree is None:
            kept, reason = None, "over" if self.over else "no_tree"
        else:
            kept, reason = tree.keep(action, self.game)
            assert not (self.over and kept is not None), "a position that ends the game has no children"
        self.kept = kept
        self.rerooted = self.rerooted + 1 if kept is not None else 0
        self.reason = "new" if kept is not None else reason
        if kept is None:
            self.fallbacks[reason] += 1
        return reason

    def play(self, u):
        reuse, self.reuse = self.reuse, False                # reuseref's play() without its re-rooting ...
        try:
            rec = super().play(u)
        finally:
            self.reuse = reuse
        self._reroot(rec["chosen"])                          # ... then this module's
        return rec

    def play_move(self, action):
        """sz_play_moves on this board -> None (the board is left alone: game over or in error), "invalid", "kept" or a fall-back's name"""
        if not self.live:
            return None
        if int(action) < 0:
            return None
        if int(action) not in self.game.legal_action_indices():
            self.error = "invalid"
            return "invalid"
        had = self.done is not None
        self.game.push_action(int(action))
        v, t = self.game.get_value_and_terminated()
        self.over = bool(t)
        self.result = 0 if not (t and v) else (-1 if self.game.board.turn else 1)
        out = self._reroot(action)
        self.moves.append((int(action), out, had))
        return out


# ---------------------------------------------------------------------------------------------------------------- scenarios
Scenario = collections.namedtuple("Scenario", "name S learning c960 edges_per_board plies boards ponder script salt_b")
# script: {(board name, ply): kind} replaces the mover's choice at that ply by pick(kind, ...); both sides then take the move by play_move
# salt_b: side B's network is side A's with salt + salt_b (0: the same network, so each side's tree has thought about the other's reply)


def pick(kind, mover):
    """a move for Script, chosen on the restatement: mover is the Game that has just searched the position"""
    g, s = mover.game, mover.search
    legal = [int(a) for a in g.legal_action_indices()]
    acts, vis = s.root_children()
    acts = [int(a) for a in acts]
    if kind == "dropped":                                    # legal, and expansion dropped it (prior exactly 0)
        return next(a for a in legal if a not in acts)
    if kind == "unvisited":
        return next(a for a, n in zip(acts, vis) if n == 0)
    if kind == "ending":                                     # a move that ends the game
        for a in legal:
            c = g.copy()
            c.push_action(a)
            if c.get_value_and_terminated()[1]:
                return a
        return None                                          # none: the mover plays its own choice
    raise KeyError(kind)


def dropped_starts(mode="dyadic", want=3, salt=None):
    """Chess960 starts (Scharnagl numbers) whose root expansion drops a legal move under the hash model with salt = the number, or `salt`"""
    import sigma_zero_amd as sz
    out = []
    for n in range(960):
        g = sz.ChessTensor(chess960=True, scharnagl=n)
        pol, _ = evaluate_packed(pack_planes(g.get_representation().numpy()), mode, n if salt is None else salt)
        if any(pol[a] == 0 for a in g.legal_action_indices()):
            out.append(n)
            if len(out) == want:
                break
    return out


def scenarios():
    base = {sc.name: sc for sc in R.scenarios()}
    by = lambda sc, names: [bd for bd in sc.boards if bd.name in names]
    greedy = lambda ply: -1.0
    g = lambda bd: bd._replace(u=greedy)
    out = []
    # 1. alternating play from Chess960 starts, greedy: a side's searches after its first continue on a grandchild's subtree
    sc = base["c960_starts_learning"]
    out.append(Scenario("alternate_c960", 64, False, True, R.worst_case(64), 8, [g(bd) for bd in sc.boards[:6]], False, {}, 0))
    # 2. a peaked evaluator: the subtree below the move played outgrows S nodes and fits again below the reply ("nodes" is decided at search begin)
    pk = base["peaked"]
    out.append(Scenario("alternate_peaked", 32, False, True, R.worst_case(32), 8, pk.boards, False, {}, 0))
    # 3. sampled moves, learning on, networks that differ: small kept subtrees, replies the tree has not visited
    out.append(Scenario("alternate_sampled", 32, True, True, R.worst_case(32), 6, sc.boards[:4], False, {}, 7001))
    # 4. positions: the 218-move position (kept spans wider than 64), mates one ply away, the 75-move rule, ring history
    sp = base["positions_learning0"]
    names = ("moves_218", "mate_or_stalemate_kqk", "back_rank_mate", "clock_140", "en_passant_root", "ring_wrap_260_plies", "fivefold_next_move", "clock_148")
    out.append(Scenario("positions", 48, False, False, R.worst_case(48), 6, [g(bd) for bd in by(sp, names)], False, {}, 0))
    # 5. pondering: the receiver has searched the position too, so play_move re-roots a finished search (one-ply re-rooting)
    out.append(Scenario("ponder", 24, False, True, R.worst_case(24), 6, [g(bd) for bd in sc.boards[:4]] + [g(bd) for bd in by(sp, ("back_rank_mate", "moves_218"))],
                        True, {}, 7001))
    # 6. the 218-move position again, with networks under which the move played does not mate: the kept grandchild has spans of 190 and more
    wide = by(sp, ("moves_218",))[0]
    out.append(Scenario("wide", 32, False, False, R.worst_case(32), 4, [g(wide)._replace(name="moves_218/%d" % k, salt=k) for k in (0, 1, 3, 5)], False, {}, 0))
    # 7. scripted moves: a dropped move (Chess960 starts whose root expansion drops one), an unvisited child, a move that ends the game
    import sigma_zero_amd as sz
    start = lambda n: (lambda: sz.ChessTensor(chess960=True, scharnagl=n))
    boards = [R.Board("drop%d" % n, start(n), "dyadic", n, greedy) for n in dropped_starts()]
    script = {(bd.name, 0): "dropped" for bd in boards}
    script.update({(bd.name, 3): "unvisited" for bd in boards})
    mates = [g(bd) for bd in by(sp, ("back_rank_mate", "mate_or_stalemate_kqk"))]
    script.update({(bd.name, 0 if bd.name == "back_rank_mate" else 2): "ending" for bd in mates})
    out.append(Scenario("scripted", 16, False, True, R.worst_case(16), 5, boards + mates, False, script, 0))
    return out


def new_games(sc, bd, reuse=True):
    """sides A and B of one board: the same game, networks of their own"""
    mk = lambda salt: Game(bd.make(), sc.S, sc.edges_per_board, reuse=reuse, c=2.0, learning=sc.learning, mode=bd.mode, salt=salt)
    return mk(bd.salt), mk(bd.salt + sc.salt_b)


def side_to_move(ply):
    return ply % 2                                           # side A searches at the scenario's even plies, whatever colour that is


def ply_of(sc, bd, ply, sides):
    """one ply of one board on the restatement -> (mover, searched: [bool, bool], the move both sides end up with, how: "play" / "given")"""
    m = side_to_move(ply)
    mover, other = sides[m], sides[1 - m]
    searched = [False, False]
    if not mover.live:
        return m, searched, -1, None
    mover.begin()
    mover.run()
    searched[m] = True
    if sc.ponder and other.live:
        other.begin()
        other.run()
        searched[1 - m] = True
    kind = sc.script.get((bd.name, ply))
    a = pick(kind, mover) if kind is not None else None
    if a is not None:
        mover.play_move(a)
        other.play_move(a)
        return m, searched, a, "given"
    rec = mover.play(bd.u(ply))
    other.play_move(rec["chosen"])
    return m, searched, rec["chosen"], "play"


def play(sc, reuse=True):
    """the restatement alone -> [(Game A, Game B)] per board"""
    games = [new_games(sc, bd, reuse) for bd in sc.boards]
    for ply in range(sc.plies):
        for sides, bd in zip(games, sc.boards):
            ply_of(sc, bd, ply, sides)
            assert R.position_record(sides[0].game) == R.position_record(sides[1].game)
    return games


def coverage(played):
    """played: [(Scenario, [(Game, Game)])] -> the figures of the coverage conditions, counted on the restatement"""
    c = dict(fallbacks=collections.Counter(), two_ply_chances=0, two_ply_continued=0, widest_grandchild_span=0, longest_two_ply_run=0,
             moves_on_finished_search=0, kept_on_finished_search=0, largest_kept_nodes=0, begin_fallbacks=collections.Counter())
    for sc, games in played:
        for sides in games:
            for g in sides:
                for r in FALLBACKS:
                    c["fallbacks"][r] += g.fallbacks[r]
                for r in R.FALLBACKS:
                    c["begin_fallbacks"][r] += g.fallbacks[r]
                c["moves_on_finished_search"] += sum(1 for _, _, had in g.moves if had)
                c["kept_on_finished_search"] += sum(1 for _, out, had in g.moves if had and out == "kept")
                run = 0
                for i, ((start, rerooted, had_kept), s) in enumerate(zip(g.begins, g.searches)):
                    if i == 0 or sc.ponder:
                        continue                             # a side's first search has no play() behind it; pondering re-roots one ply at a time
                    c["two_ply_chances"] += 1
                    two = start == "reused" and rerooted == 2
                    c["two_ply_continued"] += two
                    run = run + 1 if two else 0
                    c["longest_two_ply_run"] = max(c["longest_two_ply_run"], run)
                    if two:
                        c["widest_grandchild_span"] = max(c["widest_grandchild_span"], int(s.n[:s.kept_edges].max()))
                        c["largest_kept_nodes"] = max(c["largest_kept_nodes"], s.kept_nodes)
    return c


def assert_coverage(c):
    assert all(c["fallbacks"][r] >= 1 for r in FALLBACKS), "every fall-back at least once: %r" % dict(c["fallbacks"])
    assert 2 * c["two_ply_continued"] >= c["two_ply_chances"] > 0, "a two-ply re-rooting is followed by a continued search on at least half of the plies " \
        "where it could be: %d of %d" % (c["two_ply_continued"], c["two_ply_chances"])
    assert c["widest_grandchild_span"] > 64, "a kept grandchild node with more than 64 children: widest %d" % c["widest_grandchild_span"]
    assert c["longest_two_ply_run"] >= 3, "three two-ply re-rootings in a row on one side: longest %d" % c["longest_two_ply_run"]
    assert c["moves_on_finished_search"] >= 1 and c["kept_on_finished_search"] >= 1, "a play_move on a board with a finished search"
