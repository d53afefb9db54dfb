"""Lines and random games for the rule endings, with expectations from the plain statement (tests/plainendings.py).

A line is (name, FEN or None, chess960, history moves, continuation moves, claim).  The history is played into the game (on the device:
the ring, through upload_game); the continuation is walked INSIDE THE TREE on the device (tests/test_gpu_deep_endings.py), so depth d of
a line is tree depth d below the root.  The claim is checked on the plain statement when build() makes the line, as rule_endings.build
does on the oracle: the expectations are the plain statement's and not hand-written numbers.  A claim is a dict:
  over    None: no position of the line, root and continuation, is over; (d, kind): depth d is over by that rule, no depth before it is;
  count   {depth: repetition count}, the number of earlier equal positions (history included);
  clock   {depth: halfmove clock}.
The part of a name before the colon is the line's kind (KINDS); the device test asserts that every kind ran.

build(line, total) continues a line that is not over after its continuation with filler moves, the first legal move in (from, to,
promotion) order, up to `total` plies below the root, so that every board of one device engine has something to play at every
simulation; whatever the filler runs into is told by the plain statement like everything else.

Random games: seeded, moves drawn uniformly from plainrules.legal_moves, from the standard start, three Chess960 starts and eleven
sparse positions: nine endgames (games from those are short and repeat often) and two cages in which only the kings can move, so
that fivefold repetition is reached by chance.  check_coverage() asserts COVERAGE on the plain statement alone.  What SEED and
GAMES_PER_START as committed reach (15 starts, 300 plies at most) stands in test_plain_endings.py's docstring.
"""
import functools
import random

import plainendings as E
import plainrules as P
import rule_endings as RE

# ------------------------------------------------------------------------------------------------ lines
_CYCLE = ["g1f3", "g8f6", "f3g1", "f6g8"]
_SNAKE_FEN = "7k/8/8/8/8/8/8/R6K w - - %d 1"
KINDS = ("cycle", "wrap", "clock", "mate150", "snake", "material", "material_goes_on", "promotion", "identity", "identity960", "chain")


def _cycle_lines():
    seq = _CYCLE * 4                                                    # the start position at plies 0, 4, 8, 12 and 16
    out = []
    for d in range(1, 17):
        claim = {"over": (d, E.FIVEFOLD), "count": {d: 4}}
        if d >= 4:
            claim["count"][d - 4] = 3                                   # one cycle short of fivefold: not over
        out.append(("cycle:fivefold_at_depth_%02d" % d, None, False, seq[:16 - d], seq[16 - d:], claim))
    return out


def _wrap_lines():
    game = RE._long_game()                                              # the last block's base position at plies 248, 252, 256, 260
    more = game + game[-4:]                                             # ... and a fifth time at ply 264
    out = []
    for root in range(247, 260):
        claim = {"over": (264 - root, E.FIVEFOLD), "count": {260 - root: 3, 264 - root: 4}}
        out.append(("wrap:root_at_ply_%d" % root, None, False, more[:root], more[root:], claim))
    return out


def _clock_lines():
    snake = RE._rook_snake()
    out = []
    for d in range(1, 13):
        claim = {"over": (d, E.CLOCK), "clock": {d - 1: 149, d: 150}}
        out.append(("clock:draw_at_depth_%02d" % d, _SNAKE_FEN % (150 - d), False, [], snake[:d], claim))
    mate = ["a1a2", "h8g8", "a2a1", "g8h8", "a1a8"]
    out.append(("mate150:depth_1", "7k/8/6K1/8/8/8/8/R7 w - - 149 100", False, [], mate[-1:], {"over": (1, E.MATE), "clock": {1: 150}}))
    out.append(("mate150:depth_5", "7k/8/6K1/8/8/8/8/R7 w - - 145 100", False, [], mate, {"over": (5, E.MATE), "clock": {4: 149, 5: 150}}))
    for root in (70, 80, 83):
        claim = {"over": None, "count": {84 - root: 1, 83 - root: 0}, "clock": {84 - root: 84}}
        out.append(("snake:root_%d_plies_in" % root, _SNAKE_FEN % 0, False, snake[:root], snake[root:], claim))
    return out


# a capture by White at depth 1, 2, 5 or 9: the men shuffle in front of it (king h1-g1-h1, king a8-a7-a8); at depth 2 Black moves first
_W, _B = ["h1g1", "g1h1"], ["a8a7", "a7a8"]
_PREFIX = {1: ("w", []), 2: ("b", [_B[0]]), 5: ("w", [_W[0], _B[0], _W[1], _B[1]]), 9: ("w", [_W[0], _B[0], _W[1], _B[1]] * 2)}


def _capture_lines(kind, name, placement, capture, over, depths):
    out = []
    for d in depths:
        side, prefix = _PREFIX[d]
        claim = {"over": (d, E.MATERIAL) if over else None, "clock": {d: 0}}
        out.append(("%s:%s_at_depth_%d" % (kind, name, d), "%s %s - - 0 1" % (placement, side), False, [], prefix + [capture], claim))
    return out


def _material_lines():
    out = []
    out += _capture_lines("material", "kb_v_k", "k7/8/8/8/8/8/1n6/2B4K", "c1b2", True, (1, 2, 5, 9))
    out += _capture_lines("material", "kn_v_k", "k7/8/8/8/8/1r6/8/2N4K", "c1b3", True, (1, 2, 5, 9))
    out += _capture_lines("material", "same_coloured_bishops", "kb6/8/8/8/8/8/1n6/2B4K", "c1b2", True, (1, 2, 5, 9))
    out += _capture_lines("material_goes_on", "opposite_bishops", "k1b5/8/8/8/8/8/1n6/2B4K", "c1b2", False, (1, 2, 5, 9))
    out += _capture_lines("material_goes_on", "knn_v_k", "k7/8/8/8/8/1r6/8/2N1N2K", "c1b3", False, (2, 9))
    out += _capture_lines("material_goes_on", "kn_v_kq", "kq6/8/8/8/8/1r6/8/2N4K", "c1b3", False, (2, 9))
    for piece, over in (("n", True), ("b", True), ("r", False), ("q", False)):
        claim = {"over": (3, E.MATERIAL) if over else None, "clock": {2: 2, 3: 0}}
        out.append(("promotion:e8%s_at_depth_3" % piece, "8/4P3/8/8/8/8/k7/7K w - - 0 1", False, [], ["h1g1", "a2a3", "e7e8" + piece], claim))
    return out


def _identity_lines():
    out = []
    claim = {"over": None, "count": {4: 0, 8: 1}}                     # 4: the placement of the root again, but the rights are gone; 8 equals 4
    out.append(("identity:king_out_and_back_loses_the_rights", None, False, ["e2e4", "e7e5"],
                ["e1e2", "e8e7", "e2e1", "e7e8", "e1e2", "e8e7", "e2e1", "e7e8"], claim))
    out.append(("identity:rook_out_and_back_loses_one_right", None, False, ["a2a4", "a7a5"],
                ["a1a2", "a8a7", "a2a1", "a7a8", "a1a2", "a8a7", "a2a1", "a7a8"], claim))
    # Scharnagl 0 is BBQNNRKR: rooks on f and h, the king on g
    out.append(("identity960:rook_out_and_back_loses_one_right", P.scharnagl_fen(0), True, ["h2h4", "h7h5"],
                ["h1h2", "h8h7", "h2h1", "h7h8", "h1h2", "h8h7", "h2h1", "h7h8"], claim))
    out.append(("identity960:king_out_and_back_loses_the_rights", P.scharnagl_fen(0), True, ["g2g3", "g7g6"],
                ["g1g2", "g8g7", "g2g1", "g7g8", "g1g2", "g8g7", "g2g1", "g7g8"], claim))
    out.append(("identity960:knight_cycle_on_start_617", P.scharnagl_fen(617), True, [], None, None))      # filled in below
    # d7d5 next to the pawn on e5: exd6 is legal at depth 1, so the same placement at depth 5 is another position; 9 equals 5
    out.append(("identity:double_push_with_a_legal_capture", None, False, ["e2e4", "a7a6", "e4e5"],
                ["d7d5"] + ["g1f3", "g8f6", "f3g1", "f6g8"] * 2, {"over": None, "count": {1: 0, 5: 0, 9: 1}}))
    # e2e4 with no black pawn near: the square e3 is recorded and means nothing
    out.append(("identity:double_push_nobody_can_capture", None, False, [],
                ["e2e4", "g8f6", "g1f3", "f6g8", "f3g1"], {"over": None, "count": {1: 0, 5: 1}}))
    # d7d5 next to the pawn on e5, which the rook on e8 pins to its king: exd6 is illegal, so the positions are equal
    out.append(("identity:double_push_capturer_is_pinned", "4r2k/3p4/8/4P3/8/8/8/4K2N b - - 0 1", False, [],
                ["d7d5", "h1g3", "h8g8", "g3h1", "g8h8"], {"over": None, "count": {1: 0, 5: 1}}))
    return out


def _knight_cycle_960(n):
    """a four-ply knight cycle from Chess960 start n, four times over: fivefold at depth 16, all of it inside the tree"""
    pos = P.scharnagl_start(n)
    cyc = []
    for _ in range(2):                                                  # a white knight out, a black knight out
        m = sorted(m for m in P.legal_moves(pos) if pos.board[m[0]] in "Nn")[0]
        cyc.append(m)
        pos = P.make(pos, m)
    cyc += [(m[1], m[0], 0) for m in cyc]
    return [P.move_name(m) for m in cyc] * 4


def _chain_lines():
    snake = RE._rook_snake()                                            # 84 reversible plies, no position twice before the last
    return [("chain:%d_quiet_plies" % s, _SNAKE_FEN % 0, False, [], snake[:s], {"over": None, "clock": {s: s}, "count": {s: 0}}) for s in (8, 40)]


def _all_lines():
    out = _cycle_lines() + _wrap_lines() + _clock_lines() + _material_lines() + _identity_lines() + _chain_lines()
    for i, line in enumerate(out):
        if line[4] is None:
            out[i] = line[:4] + (_knight_cycle_960(617), {"over": (16, E.FIVEFOLD), "count": {12: 3, 16: 4}})
    assert len({l[0] for l in out}) == len(out) and {kind_of(l) for l in out} == set(KINDS)
    return out


def kind_of(line):
    return line[0].split(":")[0]


class Built:
    """A line on the plain statement: .game holds history, continuation and filler; depth d of the line is ply .root + d of .game"""

    def __init__(self, line, game, root, scripted):
        self.line, self.name, self.kind, self.fen, self.chess960 = line, line[0], kind_of(line), line[1], line[2]
        self.game, self.root, self.scripted = game, root, scripted     # scripted: plies of the continuation (the rest is filler)
        self.depths = len(game) - root                                  # the deepest position there is
        over = [d for d in range(self.depths + 1) if game.outcome(root + d)]
        self.over_depth = over[0] if over else None
        assert self.over_depth in (None, self.depths), "%s: the line goes on after the game is over" % self.name

    def at(self, d):
        """(position, legal moves, outcome or None, is_repetition(2), is_repetition(3), halfmove clock) at depth d"""
        g, p = self.game, self.root + d
        return g.pos[p], g.legal[p], g.outcome(p), g.is_repetition(2, p), g.is_repetition(3, p), g.clock[p]

    def move(self, d):
        """the move played at depth d (it leads to depth d + 1)"""
        return self.game.moves[self.root + d]


def check_claim(name, game, root, n, claim):
    """the claim on the plain game `game`, whose plies root .. root + n are the line's depths 0 .. n"""
    over = claim["over"]
    for d in range(n + 1):
        o = game.outcome(root + d)
        if over and d == over[0]:
            assert o and o[0] == over[1], "%s: depth %d should be over by %s, the plain statement says %s" % (name, d, over[1], o)
            assert o[1] == (-1 if over[1] == E.MATE else 0)
        else:
            assert o is None, "%s: depth %d should not be over, the plain statement says %s" % (name, d, o)
    assert not over or over[0] == n, "%s: the continuation does not end where the game does" % name
    for d, c in claim.get("count", {}).items():
        got = game.repetition_count(root + d)
        assert got == c, "%s: depth %d should have %d earlier equal positions, the plain statement counts %d" % (name, d, c, got)
        assert game.is_repetition(c + 1, root + d) and not game.is_repetition(c + 2, root + d)
    for d, c in claim.get("clock", {}).items():
        assert game.clock[root + d] == c, "%s: depth %d should have clock %d, the plain statement has %d" % (name, d, c, game.clock[root + d])


def build(line, total=None, rules=E.RULES, claims=True):
    """the line on the plain statement, its claim asserted; with `total`, continued by filler moves to `total` plies below the root
    unless the game ends before.  claims=False (the teeth tests, with wrong rules) leaves the claim alone and stops where those rules
    end the game."""
    name, fen, _, history, continuation, claim = line
    game = E.Game(fen, rules)
    for u in history:
        game.push_uci(u)
    root = len(game)
    for u in continuation:
        if claims or game.outcome() is None:
            game.push_uci(u)
    if claims:
        check_claim(name, game, root, len(continuation), claim)
    while total is not None and len(game) - root < total and game.outcome() is None:
        game.push(sorted(game.legal[-1])[0])
    return Built(line, game, root, len(continuation))


LINES = _all_lines()


# ------------------------------------------------------------------------------------------------ the same game on the host mirror
def host_game(fen, chess960):
    import sigma_zero_amd as sz
    if fen is None:
        return sz.ChessTensor()
    return sz.ChessTensor(chess960=chess960, fen=fen)


def host_spelling(pos, m, chess960):
    """a plain move as the host mirror and the oracle spell it: king takes own rook with chess960, the king's two-square move without"""
    return m if chess960 else E.standard_spelling(pos, m)


def host_actions(ct):
    """{(from, to, promotion): action index} of the host mirror's legal moves"""
    import ctypes as C
    from sigma_zero_amd import _native as N
    out = {}
    f, t, p = C.c_int32(), C.c_int32(), C.c_int32()
    decode, g, rf, rt, rp = N.lib().szh_action_to_move, ct._g, C.byref(f), C.byref(t), C.byref(p)
    acts = ct.legal_action_indices()
    for a in acts:
        assert decode(g, a, rf, rt, rp) == N.SZ_OK
        out[(f.value, t.value, p.value)] = a
    assert len(out) == len(acts), "two action indices decode to one move"
    return out

# ------------------------------------------------------------------------------------------------ random games
SEED = 20240607
MAX_PLIES = 300
STARTS = [
    ("start", None, False), ("c960_0", P.scharnagl_fen(0), True), ("c960_617", P.scharnagl_fen(617), True), ("c960_959", P.scharnagl_fen(959), True),
    ("kr_v_k", "8/8/8/4k3/8/8/8/R3K3 w - - 0 1", False), ("kbn_v_k", "8/8/8/4k3/8/8/8/1NB1K3 w - - 0 1", False),
    ("kp_v_k", "8/8/8/4k3/8/8/4P3/4K3 w - - 0 1", False), ("kb_v_kn", "8/8/3nk3/8/8/8/8/2B1K3 w - - 0 1", False),
    ("kq_v_k", "8/8/8/4k3/8/8/8/3QK3 w - - 0 1", False), ("kr_v_kr_with_rights", "4k2r/8/8/8/8/8/8/R3K3 w Qk - 0 1", False),
    ("knn_v_kp", "8/8/8/4k3/7p/8/8/1N2K1N1 w - - 0 1", False), ("pawns", "4k3/2p1p3/8/3P4/3p4/8/2P1P3/4K3 w - - 0 1", False),
    ("kqq_v_k", "8/8/8/4k3/8/8/8/2QQK3 w - - 0 1", False),
    # locked pawns and bishops that cannot move: each king walks three (five) squares of its back rank and nothing else ever moves
    ("cage_3", "2bk2b1/1p1p1p1p/1P1P1P1P/8/8/1p1p1p1p/1P1P1P1P/2BK2B1 w - - 0 1", False),
    ("cage_5", "2bk4/1p1p1p1p/1P1P1P1P/8/8/1p1p1p1p/1P1P1P1P/2BK4 w - - 0 1", False),
]
GAMES_PER_START = {"start": 6, "c960_0": 3, "c960_617": 3, "c960_959": 3, "kqq_v_k": 90}
GAMES_PER_SPARSE_START = 30
# at least: a game ended by each rule; positions with two or more earlier equal ones; a game longer than the device's ring
COVERAGE = (("ended by " + k, 1) for k in E.KINDS)
COVERAGE = tuple(COVERAGE) + (("positions with a repetition count >= 2", 50), ("games longer than 256 plies", 1))


@functools.lru_cache(maxsize=None)
def random_games():
    """[(start name, FEN or None, chess960, plain Game)]"""
    rng = random.Random(SEED)
    out = []
    for name, fen, c960 in STARTS:
        for _ in range(GAMES_PER_START.get(name, GAMES_PER_SPARSE_START)):
            g = E.Game(fen)
            while g.outcome() is None and len(g) < MAX_PLIES:
                g.push(rng.choice(g.legal[-1]))
            out.append((name, fen, c960, g))
    return out


def reached(games):
    """what the games reached, under the names of COVERAGE, and the totals"""
    got = {name: 0 for name, _ in COVERAGE}
    got["games"], got["positions"] = len(games), 0
    for _, _, _, g in games:
        o = g.outcome()
        if o:
            got["ended by " + o[0]] += 1
        got["games longer than 256 plies"] += len(g) > 256
        got["positions"] += len(g) + 1
        seen = {}
        for i in g.ids:                                                 # the full-history count of every ply in one pass
            got["positions with a repetition count >= 2"] += seen.get(i, 0) >= 2
            seen[i] = seen.get(i, 0) + 1
    return got


def check_coverage(games):
    got = reached(games)
    for name, least in COVERAGE:
        assert got[name] >= least, "random games: %s: %d, at least %d wanted (change the starts, not the cap): %s" % (name, got[name], least, got)
    return got
