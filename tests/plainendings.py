"""The rules that end a game or count a repetition, stated plainly on top of tests/plainrules.py: the second, independent statement
that the host mirror (csrc/sz_chess.h), the oracle (oracle/oc_chess.c) and, at depth in the tree, the device are held to
(tests/ending_lines.py, tests/test_plain_endings.py, tests/test_gpu_deep_endings.py).

Plain Python over plainrules.Position: no bitboards, no hash, nothing of the project imported.  Written from the rules as python-chess
documents them (Board.is_repetition, Board._transposition_key, Board.is_seventyfive_moves, Board.is_fivefold_repetition,
Board.has_insufficient_material, Board.outcome), not from sz_chess.h or oc_chess.c.

Identity of a position (what "the same position" means for a repetition): the placement, the side to move, the set of rook squares that
still carry a castling right, and the en-passant square ONLY IF a legal en-passant capture exists, which plainrules.legal_moves decides.
The halfmove clock and the move number are not part of it.

Repetition count: the number of EARLIER positions of the whole game list whose identity equals the current one.  No reversible window,
no irreversible-move flag, no ring, no cap.  That is a deliberate simplification of python-chess's walk-back, which stops at the first
irreversible move (a pawn move, a capture, a move that reduces the castling rights, or a move made where an en-passant capture was
legal).  The two counts are equal, because each of those moves changes the identity for good: a pawn never moves backwards and a
captured man never returns, so the placement before it is gone; a lost right never comes back, so the rights component differs ever
after; and an identity that carries an en-passant square can be reached only by the double push that has just been made.  No position
before an irreversible move can therefore equal one after it.  Game.windowed_count() is the count restricted to the plies since the
last pawn move, capture or loss of a right; tests/test_plain_endings.py checks on tens of thousands of positions that it equals
Game.repetition_count().  is_repetition(n) is count + 1 >= n.

Halfmove clock: kept by the game itself, from the FEN's fifth field; reset on a pawn move or a capture, one more otherwise.

Material, per side, as a list of cases (python-chess: "guaranteed to return False if the side can still win"):
  * any pawn, rook or queen of the side: sufficient;
  * a knight: insufficient only if the side is exactly K+N and the opponent has nothing but king and queens (any other man of the
    opponent's could block its own king's flight square);
  * only bishops: insufficient only if every bishop on the board, of either colour, stands on one square colour, and the board has no
    pawn and no knight;
  * bare king: insufficient.
The game is drawn when both sides are insufficient.  MATE_WITNESSES anchors the "sufficient" direction of that table: for every pawnless
signature of at most four men that the table calls sufficient for a side, one position in which that side HAS mated, checked with
plainrules.is_checkmate.  The "insufficient" direction (that no mate exists with K+N v K+Q, say) stays a restatement of python-chess.

Game over and result, in this order: checkmate (the side to move loses: -1); stalemate; draw by material; clock >= 150 with at least one
legal move; fivefold repetition (all 0).  Mate delivered by the move that takes the clock to 150 is a win, not a draw.
"""
import plainrules as P

START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
MATE, STALEMATE, MATERIAL, CLOCK, FIVEFOLD = "mate", "stalemate", "material", "75 moves", "fivefold"
KINDS = (MATE, STALEMATE, MATERIAL, CLOCK, FIVEFOLD)


def square_is_dark(sq):
    return ((sq & 7) + (sq >> 3)) % 2 == 0                             # a1 is dark


class Rules:
    """The statement itself.  A class so that tests/test_plain_endings.py can show that the checks have teeth by overriding one clause
    in a copy; nothing else subclasses it."""
    CLOCK_LIMIT = 150
    FOLD = 5

    def legal_en_passant(self, pos, legal):
        return any(m[1] == pos.ep and pos.board[m[0]] in "Pp" and (m[1] - m[0]) % 8 != 0 for m in legal) if pos.ep is not None else False

    def identity(self, pos, legal):
        return (tuple(pos.board), pos.white, frozenset(pos.rights), pos.ep if self.legal_en_passant(pos, legal) else None)

    def insufficient_side(self, board, white):
        mine = [c for c in board if c != "." and c.isupper() == white]
        theirs = [c for c in board if c != "." and c.isupper() != white]
        kinds = sorted(c.upper() for c in mine)
        if any(k in "PRQ" for k in kinds):
            return False
        if "N" in kinds:
            return kinds == ["K", "N"] and all(c.upper() in "KQ" for c in theirs)
        if "B" in kinds:
            colours = {square_is_dark(s) for s in range(64) if board[s] in "Bb"}
            return len(colours) == 1 and not any(c in "PpNn" for c in board)
        return True

    def insufficient(self, board):
        return self.insufficient_side(board, True) and self.insufficient_side(board, False)

    def outcome(self, pos, legal, clock, count):
        """None while the game goes on, else (kind, value for the side to move)"""
        if not legal:
            return (MATE, -1) if P.in_check(pos) else (STALEMATE, 0)
        if self.insufficient(pos.board):
            return (MATERIAL, 0)
        if clock >= self.CLOCK_LIMIT:
            return (CLOCK, 0)
        if count + 1 >= self.FOLD:
            return (FIVEFOLD, 0)
        return None


RULES = Rules()


class Game:
    """A whole game: every position since the FEN, with its legal moves, clock and identity."""

    def __init__(self, fen=None, rules=RULES):
        fen = fen or START_FEN
        parts = fen.split()
        self.rules = rules
        self.pos = [P.from_fen(fen)]
        self.clock = [int(parts[4]) if len(parts) > 4 else 0]
        self.moves = []
        self.resets = [False]                                           # ply i was reached by a pawn move, a capture or a move that lost a right
        self.legal = [P.legal_moves(self.pos[0])]
        self.ids = [rules.identity(self.pos[0], self.legal[0])]

    def retold(self, rules):
        """the same game under other rules: positions and legal moves are shared, identities are told again"""
        g = Game.__new__(Game)
        g.rules, g.pos, g.clock, g.moves, g.resets, g.legal = rules, self.pos, self.clock, self.moves, self.resets, self.legal
        g.ids = [rules.identity(p, l) for p, l in zip(self.pos, self.legal)]
        return g

    def copy(self):
        g = Game.__new__(Game)
        g.rules = self.rules
        g.pos, g.clock, g.moves, g.resets, g.legal, g.ids = (list(x) for x in (self.pos, self.clock, self.moves, self.resets, self.legal, self.ids))
        return g

    def __len__(self):
        return len(self.moves)

    def push(self, m):
        pos = self.pos[-1]
        if m not in self.legal[-1]:
            raise ValueError("illegal move %s in %s" % (P.move_name(m), pos.placement()))
        pawn = pos.board[m[0]] in "Pp"
        capture = pos.board[m[1]] != "." and not P.is_castling(pos, m)  # en passant is a pawn move already
        nxt = P.make(pos, m)
        self.moves.append(m)
        self.pos.append(nxt)
        self.clock.append(0 if pawn or capture else self.clock[-1] + 1)
        self.resets.append(pawn or capture or nxt.rights != pos.rights)
        self.legal.append(P.legal_moves(nxt))
        self.ids.append(self.rules.identity(nxt, self.legal[-1]))

    def push_uci(self, u):
        self.push(from_uci(u))

    def repetition_count(self, ply=None):
        ply = len(self.moves) if ply is None else ply
        me = self.ids[ply]
        return sum(1 for i in range(ply) if self.ids[i] == me)

    def windowed_count(self, ply=None):
        """the same count over the plies since the last pawn move, capture or loss of a right only"""
        ply = len(self.moves) if ply is None else ply
        first = max([i for i in range(ply + 1) if self.resets[i]] or [0])
        me = self.ids[ply]
        return sum(1 for i in range(first, ply) if self.ids[i] == me)

    def is_repetition(self, n, ply=None):
        return self.repetition_count(ply) + 1 >= n

    def outcome(self, ply=None):
        ply = len(self.moves) if ply is None else ply
        return self.rules.outcome(self.pos[ply], self.legal[ply], self.clock[ply], self.repetition_count(ply))

    def value_and_terminated(self, ply=None):
        o = self.outcome(ply)
        return (o[1], True) if o else (0, False)


def from_uci(u):
    f = P.FILES.index(u[0]) + 8 * (int(u[1]) - 1)
    t = P.FILES.index(u[2]) + 8 * (int(u[3]) - 1)
    return (f, t, " pnbrq".index(u[4]) if len(u) > 4 else 0)


def standard_spelling(pos, m):
    """the move as standard chess spells it: a castling is the king's own two-square move; everything else is itself"""
    if P.is_castling(pos, m):
        return (m[0], P.castling_squares(m[0], m[1])[0], 0)
    return m


# ------------------------------------------------------------------------------------------------ the material table's anchor
def signature(board, white):
    """(the side's men without the king, the opponent's men without the king): sorted letters, a bishop as D or L by its square colour"""
    def men(w):
        out = []
        for s in range(64):
            c = board[s]
            if c != "." and c.isupper() == w and c.upper() != "K":
                out.append(("D" if square_is_dark(s) else "L") if c.upper() == "B" else c.upper())
        return "".join(sorted(out))
    return men(white), men(not white)


def fold(sig):
    """bishop colours matter only relative to each other: a signature and its dark/light swap are one"""
    swap = {"D": "L", "L": "D"}
    other = tuple("".join(sorted(swap.get(c, c) for c in part)) for part in sig)
    return min(sig, other)


def pawnless_signatures(max_men=4):
    """every (side's men, opponent's men) of at most max_men men on the board, kings included, without pawns"""
    letters = "DLNQR"
    packs = [""] + [a for a in letters] + [a + b for i, a in enumerate(letters) for b in letters[i:]]
    return sorted({fold((a, b)) for a in packs for b in packs if 2 + len(a) + len(b) <= max_men})


def table_says_sufficient(sig, rules=RULES):
    """the material table's verdict on a signature, asked on a board that holds exactly those men"""
    board = ["."] * 64
    board[4], board[60] = "K", "k"
    dark = [s for s in range(8, 56) if square_is_dark(s)]
    light = [s for s in range(8, 56) if not square_is_dark(s)]
    for part, upper in ((sig[0], True), (sig[1], False)):
        for c in part:
            s = dark.pop() if c == "D" else light.pop() if c == "L" else (dark.pop() if len(dark) > len(light) else light.pop())
            letter = "B" if c in "DL" else c
            board[s] = letter if upper else letter.lower()
    return not rules.insufficient_side(board, True)


# One checkmate per sufficient signature: White has mated, Black is to move.  Found by exhaustive placement with plainrules and
# stored; test_plain_endings.py checks each with plainrules.is_checkmate, checks that its men are its signature's, and that the keys
# are exactly the signatures the table calls sufficient.
MATE_WITNESSES = {
    ("D", "L"): "kb6/8/K7/8/8/8/8/7B b - - 0 1",
    ("D", "N"): "kn6/1B6/1K6/8/8/8/8/8 b - - 0 1",
    ("DL", ""): "k7/8/K7/8/8/8/7B/7B b - - 0 1",
    ("DN", ""): "k7/8/KN6/8/8/8/7B/8 b - - 0 1",
    ("DQ", ""): "k7/Q7/K7/8/8/8/8/B7 b - - 0 1",
    ("DR", ""): "k1R5/8/K7/8/8/8/8/B7 b - - 0 1",
    ("N", "D"): "kb6/8/KN6/8/8/8/8/8 b - - 0 1",
    ("N", "N"): "kn6/2N5/1K6/8/8/8/8/8 b - - 0 1",
    ("N", "R"): "kr6/2N5/K7/8/8/8/8/8 b - - 0 1",
    ("NN", ""): "k7/8/KNN5/8/8/8/8/8 b - - 0 1",
    ("NQ", ""): "k7/Q7/K7/8/8/8/8/N7 b - - 0 1",
    ("NR", ""): "k1R5/8/K7/8/8/8/8/N7 b - - 0 1",
    ("Q", ""): "k7/Q7/K7/8/8/8/8/8 b - - 0 1",
    ("Q", "D"): "kb6/8/K7/8/8/8/8/7Q b - - 0 1",
    ("Q", "N"): "k7/Q7/K7/8/8/8/8/n7 b - - 0 1",
    ("Q", "Q"): "k7/Q7/K7/8/8/8/8/1q6 b - - 0 1",
    ("Q", "R"): "k7/Q7/K7/8/8/8/8/1r6 b - - 0 1",
    ("QQ", ""): "k7/Q7/K7/8/8/8/8/Q7 b - - 0 1",
    ("QR", ""): "k1R5/8/K7/8/8/8/8/Q7 b - - 0 1",
    ("R", ""): "k1R5/8/K7/8/8/8/8/8 b - - 0 1",
    ("R", "D"): "k1R5/8/K7/8/8/8/8/b7 b - - 0 1",
    ("R", "N"): "k1R5/8/K7/8/8/8/8/n7 b - - 0 1",
    ("R", "Q"): "k1R5/8/K7/8/8/8/8/3q4 b - - 0 1",
    ("R", "R"): "kr6/R7/K7/8/8/8/8/8 b - - 0 1",
    ("RR", ""): "k1R5/8/K7/8/8/8/8/R7 b - - 0 1",
}
