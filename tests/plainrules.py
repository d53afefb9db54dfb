"""A plain chess move generator written from the rule text: the second, independent statement of the rules that the Chess960 castling
tests hold the host mirror (csrc/sz_chess.h) and, through it, the device to (tests/test_plain_rules.py, tests/castling_lab.py).

It imports nothing of the project, uses no bitboards and shares no table with it.  A position is a 64-entry mailbox (a1 = 0, h1 = 7,
a8 = 56; "." or a FEN piece letter), the side to move, the set of rook squares that still carry a castling right (the Shredder-FEN
spelling) and the en-passant square.  Move generation is the textbook one: every pseudo-legal move is made on a copy and rejected if
the mover's king is then attacked; attacks are found by looking outward from the square along rays, knight jumps and pawn captures.
Repetition, the 75-move rule and insufficient material are not here: tests/plainendings.py states them on top of this module
(tests/rule_endings.py holds ten constructed games with the oracle's expectations).

Castling is stated as the FIDE Laws of Chess state it (FIDE Handbook E.01, edition in force from 1 January 2023):

  Article 3.8.2    "... 'castling'.  This is a move of the king and either rook of the same colour along the player's first rank,
                   counting as a single move of the king ..."
  3.8.2.1          "The right to castle has been lost: 3.8.2.1.1 if the king has already moved, or 3.8.2.1.2 with a rook that has
                   already moved."
  3.8.2.2          "Castling is prevented temporarily: 3.8.2.2.1 if the square on which the king stands, or the square which it must
                   cross, or the square which it is to occupy, is attacked by one or more of the opponent's pieces, or 3.8.2.2.2 if
                   there is any piece between the king and the rook with which castling is to be effected."
  Guidelines II (Chess960 Rules), II.3.2.5
                   "... after c-side castling (notated as 0-0-0 ...), the king is on the c-square (c1 for white and c8 for black) and
                   the rook is on the d-square (d1 for white and d8 for black).  After g-side castling (notated as 0-0 ...), the king is
                   on the g-square (g1 for white and g8 for black) and the rook is on the f-square (f1 for white and f8 for black)."
  II.3.2.6.2       "In some starting positions, the king or rook (but not both) does not move during castling."
  II.3.2.6.4       "All the squares between the king's initial and final squares (including the final square) and all the squares
                   between the rook's initial and final squares (including the final square) must be vacant except for the king and
                   castling rook."
  II.3.2.6.5       "In some starting positions, some squares can stay filled during castling that would have to be vacant in standard
                   chess.  For example, after c-side castling 0-0-0, it is possible to have a, b, and/or e still filled, and after
                   g-side castling (0-0), it is possible to have e and/or h filled."

How the clauses are read here (why_not_castle):
  * the right: a rook square in `rights`; it goes when the king moves, when something leaves that square or when something is
    captured on it (3.8.2.1; a captured rook cannot castle);
  * vacancy: II.3.2.6.4 word for word, on the board as it stands;
  * "the square on which the king stands": the king is not in check;
  * "the square which it must cross": every square strictly between the king's start and its destination, looked at on the board as
    it stands with the king lifted off it (a king that shields a square from the piece that checks it is refused by the clause above
    already, so lifting it changes no answer);
  * "the square which it is to occupy": decided by MAKING the move (king on c/g, rook on d/f, both start squares cleared first) and
    asking whether the king is attacked on the resulting board, exactly as for any other move.  No occupancy formula: a castling rook
    that shielded the king's destination (king c1, rook b1, enemy rook a1) has left when the question is asked.

Moves are (from, to, promotion) with promotion 0 or 2..5 for knight, bishop, rook, queen; a castling is spelled king's square -> the
castling rook's square.  The en-passant square is recorded after every double push (whether or not a capture is possible).
"""

FILES = "abcdefgh"
KNIGHT, BISHOP, ROOK, QUEEN = 2, 3, 4, 5
PROMO_LETTER = {KNIGHT: "n", BISHOP: "b", ROOK: "r", QUEEN: "q"}

_ORTHO = ((1, 0), (-1, 0), (0, 1), (0, -1))
_DIAG = ((1, 1), (1, -1), (-1, 1), (-1, -1))
_JUMPS = ((1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1), (-2, 1), (-1, 2))


def _walk(sq, df, dr):
    """the squares met when walking from sq in direction (df, dr) to the edge of the board"""
    out, f, r = [], (sq & 7) + df, (sq >> 3) + dr
    while 0 <= f < 8 and 0 <= r < 8:
        out.append(r * 8 + f)
        f, r = f + df, r + dr
    return tuple(out)


# geometry of the empty board, from coordinates alone
ORTHO_RAYS = tuple(tuple(_walk(s, df, dr) for df, dr in _ORTHO) for s in range(64))
DIAG_RAYS = tuple(tuple(_walk(s, df, dr) for df, dr in _DIAG) for s in range(64))
JUMPS = tuple(tuple(_walk(s, df, dr)[0] for df, dr in _JUMPS if _walk(s, df, dr)) for s in range(64))
STEPS = tuple(tuple(ray[0] for ray in ORTHO_RAYS[s] + DIAG_RAYS[s] if ray) for s in range(64))


def square_name(sq):
    return FILES[sq & 7] + str((sq >> 3) + 1)


def move_name(m):
    return square_name(m[0]) + square_name(m[1]) + PROMO_LETTER.get(m[2], "")


class Position:
    __slots__ = ("board", "white", "rights", "ep")

    def __init__(self, board, white, rights, ep):
        self.board, self.white, self.rights, self.ep = board, white, rights, ep

    def placement(self):
        """the piece-placement field of a FEN"""
        rows = []
        for r in range(7, -1, -1):
            row, gap = "", 0
            for f in range(8):
                c = self.board[r * 8 + f]
                if c == ".":
                    gap += 1
                else:
                    row, gap = row + (str(gap) if gap else "") + c, 0
            rows.append(row + (str(gap) if gap else ""))
        return "/".join(rows)

    def king_square(self, white):
        return self.board.index("K" if white else "k")

    def castling_flags(self):
        """(white g-side, white c-side, black g-side, black c-side): does that side hold a right with a rook on that side of its king"""
        out = []
        for white in (True, False):
            base = 0 if white else 56
            k = self.king_square(white)
            mine = [s for s in self.rights if base <= s < base + 8] if base <= k < base + 8 else []
            out += [any(s > k for s in mine), any(s < k for s in mine)]
        return tuple(out)


def from_fen(fen):
    """FEN with KQkq (the outermost rook on that side of the king) or Shredder file letters in the castling field"""
    parts = fen.split()
    board = ["."] * 64
    r, f = 7, 0
    for c in parts[0]:
        if c == "/":
            r, f = r - 1, 0
        elif c.isdigit():
            f += int(c)
        else:
            board[r * 8 + f] = c
            f += 1
    rights = set()
    for c in parts[2] if len(parts) > 2 else "-":
        if c == "-":
            continue
        white = c.isupper()
        base, rook, king = (0, "R", "K") if white else (56, "r", "k")
        rank = board[base:base + 8]
        if king not in rank:
            continue
        k = rank.index(king)
        rooks = [i for i in range(8) if rank[i] == rook]
        if c in "Kk":
            side = [i for i in rooks if i > k]
            file = max(side) if side else None
        elif c in "Qq":
            side = [i for i in rooks if i < k]
            file = min(side) if side else None
        else:
            file = FILES.index(c.lower())
            file = file if file in rooks else None
        if file is not None:
            rights.add(base + file)
    ep = None
    if len(parts) > 3 and parts[3] != "-":
        ep = FILES.index(parts[3][0]) + 8 * (int(parts[3][1]) - 1)
    return Position(board, parts[1] != "b" if len(parts) > 1 else True, frozenset(rights), ep)


# ------------------------------------------------------------------------------------------------ attacks
def attacked(board, sq, by_white):
    """is `sq` attacked by a piece of that colour?  Looks outward from the square."""
    pawn, knight, bishop, rook, queen, king = "PNBRQK" if by_white else "pnbrqk"
    for s in JUMPS[sq]:
        if board[s] == knight:
            return True
    for ray in ORTHO_RAYS[sq]:
        for n, s in enumerate(ray):
            c = board[s]
            if c != ".":
                if c == rook or c == queen or (n == 0 and c == king):
                    return True
                break
    for ray in DIAG_RAYS[sq]:
        for n, s in enumerate(ray):
            c = board[s]
            if c != ".":
                if c == bishop or c == queen or (n == 0 and c == king):
                    return True
                break
    # a white pawn captures one rank up, so it attacks sq from the rank below; a black one from the rank above
    f, r = sq & 7, (sq >> 3) + (-1 if by_white else 1)
    if 0 <= r < 8:
        if f > 0 and board[r * 8 + f - 1] == pawn:
            return True
        if f < 7 and board[r * 8 + f + 1] == pawn:
            return True
    return False


def in_check(pos, white=None):
    white = pos.white if white is None else white
    return attacked(pos.board, pos.king_square(white), not white)


# ------------------------------------------------------------------------------------------------ making a move
def is_castling(pos, m):
    return pos.board[m[0]] == ("K" if pos.white else "k") and pos.board[m[1]] == ("R" if pos.white else "r")


def castling_squares(ksq, rsq):
    """(king's destination, rook's destination): c and d on the a-side, g and f on the h-side, on the king's rank"""
    base = ksq & ~7
    return (base + 2, base + 3) if rsq < ksq else (base + 6, base + 5)


def board_after(pos, m):
    """the mailbox after m, whose legality is not looked at"""
    frm, to, promo = m
    board = pos.board[:]
    piece = board[frm]
    if is_castling(pos, m):
        kto, rto = castling_squares(frm, to)
        board[frm] = board[to] = "."                                    # both start squares cleared first: either may be a destination
        board[kto], board[rto] = piece, pos.board[to]
        return board
    board[frm] = "."
    if piece in "Pp" and to == pos.ep and (to - frm) % 8 != 0:
        board[to - 8 if pos.white else to + 8] = "."                    # en passant: the pawn that made the double push
    if promo:
        piece = PROMO_LETTER[promo].upper() if pos.white else PROMO_LETTER[promo]
    board[to] = piece
    return board


def make(pos, m):
    """the position after m: the mailbox, the other side to move, the rights that are left, the en-passant square"""
    frm, to, _ = m
    white, piece, rights = pos.white, pos.board[frm], pos.rights
    ep = (frm + to) // 2 if piece in "Pp" and abs(to - frm) == 16 else None
    king_moved = piece in "Kk"
    if rights and (king_moved or frm in rights or to in rights):
        gone = {frm, to}                                                # that rook moved, or something was captured on its square
        if king_moved:
            base = 0 if white else 56
            gone |= set(range(base, base + 8))                          # the king moved (castling included)
        rights = frozenset(s for s in rights if s not in gone)
    return Position(board_after(pos, m), not white, rights, ep)


# ------------------------------------------------------------------------------------------------ castling
BLOCKED, IN_CHECK, CROSSING, DESTINATION, UNCOVERED = "blocked", "in check", "crossing attacked", "destination attacked", \
    "destination attacked only after the rook left"


def why_not_castle(pos, rsq):
    """None if the side to move may castle with the rook on rsq (a square of pos.rights on its back rank), else the first reason
    that forbids it, in the order of the module docstring"""
    white, board = pos.white, pos.board
    ksq = pos.king_square(white)
    kto, rto = castling_squares(ksq, rsq)
    must_be_vacant = set(range(min(ksq, kto), max(ksq, kto) + 1)) | set(range(min(rsq, rto), max(rsq, rto) + 1))
    between = set(range(min(ksq, rsq) + 1, max(ksq, rsq)))              # 3.8.2.2.2; inside must_be_vacant in every geometry but stated
    if any(board[s] != "." for s in (must_be_vacant | between) - {ksq, rsq}):
        return BLOCKED
    if attacked(board, ksq, not white):
        return IN_CHECK
    lifted = board[:]
    lifted[ksq] = "."
    step = 1 if kto > ksq else -1
    for s in range(ksq + step, kto, step):
        if attacked(lifted, s, not white):
            return CROSSING
    after = board_after(pos, (ksq, rsq, 0))
    if attacked(after, after.index(board[ksq]), not white):             # the king, wherever the move put it
        return DESTINATION if attacked(lifted, kto, not white) else UNCOVERED       # the rook's leaving rsq is all that differs
    return None


def castling_rooks(pos):
    """rook squares with which the side to move still holds a right (king on its back rank)"""
    base = 0 if pos.white else 56
    king = "K" if pos.white else "k"
    if king not in pos.board[base:base + 8]:
        return []
    return sorted(s for s in pos.rights if base <= s < base + 8 and pos.board[s] == ("R" if pos.white else "r"))


# ------------------------------------------------------------------------------------------------ move generation
def pseudo_legal(pos):
    board, white = pos.board, pos.white
    mine = "PNBRQK" if white else "pnbrqk"
    moves = []
    for frm in range(64):
        piece = board[frm]
        if piece == "." or piece not in mine:
            continue
        kind = piece.upper()
        if kind == "P":
            up = 8 if white else -8
            rank = frm >> 3
            last = rank == (6 if white else 1)
            targets = []
            if board[frm + up] == ".":
                targets.append(frm + up)
                if rank == (1 if white else 6) and board[frm + 2 * up] == ".":
                    targets.append(frm + 2 * up)
            for df in (-1, 1):
                f = (frm & 7) + df
                if 0 <= f < 8:
                    to = frm + up + df
                    c = board[to]
                    if (c != "." and c not in mine) or (c == "." and to == pos.ep):
                        targets.append(to)
            for to in targets:
                if last:
                    moves += [(frm, to, p) for p in (QUEEN, ROOK, BISHOP, KNIGHT)]
                else:
                    moves.append((frm, to, 0))
        elif kind == "N" or kind == "K":
            for to in (JUMPS if kind == "N" else STEPS)[frm]:
                if board[to] == "." or board[to] not in mine:
                    moves.append((frm, to, 0))
        else:
            rays = (ORTHO_RAYS[frm] if kind != "B" else ()) + (DIAG_RAYS[frm] if kind != "R" else ())
            for ray in rays:
                for to in ray:
                    c = board[to]
                    if c == ".":
                        moves.append((frm, to, 0))
                        continue
                    if c not in mine:
                        moves.append((frm, to, 0))
                    break
    return moves


def legal_moves(pos):
    white = pos.white
    out = []
    king = "K" if white else "k"
    for m in pseudo_legal(pos):
        after = board_after(pos, m)
        if not attacked(after, after.index(king), not white):
            out.append(m)
    ksq = pos.king_square(white)
    for rsq in castling_rooks(pos):
        if why_not_castle(pos, rsq) is None:
            out.append((ksq, rsq, 0))
    return out


def perft(pos, depth):
    moves = legal_moves(pos)
    if depth <= 1:
        return len(moves) if depth == 1 else 1
    return sum(perft(make(pos, m), depth - 1) for m in moves)


def is_checkmate(pos):
    return in_check(pos) and not legal_moves(pos)


def is_stalemate(pos):
    return not in_check(pos) and not legal_moves(pos)


# ------------------------------------------------------------------------------------------------ start positions
_KNIGHT_PAIRS = ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4), (2, 3), (2, 4), (3, 4))


def scharnagl_back_rank(n):
    """the white back rank of Chess960 start position n (Scharnagl's numbering), a-file first, as eight letters"""
    assert 0 <= n < 960
    rank = [None] * 8
    n, light = divmod(n, 4)
    rank[2 * light + 1] = "B"                                           # b, d, f, h
    n, dark = divmod(n, 4)
    rank[2 * dark] = "B"                                                # a, c, e, g
    n, q = divmod(n, 6)
    free = [i for i in range(8) if rank[i] is None]
    rank[free[q]] = "Q"
    free = [i for i in range(8) if rank[i] is None]
    for k in _KNIGHT_PAIRS[n]:
        rank[free[k]] = "N"
    free = [i for i in range(8) if rank[i] is None]
    for i, c in zip(free, "RKR"):
        rank[i] = c
    return "".join(rank)


def scharnagl_fen(n):
    rank = scharnagl_back_rank(n)
    letters = "".join(FILES[i] for i in range(8) if rank[i] == "R")
    return "%s/pppppppp/8/8/8/8/PPPPPPPP/%s w %s%s - 0 1" % (rank.lower(), rank, letters[::-1].upper(), letters[::-1])


def scharnagl_start(n):
    return from_fen(scharnagl_fen(n))
