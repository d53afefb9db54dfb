"""Positions built to meet every Chess960 castling geometry: (name, FEN) pairs made in code, no hand-written expectations.  What is
legal in them is decided by the plain generator (tests/plainrules.py); the host mirror is held to it in tests/test_plain_rules.py and
the device to the host mirror in tests/test_gpu_chess960_castling.py.

For each of the 56 triples a-rook file < king file < h-rook file, white's king and rooks stand on those files of rank 1, black's on the
same files of rank 8, with the same rights (Shredder letters); all 16 pawns stand on ranks 2 and 7 unless a variant removes one, so that
nothing reaches a back rank by accident; white is to move.  A name reads "<a><k><h>:<variant>", e.g. "bcf:shield_a".  Variants:

  base            both castlings available
  blocked(s)      one white knight on s, for each back-rank square s that is empty in base
  file(f)         white's f-pawn removed and an extra black rook on f4, attacking f1 along the file, for f in a..h: the king in check
                  (f = king's file), a crossing square or the destination attacked, or only a rook or a square the king does not cross
                  attacked (castling stays legal)
  shield_a/_h     where a1 (h1) lies outside the castling rook: a black rook on a1 (h1); the castling rook is all that stands between it
                  and the king's path.  King c1, rook b1, black rook a1 must not castle.
  rights(...)     only the a-side right, only the h-side right, none
  inner_right_a/_h  where the a-rook (h-rook) is not on the a-file (h-file): an extra rook on a1 and a8 (h1 and h8) WITHOUT a right, the
                  inner rook keeps its right; only Shredder letters can say this
  open_a/_h       both pawns of the a-rook's (h-rook's) file removed: the two rooks that carry a right face each other, so the root has a
                  move that captures a rook with a right (with a rook that loses its own)
  alone_a/_h      the other rook stands on the third (sixth) rank of its file, without a right: where the three stand side by side (a1 b1 c1) the other rook blocks this
                  castling in every variant above, and a rule that is never met is not tested

Every position appears a second time colour-flipped ("~" in front of the name): ranks mirrored, colours swapped, black to move.
STARTS is the second list: the 960 start positions by Scharnagl number.

coverage() checks, on the plain generator alone, that the lab can tell a rule that is applied from one that is not: castling on either
side is legal in some variant of every triple for either colour, and is refused for every named reason in some triple.
"""
import itertools

import plainrules as P

FILES = P.FILES
TRIPLES = list(itertools.combinations(range(8), 3))                     # (a-rook file, king file, h-rook file), 56 of them


def _base(a, k, h):
    grid = {}
    for f in range(8):
        grid[8 + f], grid[48 + f] = "P", "p"
    for f, c in ((a, "R"), (k, "K"), (h, "R")):
        grid[f], grid[56 + f] = c, c.lower()
    return grid


def _fen(grid, files, white_to_move=True):
    """files: the files whose rooks carry a right, the same for both colours"""
    pos = P.Position([grid.get(s, ".") for s in range(64)], white_to_move, frozenset(), None)
    letters = "".join(FILES[f] for f in sorted(files, reverse=True))
    return "%s %s %s - 0 1" % (pos.placement(), "w" if white_to_move else "b", (letters.upper() + letters) or "-")


def flip(fen):
    """ranks mirrored, colours swapped, the other side to move"""
    placement, turn, rights, ep, half, full = fen.split()
    assert ep == "-"
    rights = "".join(sorted(rights.swapcase(), key=lambda c: (c.islower(), -ord(c)))) if rights != "-" else "-"
    return "%s %s %s - %s %s" % ("/".join(reversed(placement.swapcase().split("/"))), "b" if turn == "w" else "w", rights, half, full)


def _variants(a, k, h):
    both = (a, h)
    yield "base", _fen(_base(a, k, h), both)
    for s in range(8):
        if s not in (a, k, h):
            g = _base(a, k, h)
            g[s] = "N"
            yield "blocked(%s1)" % FILES[s], _fen(g, both)
    for f in range(8):
        g = _base(a, k, h)
        del g[8 + f]
        g[24 + f] = "r"
        yield "file(%s)" % FILES[f], _fen(g, both)
    if a != 0:
        g = _base(a, k, h)
        g[0] = "r"
        yield "shield_a", _fen(g, both)
    if h != 7:
        g = _base(a, k, h)
        g[7] = "r"
        yield "shield_h", _fen(g, both)
    yield "rights(a-side only)", _fen(_base(a, k, h), (a,))
    yield "rights(h-side only)", _fen(_base(a, k, h), (h,))
    yield "rights(none)", _fen(_base(a, k, h), ())
    if a != 0:
        g = _base(a, k, h)
        g[0], g[56] = "R", "r"
        yield "inner_right_a", _fen(g, both)
    if h != 7:
        g = _base(a, k, h)
        g[7], g[63] = "R", "r"
        yield "inner_right_h", _fen(g, both)
    for side, f, other in (("a", a, h), ("h", h, a)):
        g = _base(a, k, h)
        del g[8 + f], g[48 + f]
        yield "open_%s" % side, _fen(g, both)
        g = _base(a, k, h)
        g[16 + other], g[40 + other] = g.pop(other), g.pop(56 + other)
        yield "alone_%s" % side, _fen(g, (f,))


def triple_name(t):
    return "".join(FILES[f] for f in t)


def _build():
    lab = []
    for t in TRIPLES:
        for variant, fen in _variants(*t):
            name = "%s:%s" % (triple_name(t), variant)
            lab.append((name, fen))
            lab.append(("~" + name, flip(fen)))
    assert len({n for n, _ in lab}) == len(lab) == len({f for _, f in lab})
    return lab


LAB = _build()
LAB_BY_KING_FILE = {k: [(n, f) for n, f in LAB if FILES.index(n.lstrip("~")[1]) == k] for k in range(1, 7)}
STARTS = [(n, P.scharnagl_fen(n)) for n in range(960)]

REASONS = (P.BLOCKED, P.IN_CHECK, P.CROSSING, P.DESTINATION, P.UNCOVERED)


def coverage():
    """On the plain generator alone: {(triple, colour, side): number of lab positions in which that castling is legal} and
    {reason: set of triples in which a castling is refused for it}.  Asserts that every entry of the first is positive for all 56
    triples, both colours and both sides, that every reason occurs, and that the known case (king c1, rook b1, black rook a1) is among
    those refused because the destination is attacked only after the rook left."""
    legal = {(t, colour, side): 0 for t in TRIPLES for colour in "wb" for side in "ah"}
    refused = {r: set() for r in REASONS}
    for name, fen in LAB:
        pos = P.from_fen(fen)
        t = tuple(FILES.index(c) for c in name.lstrip("~")[:3])
        ksq = pos.king_square(pos.white)
        for rsq in P.castling_rooks(pos):
            why = P.why_not_castle(pos, rsq)
            if why is None:
                legal[(t, "w" if pos.white else "b", "a" if rsq < ksq else "h")] += 1
            else:
                refused[why].add(t)
    missing = [k for k, n in legal.items() if n == 0]
    assert not missing, "castling is never legal for %s" % (missing[:5],)
    for r in REASONS:
        assert refused[r], "no lab position refuses castling because: %s" % r
    assert (1, 2, 7) in refused[P.UNCOVERED] and (1, 3, 7) in refused[P.UNCOVERED]
    return legal, refused
