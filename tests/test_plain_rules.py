"""Chess960 castling and the 960 start positions held to a generator written from the rule text (tests/plainrules.py).  CPU only.

Until here everything that checked Chess960 castling compared restatements of one reading of python-chess's generate_castling_moves
(sz_king_targets in csrc/sz_chess.h, oracle/oc_chess.c, the fixtures made with the oracle's rules), and one public perft table.  The
plain generator is a second statement, from the FIDE text, structured differently (mailbox, make-and-test; the king's destination is
tested on the board after the move).  Here
  (1) it reproduces the seven public perft tables of perftwalk.PERFT (depth 3 at least; the numbers are perftwalk's), so it is held to
      something public itself;
  (2) its Scharnagl start positions are 960 distinct legal ones, and the host mirror's and the oracle's equal them for every n;
  (3) on every position of tests/castling_lab.py (every (a-rook, king, h-rook) file triple x the variants, both colours) the host
      mirror agrees with it on the legal (from, to, promotion) set of the root, on every child's placement, side to move, en-passant
      square, castling rook squares, castling planes and legal move set (perft(2) move by move), and one ply deeper (perft(3) move by
      move) below every castling and every capture of a rook that carried a right;
  (4) the same for root move sets and perft(2) counts of the 960 start positions;
  (5) a position and its colour flip have the same perft(1), perft(2) on the host mirror and on the oracle, which are the plain
      generator's counts too.
No tolerance, nothing skipped.  Run time of this module: 56 s (sum of pytest --durations on the build machine, 45 s of it the six lab
cases; the slowest CPU module of the parent commit, test_compose_ref.py, took 65 s in the same run).  The public tables are therefore
walked to depth 3-4 only; no lab position was dropped.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from oracle import oracle as O
import perftwalk as W
import plainrules as P
import castling_lab as LAB

# depth walked by the plain generator per public table: 3 everywhere, deeper where it costs a few seconds
TABLE_DEPTH = {"startpos": 4, "kiwipete": 3, "pos3": 4, "pos4": 3, "pos5": 3, "pos6": 3, "c960": 4}
STARTPOS_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
WORD = {w: i for i, w in enumerate(W.RECORD_WORDS)}


def test_lab_tells_a_rule_applied_from_a_rule_ignored():
    legal, refused = LAB.coverage()
    assert len(legal) == 56 * 2 * 2 and min(legal.values()) >= 1
    assert set(refused) == set(LAB.REASONS) and all(refused.values())
    print({r: len(t) for r, t in refused.items()})


@pytest.mark.parametrize("name", [p[0] for p in W.PERFT])
def test_plain_generator_reproduces_the_public_tables(name):
    _, fen, _, want = W.PERFT_BY_NAME[name]
    d = TABLE_DEPTH[name]
    assert 3 <= d <= len(want)
    pos = P.from_fen(fen or STARTPOS_FEN)
    assert [P.perft(pos, k + 1) for k in range(d)] == want[:d]


def test_plain_generator_knows_check_mate_and_stalemate():
    assert P.is_checkmate(P.from_fen("rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3"))
    assert P.is_stalemate(P.from_fen("7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"))
    assert not P.is_stalemate(P.from_fen(W.MATE_IN_ONE)) and len(P.legal_moves(P.from_fen(W.MAX_FANOUT))) == 218
    # the capture that uncovers a rank attack: both pawns leave the fifth rank at once
    assert (33, 42, 0) not in P.legal_moves(P.from_fen("8/8/8/KPp4r/8/8/8/7k w - c6 0 2"))
    assert (33, 42, 0) in P.legal_moves(P.from_fen("8/8/8/KPp5/8/8/8/7k w - c6 0 2"))


# ------------------------------------------------------------------------------------------------ reading the host mirror
def host_position(ct):
    """the host mirror's position as the plain generator spells it: (mailbox, white to move, castling rook squares, ep square)"""
    rec = ct.board.bitboards()
    board = ["."] * 64
    white = rec[WORD["white"]]
    for word, letter in zip(W.RECORD_WORDS[:6], "pnbrqk"):
        bb = rec[WORD[word]]
        while bb:
            s = (bb & -bb).bit_length() - 1
            bb &= bb - 1
            assert board[s] == ".", "two pieces on one square"
            board[s] = letter.upper() if white >> s & 1 else letter
    st = ct.board._st()
    rights = frozenset(s for s in range(64) if rec[WORD["castling"]] >> s & 1)
    return board, bool(st[0]), rights, (st[3] if st[3] >= 0 else None)


def plain_position(pos):
    return pos.board, pos.white, pos.rights, pos.ep


def host_moves(ct):
    """{(from, to, promotion): action index}, the mirror's action indices decoded with the project's codec (ChessTensor.move_from_index
    without the Move objects)"""
    out = {}
    acts = ct.legal_action_indices()
    f, t, p = C.c_int32(), C.c_int32(), C.c_int32()
    decode, g, rf, rt, rp = N.lib().szh_action_to_move, ct._g, C.byref(f), C.byref(t), C.byref(p)
    for a in acts:
        assert decode(g, a, rf, rt, rp) == N.SZ_OK
        out[(f.value, t.value, p.value)] = a
    assert len(out) == len(acts), "two action indices decode to one move"
    return out


def show(x):
    return P.Position(x, True, None, None).placement() if isinstance(x, list) else sorted(x) if isinstance(x, frozenset) else x


def names(moves):
    return sorted(P.move_name(m) for m in moves)


def assert_same_moves(tag, ct, pos):
    hm, pm = host_moves(ct), P.legal_moves(pos)
    assert len(set(pm)) == len(pm)
    if set(hm) != set(pm):
        raise AssertionError("%s: legal moves differ: only the host mirror has %s, only the plain generator has %s"
                             % (tag, names(set(hm) - set(pm)), names(set(pm) - set(hm))))
    return hm, pm


def assert_same_position(tag, ct, pos, planes=True):
    got, want = host_position(ct), plain_position(pos)
    for what, g, w in zip(("piece placement", "side to move", "castling rook squares", "en-passant square"), got, want):
        assert g == w, "%s: %s: host mirror %s, plain generator %s" % (tag, what, show(g), show(w))
    if planes:
        wk, wq, bk, bq = pos.castling_flags()
        want_planes = (wk, wq, bk, bq) if pos.white else (bk, bq, wk, wq)           # own g-side, own c-side, theirs
        rep = ct.get_representation().numpy().reshape(119, 64)[114:118]
        assert (rep == np.array(want_planes, bool)[:, None]).all(), "%s: castling planes %s, plain generator %s" % (
            tag, rep.any(1).tolist(), list(want_planes))


def loses_a_right_by_force(pos, m):
    """a castling, or the capture of a rook that carried a right"""
    return P.is_castling(pos, m) or (m[1] in pos.rights and pos.board[m[1]] in "Rr")


def walk_lab_position(name, fen):
    """(3) of the module docstring for one position; returns (perft(1), perft(2), children walked one ply deeper)"""
    ct, pos = sz.ChessTensor(chess960=True, fen=fen), P.from_fen(fen)
    assert_same_position(name, ct, pos, planes=False)                      # a root sits at ply 0, where the castling planes are all ones
    hm, pm = assert_same_moves(name, ct, pos)
    # the device test takes these children as further roots, read off the host mirror's record: the same children
    assert {a for a, _ in W.children_that_take_a_right(ct)} == {hm[m] for m in pm if loses_a_right_by_force(pos, m)}, name
    n2 = deeper = 0
    for m in pm:
        tag = "%s %s" % (name, P.move_name(m))
        c, cpos = ct.copy(), P.make(pos, m)
        c.push_action(hm[m])
        assert_same_position(tag, c, cpos)
        chm, cpm = assert_same_moves(tag, c, cpos)
        n2 += len(cpm)
        if loses_a_right_by_force(pos, m):
            deeper += 1
            for m2 in cpm:
                g, gpos = c.copy(), P.make(cpos, m2)
                g.push_action(chm[m2])
                assert_same_position("%s %s" % (tag, P.move_name(m2)), g, gpos)
                assert_same_moves("%s %s" % (tag, P.move_name(m2)), g, gpos)
    return len(pm), n2, deeper


@functools.lru_cache(maxsize=None)
def lab_counts(king_file):
    return {name: walk_lab_position(name, fen) for name, fen in LAB.LAB_BY_KING_FILE[king_file]}


# ------------------------------------------------------------------------------------------------ (2) start positions
def test_scharnagl_numbers_give_960_distinct_legal_back_ranks():
    ranks = [P.scharnagl_back_rank(n) for n in range(960)]
    assert len(set(ranks)) == 960
    for r in ranks:
        assert sorted(r) == sorted("RNBQKBNR")
        b1, b2 = [i for i in range(8) if r[i] == "B"]
        assert (b1 + b2) % 2 == 1                                       # opposite colours
        assert r.index("R") < r.index("K") < r.rindex("R")
    assert (ranks[0], ranks[518], ranks[959]) == ("BBQNNRKR", "RNBQKBNR", "RKRNNQBB")


def test_host_mirror_and_oracle_start_positions_equal_the_plain_ones():
    for n in range(960):
        pos = P.scharnagl_start(n)
        assert len(pos.rights) == 4
        ct = sz.ChessTensor(chess960=True, scharnagl=n)
        assert host_position(ct) == plain_position(pos), "Scharnagl %d: host mirror" % n
        ob = O.Board.from_chess960_pos(n)
        assert ob.board_fen() == pos.placement() and ob.turn == 1 and ob.ep_square in (-1, None), "Scharnagl %d: oracle" % n
        assert ob.castling_rights == sum(1 << s for s in pos.rights), "Scharnagl %d: oracle castling rook squares" % n
        rec = ct.board.bitboards()
        assert rec[:7] == ob.bitboards()[:7] and rec[WORD["castling"]] == ob.castling_rights, "Scharnagl %d: host mirror and oracle" % n


def test_start_positions_root_moves_and_perft2():
    total = [0, 0]
    for n, fen in LAB.STARTS:
        ct, pos = sz.ChessTensor(chess960=True, scharnagl=n), P.from_fen(fen)
        _, pm = assert_same_moves("Scharnagl %d" % n, ct, pos)
        p2 = P.perft(pos, 2)
        assert (ct.perft(1), ct.perft(2)) == (len(pm), p2), "Scharnagl %d" % n
        assert O.Board.from_chess960_pos(n).perft(2) == p2, "Scharnagl %d: oracle" % n
        total[0] += len(pm)
        total[1] += p2
    print("960 starts: perft(1) total %d, perft(2) total %d" % tuple(total))


# ------------------------------------------------------------------------------------------------ (3) the lab
@pytest.mark.parametrize("king_file", range(1, 7), ids=["king_%s" % P.FILES[k] for k in range(1, 7)])
def test_lab_positions_move_by_move(king_file):
    counts = lab_counts(king_file)
    assert len(counts) == len(LAB.LAB_BY_KING_FILE[king_file])
    castled = sum(d for _, _, d in counts.values())
    print("king on the %s-file: %d positions, %d root moves, %d child moves, %d children walked one ply deeper"
          % (P.FILES[king_file], len(counts), sum(c[0] for c in counts.values()), sum(c[1] for c in counts.values()), castled))
    # alone_a and alone_h of each of the k * (7 - k) triples hold a legal castling for either colour, open_a and open_h a capture
    assert castled >= 8 * king_file * (7 - king_file)
    flipped = {n: c for n, c in counts.items() if n.startswith("~")}
    assert len(flipped) * 2 == len(counts) and all(counts[n[1:]] == c for n, c in flipped.items())


def test_a_capture_of_a_rook_with_a_right_is_among_the_children_walked_deeper():
    pos = P.from_fen(dict(LAB.LAB)["beg:open_h"])
    m = (6, 62, 0)
    assert m in P.legal_moves(pos) and loses_a_right_by_force(pos, m) and not P.is_castling(pos, m)
    assert P.make(pos, m).rights == frozenset({1, 57})


# ------------------------------------------------------------------------------------------------ (5) colour flip
@pytest.mark.parametrize("king_file", range(1, 7), ids=["king_%s" % P.FILES[k] for k in range(1, 7)])
def test_colour_flip_keeps_perft_on_host_mirror_and_oracle(king_file):
    counts = lab_counts(king_file)
    fens = dict(LAB.LAB_BY_KING_FILE[king_file])
    for name, fen in fens.items():
        if name.startswith("~"):
            continue
        got = []
        for f in (fen, fens["~" + name]):
            ct = sz.ChessTensor(chess960=True, fen=f)
            got.append((ct.perft(1), ct.perft(2)))
            ob = O.Board.from_fen(f, chess960=True)
            got.append((ob.perft(1), ob.perft(2)))
        assert got[0] == got[1] == got[2] == got[3] == counts[name][:2], "%s: (perft(1), perft(2)) host, oracle, host flipped, oracle flipped: %s; plain %s" % (
            name, got, counts[name][:2])
