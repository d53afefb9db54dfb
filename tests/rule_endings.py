"""Constructed games whose NEXT move ends the game or changes a counter class: the rule endings the perft tables do not contain.
Each case is (name, FEN or None, uci moves, the move to look at, claim); the claim is checked on the oracle (oracle/oc_chess.c), so
the expectations are the oracle's and not hand-written numbers.  The second, independent statement of these rules is
tests/plainendings.py; tests/ending_lines.py places the same endings (and _long_game, _rook_snake below) at chosen depths inside the tree
with the plain statement's expectations.  Used on the CPU (host mirror against the oracle on every child and
grandchild, tests/test_perft_walk_driver.py) and on the device (tests/test_gpu_device_perft.py)."""
import numpy as np

import sigma_zero_amd as sz
from oracle import oracle as O

_CYCLE_W = ["g1f3", "g8f6", "f3g1", "f6g8"]


def _rook_snake():
    """K+R v K, kings on h1 / h8: the rook walks a1..a7, b7..b1, c1..c7, d7..d1, e1..e7, f7..f1 and returns to a1 (42 white moves) while the
    black king steps h8-g8-h8...: 84 reversible plies without a repeated position, and the 84th recreates the start position."""
    sq = []
    for f, name in enumerate("abcdef"):
        ranks = range(1, 8) if f % 2 == 0 else range(7, 0, -1)
        sq += ["%s%d" % (name, r) for r in ranks]
    sq.append("a1")
    moves = []
    for k in range(len(sq) - 1):
        moves.append(sq[k] + sq[k + 1])
        moves.append("h8g8" if k % 2 == 0 else "g8h8")
    return moves


def _long_game():
    """260 plies from the start position: 20 blocks of one pawn push (clock reset) and three knight cycles of 4 plies.  A block's base
    position occurs 4 times (never 5); the last block's occurrences are at plies 248, 252, 256 and 260: on both sides of the ring's wrap."""
    white = ["a2a3", "b2b3", "d2d3", "e2e3", "g2g3", "h2h3", "a3a4", "b3b4", "d3d4", "h3h4"]
    black = ["a7a6", "b7b6", "d7d6", "e7e6", "g7g6", "h7h6", "a6a5", "b6b5", "d6d5", "h6h5"]
    moves, w, b = [], 0, 0
    for block in range(20):
        if len(moves) % 2 == 0:                      # white to move
            moves.append(white[w]); w += 1
            cyc = ["g8f6", "g1f3", "f6g8", "f3g1"]
        else:
            moves.append(black[b]); b += 1
            cyc = ["g1f3", "g8f6", "f3g1", "f6g8"]
        moves += cyc * 3
    return moves


# claim: an oracle predicate (see _claim) that holds on the oracle game AFTER `look` was played
CASES = [
    ("fivefold_next_move", None, (_CYCLE_W * 4)[:-1], "f6g8", "fivefold"),
    ("threefold_next_move", None, (_CYCLE_W * 2)[:-1], "f6g8", "threefold_not_over"),
    ("threefold_two_plies_away", None, (_CYCLE_W * 2)[:-2], "f3g1", "not_over"),
    ("clock_149", "8/8/5k2/8/8/3KR3/8/8 w - - 149 100", [], "e3e4", "seventyfive"),
    ("clock_148", "8/8/5k2/8/8/3KR3/8/8 w - - 148 100", [], "e3e4", "clock_149_not_over"),
    ("window_84_plies", "7k/8/8/8/8/8/8/R6K w - - 0 1", _rook_snake()[:-1], "g8h8", "twofold_clock_84"),
    ("ring_wrap_260_plies", None, _long_game()[:-1], "f6g8", "fourth_occurrence_ply_260"),
    ("kb_v_k_by_capture", "k7/8/8/8/8/8/1n6/K1B5 w - - 0 1", [], "a1b2", "insufficient"),
    ("kn_v_k_by_capture", "k7/8/8/8/8/8/1r6/K1N5 w - - 0 1", [], "a1b2", "insufficient"),
    ("same_coloured_bishops_by_capture", "kb6/8/8/8/8/8/1n6/K1B5 w - - 0 1", [], "c1b2", "insufficient"),
]


def _claim(name, ob, oct_):
    v, t = oct_.get_value_and_terminated()
    if name == "fivefold":
        return t and v == 0 and ob.is_repetition(5)
    if name == "threefold_not_over":
        return (not t) and ob.is_repetition(3) and not ob.is_repetition(4)
    if name == "not_over":
        return not t
    if name == "seventyfive":
        return t and v == 0 and ob.halfmove_clock == 150 and not ob.is_insufficient_material()
    if name == "clock_149_not_over":
        return (not t) and ob.halfmove_clock == 149
    if name == "twofold_clock_84":
        return (not t) and ob.halfmove_clock == 84 and ob.is_repetition(2) and not ob.is_repetition(3)
    if name == "fourth_occurrence_ply_260":
        return (not t) and ob.ply == 260 and ob.is_repetition(4) and not ob.is_repetition(5)
    if name == "insufficient":
        return t and v == 0 and ob.is_insufficient_material()
    raise KeyError(name)


def build(case):
    """(host mirror game, oracle game) after the case's moves; asserts the case's claim on the oracle"""
    name, fen, moves, look, claim = case
    ct = sz.ChessTensor(fen=fen) if fen else sz.ChessTensor()
    oct_ = O.ChessTensor.from_fen(fen) if fen else O.ChessTensor()
    for u in moves:
        ct.move_piece(sz.Move.from_uci(u))
        oct_.move_piece(O.Move.from_uci(u))
    assert not oct_.get_value_and_terminated()[1], "%s: the game is over before the move under test" % name
    nxt = oct_.copy()
    nxt.move_piece(O.Move.from_uci(look))
    assert _claim(claim, nxt.board, nxt), "%s: the constructed game does not do what its name says (%s)" % (name, claim)
    return ct, oct_


def assert_host_equals_oracle(tag, ct, oct_):
    """legal moves, planes and terminal value of one position, host mirror against oracle"""
    idx, moves = oct_.legal_action_indices()
    assert ct.legal_action_indices() == idx, "%s: legal moves" % tag
    assert np.array_equal(ct.get_representation().numpy().astype(np.uint8), oct_.get_representation()), "%s: planes" % tag
    assert ct.get_value_and_terminated() == oct_.get_value_and_terminated(), "%s: terminal value" % tag
    return idx, moves


def two_levels(tag, ct, oct_):
    """the game, its children and its grandchildren, host mirror against oracle; returns the game and its non-terminal children as
    roots for the device walk ((path, ChessTensor) pairs), so that an ending two plies away is reached by a device-created child too"""
    roots = [((), ct)]
    idx, moves = assert_host_equals_oracle(tag, ct, oct_)
    for a, m in zip(idx, moves):
        c, oc = ct.copy(), oct_.copy()
        c.push_action(a)
        oc.move_piece(m)
        idx2, moves2 = assert_host_equals_oracle("%s child %d" % (tag, a), c, oc)
        if c.get_value_and_terminated()[1]:
            continue
        roots.append(((a,), c))
        for a2, m2 in zip(idx2, moves2):
            g, og = c.copy(), oc.copy()
            g.push_action(a2)
            og.move_piece(m2)
            assert_host_equals_oracle("%s child %d grandchild %d" % (tag, a, a2), g, og)
    return roots
