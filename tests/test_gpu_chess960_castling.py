"""The device's Chess960 castling and its 960 start positions, exact against the host mirror, on the positions of tests/castling_lab.py.

The chain: device = host mirror here; host mirror = the rule-text generator in tests/test_plain_rules.py (CPU).  The plain generator is
not run here.  On the device the castling code is composed differently from the host's: the king's danger set comes from ballots over
I.need (the whole back rank as soon as one right exists), one lane runs sz_king_targets with an sz_attackers call on the relocated
occupancy, and sz_make_move meets the king-takes-rook spelling in wave_create_position and in k_play.

 (a) every lab position is a root, and so is every child of one reached by a castling or by the capture of a rook that carried a right
     (so what follows a castling is walked too: rights gone, rook on d/f).  perftwalk.device_walk(compare=True): the legal mask, the 119
     planes and terminal-or-not of every root and of every device-created child equal the host mirror's.
 (b) perftwalk.device_play: k_play applies every legal move of every such root; the 80-byte position record (castling word and hash key
     included) equals the host mirror's byte for byte.
 (c) one engine of 960 boards gets new_games(range(960)): every record equals the host mirror's for that number; the walk from those
     device-made starts agrees with the host mirror node by node, and the device's root-mask popcounts sum to the host's perft(1) total
     over the 960 (18,882), its child-mask popcounts to the perft(2) total (371,766), the totals test_plain_rules.py establishes against
     the plain generator.
Nothing is skipped, no tolerance.  A case is the lab positions of one king file.

Measured on MI355X (seconds are pytest's call durations, (a) + (b), host-side enumeration included, of a run of this module with
test_gpu_device_perft.py, whose slowest case, pos3, took 12.1 s in it; in a run of the whole GPU suite: pos3 12.2 s, king_e 3.7 s,
king_d 3.6 s.  Every case here stays below a third of pos3):
  king file  lab positions  roots  device-created nodes (terminal)  moves counted  k_play boards  seconds
      b           272         508        12,484  (26)                   318,096        12,484        2.0
      c           472         986        25,514  (50)                   637,860        25,514        2.7
      d           572       1,304        34,294  (66)                   845,806        34,294        3.6
      e           572       1,306        34,334  (64)                   850,392        34,334        3.6
      f           472       1,080        28,226  (50)                   698,846        28,226        2.9
      g           272         580        14,740  (24)                   369,122        14,740        1.5
  960 starts: 960 roots made by k_new_games, 18,882 device-created nodes, 371,766 moves counted, 0.4 s.
  In all 2,632 lab positions, 5,764 roots, 149,592 device-created nodes, 149,592 k_play boards.
Teeth (shown once, not committed): a scratch library whose DEVICE code alone tests the king's castling destination on I.occ ^ kb, without
the rook relocated.  The whole GPU suite of the parent commit passes on it (474 tests, test_gpu_device_perft.py's c960 table, the Chess960
runs of test_gpu_parity.py and the Chess960 fixtures of test_gpu_reference_golden.py among them): none notices.  This module fails it in
five of its seven cases, by position name: "king on the c-file: root path ['bce:shield_a']: device differs from the host mirror at
legal-mask word 42: got 0x1600000000000000, want 0x1200000000000000" (king c1, rook b1, black rook a1: the device castles), likewise
bde:, bef:, bfg: and bgh:shield_a; king_b (no square outside an a-rook on a1) and the start positions pass.  On the CPU the same alteration
in the host mirror alone passes the parent's whole CPU suite (307 tests, test_host_rules.py included) and fails test_plain_rules.py:
"bce:shield_a: legal moves differ: only the host mirror has ['c1b1'], only the plain generator has []".
"""
import numpy as np
import pytest

import sigma_zero_amd as sz
import perftwalk as W
import castling_lab as LAB

pytestmark = pytest.mark.gpu

BOARDS_PER_ENGINE = 4096
KING_FILES = sorted(LAB.LAB_BY_KING_FILE)


def lab_roots(king_file):
    """((name[, action]), game) for the lab positions of one king file and their children that take a right"""
    roots = []
    for name, fen in LAB.LAB_BY_KING_FILE[king_file]:
        ct = sz.ChessTensor(chess960=True, fen=fen)
        roots.append(((name,), ct))
        roots += [((name, a), ch) for a, ch in W.children_that_take_a_right(ct) if not ch.get_value_and_terminated()[1]]
    return roots


@pytest.mark.parametrize("king_file", KING_FILES, ids=["king_%s" % LAB.FILES[k] for k in KING_FILES])
def test_device_walks_the_castling_lab(king_file):
    """(a) + (b)"""
    tag = "king on the %s-file" % LAB.FILES[king_file]
    roots = lab_roots(king_file)
    n_lab = len(LAB.LAB_BY_KING_FILE[king_file])
    assert len(roots) >= n_lab + 8 * king_file * (7 - king_file)         # alone_a/_h castle and open_a/_h capture, either colour, per triple
    total = W.WalkResult()
    for chunk in W.chunks(roots, BOARDS_PER_ENGINE):
        total.add(W.device_walk(tag, chunk, True, compare=True))
    assert total.roots == len(roots) and total.children == total.root_moves > 0
    played = 0
    for chunk in W.chunks(roots, BOARDS_PER_ENGINE, weight=lambda r: len(r[1].legal_action_indices())):
        played += W.device_play(tag, chunk, True)
    print("%s: %d lab positions, %d roots, %d device-created nodes (%d terminal), %d moves counted, %d boards played"
          % (tag, n_lab, total.roots, total.children, total.terminal_children, total.child_moves, played))
    assert played == total.children


def test_device_start_positions_are_the_host_mirrors():
    """(c)"""
    from sigma_zero_amd.selfplay import SelfPlayEngine
    numbers = list(range(960))
    games = [sz.ChessTensor(chess960=True, scharnagl=n) for n in numbers]
    eng = SelfPlayEngine(None, {"C": W.WALK_C, "num_searches": 2}, 960, chess960=True, learning=False)
    try:
        eng.new_games(numbers)
        eng.check_errors()
        for n, g in zip(numbers, games):
            pos, ply = eng.debug_position(n)
            want = np.array(g.board.bitboards(), np.uint64)
            bad = np.nonzero(pos != want)[0]
            assert not len(bad) and ply == 0, "Scharnagl %d: the device's start record differs from the host mirror's in %s" % (
                n, [W.RECORD_WORDS[i] for i in bad])
    finally:
        eng.close()
    res = W.device_walk("960 starts", [((n,), g) for n, g in zip(numbers, games)], True, compare=True, scharnagl=numbers)
    p1, p2 = sum(g.perft(1) for g in games), sum(g.perft(2) for g in games)
    print("960 starts: %d root moves, %d device-created nodes, %d moves counted" % (res.root_moves, res.children, res.child_moves))
    assert res.roots == 960 and res.root_moves == res.children == p1 and res.child_moves == p2
