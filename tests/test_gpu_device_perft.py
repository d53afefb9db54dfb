"""The device's chess rules held to the public perft tables, move by move.

The host mirror and the oracle pass the seven public perft tables on the CPU (test_host_rules.py, test_oracle_chess.py).  The kernels run
the same sz_chess.h functions, but compiled for another target and composed differently: wave_movegen (a lane per square, the king's danger
set and en-passant legality from ballots, 73 ballots for the mask), wave_count_reps, wave_create_position and the move application of
k_play exist only on the device.  Here the SEARCH ITSELF enumerates every child of every root (the walk of tests/perftwalk.py: uniform
evaluator, C = 1e6, num_searches = K + 1; its driver is tested on the CPU in test_perft_walk_driver.py), so every node of the tables'
last two plies is created by wave_create_position, and every move of the ply above is applied by k_play.

For each table, d = the depth used (the table's deepest entry unless noted):
 (a) roots = all positions at depth d - 2 (host mirror moves, uploaded as live games with their ring); the sum of the DEVICE's root
     legal-mask popcounts is perft(d - 1) and the sum over all device-created children of their mask popcounts is perft(d);
 (b) every device-created child equals the host mirror's child: legal mask (73 words), 119 planes, terminal or not, loss or draw;
 (c) k_play: every position at depth d - 3 sits on K boards, copy i plays child i; the device's 80-byte position record (its own
     sz_finish_meta, key, repetition count, check flag; no field masked) and sz_fetch_ply's chosen / game_over / result equal the host's;
 (d) constructed rule endings the tables do not contain (rule_endings.py; expectations from the oracle), walked with (b) and (c).
Per board the walk asserts that exactly its K children were seen, each once: pending at depth 1, or terminal.  Nothing is skipped.
No tolerance anywhere: counts are the public numbers, everything else is exact equality.

Measured on MI355X (seconds are the pytest --durations figures of one run of the whole GPU suite, host-side enumeration included):
  table     depth  roots (d-2)  device-created nodes (terminal)  moves counted   (a)+(b)   (c) boards   (c)
  startpos    5        8,902        197,281   (8)                  4,865,609      3.5 s       8,902     0.8 s
  kiwipete    4        2,039         97,862   (1)                  4,085,603      1.4 s       2,039     0.2 s (both chess960 settings)
  pos3        6       43,238        674,624   (0)                 11,030,083     10.7 s      43,238     3.7 s
  pos4        5        9,467        422,333   (5)                 15,833,292      6.1 s       9,467     0.9 s
  pos5        4        1,486         62,379  (44)                  2,103,487      0.9 s       1,486     0.1 s
  pos6        4        2,079         89,890   (0)                  3,894,594      1.2 s       2,079     0.2 s
  c960        5       12,189        326,672   (0)                  8,146,062      4.9 s      12,189     1.1 s (12,139 boards, 1.1 s, with chess960 off)
Every table runs at its deepest entry: the slowest case here (pos3, 10.7 s) is below the slowest pre-existing case of the same run
(test_gpu_round3.py::test_bench_plain_run_is_the_headline_and_full_adds_the_side_measurements, 26.1 s), so no table was dropped a ply.
The ten rule endings take 0.01-0.2 s each; the whole module 39 s.
Teeth (shown once, not committed): a scratch library whose DEVICE code alone leaves the en-passant victim on the board in sz_make_move
passes the CPU perft tests and fails here by name, e.g. "kiwipete: root path [2292, 117], child action 3163: device differs from the host
mirror at legal-mask word 0" in (a)/(b) and "kiwipete: root path [112], child action 478: position record after k_play differs from the
host mirror's in pawns" in (c); likewise on pos3.
"""
import pytest

import perftwalk as W
import rule_endings as RE

pytestmark = pytest.mark.gpu

# depth d used per table; see the docstring for the time condition
DEPTH = {"startpos": 5, "kiwipete": 4, "pos3": 6, "pos4": 5, "pos5": 4, "pos6": 4, "c960": 5}
BOARDS_PER_ENGINE = 4096


@pytest.mark.parametrize("name", [p[0] for p in W.PERFT])
def test_device_created_nodes_match_perft_and_host_mirror(name):
    """(a) + (b)"""
    _, _, c960, want = W.PERFT_BY_NAME[name]
    d = DEPTH[name]
    assert 3 <= d <= len(want)
    total = W.WalkResult()
    for chunk in W.chunks(W.positions_at_depth(W.table_root(name), d - 2), BOARDS_PER_ENGINE):
        total.add(W.device_walk(name, chunk, c960, compare=True))
    print("%s: depth %d, %d roots, %d device-created nodes (%d terminal), %d moves counted" %
          (name, d, total.roots, total.children, total.terminal_children, total.child_moves))
    assert total.roots == want[d - 3]
    assert total.root_moves == want[d - 2] == total.children        # device root masks; one device-created child per root move
    assert total.child_moves == want[d - 1]                         # device child masks


PLAY = [(p[0], p[2]) for p in W.PERFT] + [("c960", False), ("kiwipete", True)]


@pytest.mark.parametrize("name,engine960", PLAY, ids=["%s-%s" % (n, "960" if c else "std") for n, c in PLAY])
def test_k_play_applies_every_legal_move(name, engine960):
    """(c).  Both chess960 settings of the engine for the Chess960 table (without the setting the FEN's castling rights do not survive
    clean_castling_rights, so that run holds no castling and is not held to the table's count) and for Kiwipete (castling spelled
    king-takes-rook: the same counts)."""
    _, _, c960, want = W.PERFT_BY_NAME[name]
    d = DEPTH[name]
    root = W.table_root(name, chess960=engine960)
    n = 0
    for chunk in W.chunks(W.positions_at_depth(root, d - 3), BOARDS_PER_ENGINE, weight=lambda r: len(r[1].legal_action_indices())):
        n += W.device_play("%s (engine chess960=%d)" % (name, engine960), chunk, engine960)
    print("%s: %d boards played" % (name, n))
    if engine960 or not c960:
        assert n == want[d - 3]
    else:
        assert n > 0


@pytest.mark.parametrize("case", RE.CASES, ids=[c[0] for c in RE.CASES])
def test_rule_endings_on_the_device(case):
    """(d): the game and each of its non-terminal children as roots, so an ending one move away is met by a device-created child and
    by k_play, and an ending two moves away by a device-created child of a child"""
    ct, oct_ = RE.build(case)
    roots = RE.two_levels(case[0], ct, oct_)
    res = W.device_walk(case[0], roots, False, compare=True)
    assert res.roots == len(roots) and res.children == res.root_moves > 0
    if case[4] in ("fivefold", "seventyfive", "insufficient"):
        assert res.terminal_children > 0
    assert W.device_play(case[0], roots, False) == res.children
