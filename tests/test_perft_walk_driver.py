"""The driver of tests/test_gpu_device_perft.py on the CPU (no GPU needed): the walk of tests/perftwalk.py — uniform evaluator, C = 1e6,
num_searches = K + 1 — run on the oracle's search (oracle.Search.on_chess) really visits every root child exactly once, in index
order, and the pending leaves' legal-move counts sum to perft(2); the host-side arrays the device is compared with reproduce the
public perft numbers; and the constructed rule endings do what their names say, with the host mirror equal to the oracle on every
child and grandchild.  This keeps the GPU harness honest on a machine without a GPU."""
import numpy as np
import pytest

import perftwalk as W
import rule_endings as RE
from oracle import oracle as O

WALK_ROOTS = [
    ("kiwipete", W.PERFT_BY_NAME["kiwipete"][1], W.PERFT_BY_NAME["kiwipete"][3][1]),
    ("pos3", W.PERFT_BY_NAME["pos3"][1], W.PERFT_BY_NAME["pos3"][3][1]),
    ("mate_in_one", W.MATE_IN_ONE, None),            # 20 moves, one of them mate
    ("max_fanout", W.MAX_FANOUT, None),              # 218 moves, most of them mate or stalemate
]


def _terminal_children(fen):
    oct_ = O.ChessTensor.from_fen(fen)
    out = []
    for m in oct_.legal_action_indices()[1]:
        c = oct_.copy()
        c.move_piece(m)
        out.append(c.get_value_and_terminated()[1])
    return out


@pytest.mark.parametrize("name,fen,perft2", WALK_ROOTS, ids=[r[0] for r in WALK_ROOTS])
@pytest.mark.parametrize("extra", [0, 7])
def test_walk_visits_every_root_child_once_in_index_order(name, fen, perft2, extra):
    """extra > 0: boards of one engine share num_searches, so a board may get more than K + 1 simulations; the children are still all
    created first, in the same order (oracle_walk asserts that no child appears after a deeper leaf)"""
    K, vis, order, leaf_total, root_legal = W.oracle_walk(O.ChessTensor.from_fen(fen), extra=extra)
    term = _terminal_children(fen)
    if perft2 is None:
        perft2 = O.Board.from_fen(fen).perft(2)
    assert root_legal == K == len(term) == O.Board.from_fen(fen).perft(1)
    assert order == [i for i in range(K) if not term[i]]          # ascending, each once, exactly the non-terminal children
    assert leaf_total == perft2
    if extra == 0:
        assert vis == [1] * K
    else:
        assert min(vis) >= 1 and sum(vis) == K + extra
    if name == "mate_in_one":
        assert sum(term) == 1 and K == 20
    if name == "max_fanout":
        assert K == 218 and sum(term) == 182


def test_usual_c_does_not_walk():
    """at C = 2 a mating child is selected again and again (q = 1): the other children are never created.  C must stay huge."""
    K, vis, order, _, _ = W.oracle_walk(O.ChessTensor.from_fen(W.MATE_IN_ONE), c=2.0)
    assert vis != [1] * K and min(vis) == 0 and max(vis) > 1
    assert len(order) < K - 1


def test_host_level_arrays_reproduce_the_public_numbers():
    """the arrays the device is compared with (HostLevel: masks, packed planes, records, terminal flags) on Kiwipete's 48 children and
    their 2,039 children, and the mask / plane packing against the plain accessors"""
    want = W.PERFT_BY_NAME["kiwipete"][3]
    roots = list(W.positions_at_depth(W.table_root("kiwipete"), 1))
    H = W.HostLevel(roots)
    assert len(roots) == want[0] and W.popcount(H.mask) == want[1] == len(H.c_mask) and W.popcount(H.c_mask) == want[2]
    assert (H.c_nlegal == [W.popcount(m) for m in H.c_mask]).all()
    for r in (0, 17, 47):
        g = roots[r][1]
        acts = g.legal_action_indices()
        assert [p * 64 + v for p in range(73) for v in range(64) if (int(H.mask[r, p]) >> v) & 1] == acts
        rep = g.get_representation().numpy().astype(np.uint8).reshape(119, 64)
        assert all(int(H.planes[r, p]) == sum(int(rep[p, q]) << q for q in range(64)) for p in range(119))
        for i in (0, len(acts) - 1):
            c = g.copy()
            c.push_action(acts[i])
            k = int(H.o[r]) + i
            assert [int(x) for x in H.c_record[k]] == c.board.bitboards() and H.c_action[k] == acts[i]
            assert bool(H.c_term[k]) == c.get_value_and_terminated()[1]
            rep = c.get_representation().numpy().astype(np.uint8).reshape(119, 64)
            assert all(int(H.c_planes[k, p]) == sum(int(rep[p, q]) << q for q in range(64)) for p in range(119))
    # terminal children are flagged with their value: the mate-in-one root
    import sigma_zero_amd as sz
    H = W.HostLevel([((), sz.ChessTensor(fen=W.MATE_IN_ONE))])
    assert int(H.c_term.sum()) == 1 == int(H.c_loss.sum()) and H.K_live[0] == 20


def test_sample_uniforms_select_the_intended_child():
    """the uniform handed to sz_play lies inside child i's interval of np.random.choice's cdf, also with unequal visit counts"""
    visits = np.array([[1, 3, 1, 2, 0, 0], [5, 1, 1, 1, 1, 1]], np.int32)
    n_child = np.array([4, 6])
    for i in range(4):
        u = W.sample_uniforms(visits, n_child, np.array([i, i]))
        assert [O.sample_move(visits[b, :n_child[b]], u[b]) for b in range(2)] == [i, i]


@pytest.mark.parametrize("case", RE.CASES, ids=[c[0] for c in RE.CASES])
def test_rule_endings_host_mirror_equals_oracle(case):
    ct, oct_ = RE.build(case)
    roots = RE.two_levels(case[0], ct, oct_)
    assert roots[0][1] is ct and (len(roots) >= 2 or case[0] == "clock_149")       # at clock 149 every reply ends the game
