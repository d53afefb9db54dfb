"""CPU checks of leaf batching with virtual loss (sz_set_leaf_batching, a NON-REFERENCE option): the plain-Python restatement
(tests/vlref.py) reproduces the reference's own search traces at L = 1 and keeps the invariants of the option at L > 1; the C ABI
declares and exports the entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vlref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(golden_dir, name):
    with np.load(os.path.join(golden_dir, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _cases(z):
    for i in range(int(z["n_cases"])):
        yield i, {k[len("c%d_" % i):]: z[k] for k in z if k.startswith("c%d_" % i)}


@pytest.fixture(scope="module")
def games(golden_dir):
    return _load(golden_dir, "chess_tensor_games.npz")


def host_game(z, g, upto=None):
    import sigma_zero_amd as sz
    ct = sz.ChessTensor(chess960=bool(z["c960"][g]), scharnagl=int(z["scharnagl"][g]) if z["c960"][g] else None)
    lo, hi = z["move_off"][g], z["move_off"][g + 1]
    hi = hi if upto is None else min(hi, lo + upto)
    for f, t, p in z["moves"][lo:hi]:
        ct.move_piece(sz.Move(int(f), int(t), int(p) or None))
    return ct


def test_restatement_at_L1_reproduces_reference_traces(games, golden_dir):
    """L = 1: every dyadic case of the reference's MCTS0.search traces, bit for bit (network inputs in order, whole tree)"""
    tr = _load(golden_dir, "chess_search_traces.npz")
    n = 0
    for i, case in _cases(tr):
        if str(case["mode"]) != "dyadic":
            continue
        tag = "case %d game %d ply %d S=%d learning=%d" % (i, case["game"], case["ply"], case["S"], case["learning"])
        ct = host_game(games, int(case["game"]), int(case["ply"]))
        s = vlref.search(ct, int(case["S"]), learning=bool(case["learning"]), L=1, mode="dyadic", salt=int(case["salt"]))
        inputs = np.concatenate(s.steps) if s.steps else np.zeros((0, 119, 8), np.uint8)
        assert all(len(st) == 1 for st in s.steps) and s.collisions == 0, tag
        assert np.array_equal(inputs, case["leaf_planes"]), tag
        d, a, v, w, p = s.tree()
        assert int(v[0]) == int(case["root_visits"]) and w[0] == float(case["root_value_sum"]), tag
        assert np.array_equal(d[1:], case["tree_depth"]) and np.array_equal(a[1:], case["tree_action"]), tag
        assert np.array_equal(v[1:], case["tree_visits"]), tag
        assert np.array_equal(w[1:], case["tree_value_sum"]), tag
        assert np.array_equal(p[1:].view(np.uint32), case["tree_prior"].view(np.uint32)), tag
        n += 1
    assert n >= 30


def _decisive_late_positions(z, back=3, limit=4):
    """positions a few plies before the end of decisive games: trees there reach terminal (mate) leaves"""
    out = []
    for g in range(int(z["n_games"])):
        if int(z["result"][g]) in (1, -1):
            n_moves = int(z["move_off"][g + 1] - z["move_off"][g])
            if n_moves > back:
                out.append((g, n_moves - back))
        if len(out) >= limit:
            break
    return out


@pytest.mark.parametrize("L,lam", [(2, 1.0), (7, 0.5), (32, 0.0), (16, 1.0), (8, 0.0)])
def test_restatement_invariants_at_L_above_1(games, L, lam):
    """k back to zero, root N = 1 + S, at most S network calls, every call carries 1..L leaves; the cases include collisions and
    terminal leaves met while a gather had leaves pending"""
    z = games
    positions = [(9, 5), (10, 60), (13, 150)] + _decisive_late_positions(z)
    collisions = terminals = 0
    for g, ply in positions:
        for S, learning in ((64, True), (150, False)):
            ct = host_game(z, g, ply)
            if ct.get_value_and_terminated()[1]:
                continue
            s = vlref.search(ct, S, learning=learning, L=L, lam=lam, mode="dyadic", salt=g)
            tag = "game %d ply %d S=%d L=%d" % (g, ply, S, L)
            assert not s.K.any(), tag
            assert int(s.N[0]) == 1 + S and s.sims == S, tag
            assert 1 <= len(s.steps) <= S and all(1 <= len(st) <= L for st in s.steps), tag
            assert sum(len(st) for st in s.steps) + int((s.term[:s.n_edges] == 1).sum()) >= 1, tag
            collisions += s.collisions
            terminals += s.gather_terminals
    assert terminals > 0, terminals
    assert collisions > 0 or lam > 0, collisions                  # without a virtual loss repeated descents collide at once


def test_L_above_1_differs_from_L1_and_uses_fewer_calls(games):
    ct = host_game(games, 10, 60)
    s1 = vlref.search(ct, 100, L=1, mode="dyadic")
    s8 = vlref.search(ct, 100, L=8, lam=1.0, mode="dyadic")
    assert len(s1.steps) == 100 and len(s8.steps) < 50
    assert int(s8.root_children()[1].sum()) == int(s1.root_children()[1].sum()) == 99


def test_header_declares_and_library_exports_leaf_batching():
    with open(os.path.join(ROOT, "include", "sigmazero.h")) as f:
        h = f.read()
    assert re.search(r"int\s+sz_set_leaf_batching\s*\(\s*sz_engine\s*\*\s*e\s*,\s*int32_t\s+leaves_per_step\s*,\s*float\s+virtual_loss\s*,\s*void\s*\*\s*stream\s*\)", h)
    assert re.search(r"int\s+sz_pending_boards\s*\(", h)
    assert re.search(r"#define\s+SZ_MAX_LEAVES_PER_STEP\s+256", h)
    from sigma_zero_amd import _native as N
    L = N.lib()
    for name in ("sz_set_leaf_batching", "sz_pending_boards"):
        assert hasattr(L, name) and name in N.EXPORTS
    assert N.SZ_MAX_LEAVES_PER_STEP == 256
    # refusals that need no device: a NULL engine
    assert L.sz_set_leaf_batching(None, 2, 1.0, None) == N.SZ_ERR_INVALID
    n = C.c_int32(-1)
    assert L.sz_pending_boards(None, C.byref(n), None) == N.SZ_ERR_INVALID
