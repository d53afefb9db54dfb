"""CPU checks of proven-result propagation (sz_set_solver, a NON-REFERENCE option): the plain-Python restatement tests/solverref.py
equals vlref's search with the solver off, keeps the fixpoint of the rules with it on, and gives the known answers of constructed
positions; the case set exercises every rule (asserted, so a case set that stops doing so fails); the C ABI declares and exports the
entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import solver_cases as SC
import solverref
import vlref
from solverref import UNKNOWN, WIN, DRAW, LOSS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(golden_dir, name):
    with np.load(os.path.join(golden_dir, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _cases(z):
    for i in range(int(z["n_cases"])):
        yield i, {k[len("c%d_" % i):]: z[k] for k in z if k.startswith("c%d_" % i)}


def host_game(z, g, upto=None):
    import sigma_zero_amd as sz
    ct = sz.ChessTensor(chess960=bool(z["c960"][g]), scharnagl=int(z["scharnagl"][g]) if z["c960"][g] else None)
    lo, hi = z["move_off"][g], z["move_off"][g + 1]
    hi = hi if upto is None else min(hi, lo + upto)
    for f, t, p in z["moves"][lo:hi]:
        ct.move_piece(sz.Move(int(f), int(t), int(p) or None))
    return ct


def _same_search(a, b, tag):
    assert len(a.steps) == len(b.steps) and all(np.array_equal(x, y) for x, y in zip(a.steps, b.steps)), tag
    for x, y in zip(a.tree(), b.tree()):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), tag
    assert a.sims == b.sims, tag


def test_solver_off_is_vlref_at_L1(golden_dir):
    """the positions of tests/test_leaf_batching_ref.py (the reference's dyadic traces, which pin vlref, and its extra positions) and the
    solver's own case set: whole trees and every network input, bit for bit"""
    games = _load(golden_dir, "chess_tensor_games.npz")
    n = 0
    for i, case in _cases(_load(golden_dir, "chess_search_traces.npz")):
        if str(case["mode"]) != "dyadic":
            continue
        ct = host_game(games, int(case["game"]), int(case["ply"]))
        kw = dict(learning=bool(case["learning"]), mode="dyadic", salt=int(case["salt"]))
        _same_search(solverref.search(ct, int(case["S"]), solver=False, **kw), vlref.search(ct, int(case["S"]), L=1, **kw), "trace case %d" % i)
        n += 1
    assert n >= 30
    for g, ply in ((9, 5), (10, 60), (13, 150)):
        for S, learning in ((64, True), (150, False)):
            ct = host_game(games, g, ply)
            kw = dict(learning=learning, mode="dyadic", salt=g)
            _same_search(solverref.search(ct, S, solver=False, **kw), vlref.search(ct, S, L=1, **kw), "game %d ply %d" % (g, ply))
    for name, S, salt in SC.CASES:
        off = SC.run(name, S, salt, solver=False)
        _same_search(off, vlref.search(SC.game(name), S, L=1, mode="dyadic", salt=salt), name)
        assert not off.R.any() and not off.complete.any() and off.proved == off.proven_stops == off.skips == 0


@pytest.fixture(scope="module")
def solved():
    """every case, learning off and on, searched once with the solver on"""
    return {(name, S, salt, learning): SC.run(name, S, salt, learning=learning) for name, S, salt in SC.CASES for learning in (False, True)}


def test_fixpoint_and_counters(solved):
    for key, s in solved.items():
        SC.check_fixpoint(s, str(key))
        S = key[1]
        assert s.sims == S and int(s.N[0]) == 1 + S and s.expansions + s.terminal_hits == S, key
        assert s.expansions == len(s.steps), key
        assert s.proved == sum(s.proved_by_label.values()), key
        if s.root_proven_at is not None:                         # a proven root: every later simulation ended at the root
            assert s.R[0] != UNKNOWN and len(s.steps) <= s.root_proven_at, key


def _eval_root(s):
    """value of the root's one network evaluation: all the forced draw's root ever receives besides zeros"""
    from hashmodel import evaluate_packed
    return float(evaluate_packed(s.steps[0][0], s.mode, s.salt)[1])


def test_known_answers(solved):
    from sigma_zero_amd.chess_tensor import Move, action_index
    # mate in one
    for S, salt in ((64, 0), (200, 1)):
        s = solved[("mate_in_1", S, salt, False)]
        r, rc = s.root_proven()
        ct = SC.game("mate_in_1")
        mate = ct.legal_action_indices().index(action_index(Move.from_uci("a1a8"), True))
        assert r == WIN and rc[mate] == LOSS and s.choose(0.999) == mate and s.choose(-1.0) == mate
        assert s.root_proven_at < S and s.proven_stops == S - s.root_proven_at
    # 218 moves: four passes of 64 lanes, the proving child beyond the first
    for S, salt in ((200, 0), (64, 1)):
        s = solved[("moves_218", S, salt, False)]
        r, rc = s.root_proven()
        assert len(SC.game("moves_218").legal_action_indices()) == 218 and int(s.n[0]) > 192          # a few moves may lose their child to a zero prior
        assert r == WIN and int(np.nonzero(rc == LOSS)[0][0]) >= 64
    assert int(np.nonzero(solved[("moves_218", 200, 0, False)].root_proven()[1] == LOSS)[0][0]) >= 192
    # forced draw: complete root, one child
    s = solved[("forced_draw", 64, 0, False)]
    r, rc = s.root_proven()
    assert r == DRAW and rc.tolist() == [DRAW] and s.complete[0] == 1 and s.root_proven_at == 2 and len(s.steps) == 1
    assert s.W[0] == _eval_root(s) and s.proven_stops == 62
    # mated in two whatever it plays: every child WIN through its own LOSS grandchild
    for salt in (0, 2):
        s = solved[("mated_in_2", 200, salt, False)]
        r, rc = s.root_proven()
        assert r == LOSS and rc.tolist() == [WIN, WIN] and s.complete[0] == 1 and s.two_up >= 1
        for c in range(2):
            e = int(s.first[0]) + c
            assert (s.R[s.first[e]:s.first[e] + s.n[e]] == LOSS).sum() >= 1
    # a refuted move: the root stays open, the child is WIN, and the search stops visiting it
    for S in (200, 64):
        on, off = solved[("refuted_move", S, 2, False)], SC.run("refuted_move", S, 2, solver=False)
        r, rc = on.root_proven()
        assert r == UNKNOWN and (rc == WIN).sum() == 1 and on.skips > 0
        c = int(np.nonzero(rc == WIN)[0][0])
        assert SC.game("refuted_move").move_from_index(int(on.root_children()[0][c])).uci() == "g8h8"
        assert on.root_children()[1][c] < off.root_children()[1][c]
        assert not np.array_equal(on.root_children()[1], off.root_children()[1])


def test_case_set_exercises_every_rule(solved):
    """conditions, not measurements: counted over the case set at S <= 200, in the restatement alone"""
    assert all(S <= 200 for _, S, _ in SC.CASES)
    for learning in (False, True):
        runs = [s for k, s in solved.items() if k[3] == learning]
        for label in (WIN, DRAW, LOSS):
            assert sum(s.proved_by_label[label] for s in runs) >= 1, (learning, label)       # by the update rule, not merely terminal
        assert sum(s.two_up for s in runs) >= 1, learning                                   # a proof two levels above a terminal
        assert sum(s.skips for s in runs) >= 1, learning                                    # a selection that skipped a WIN child
        assert sum(1 for s in runs if s.root_proven_at is not None and s.root_proven_at < s.S) >= 1, learning
        assert sum(s.proven_stops for s in runs) >= 1, learning


def test_header_declares_and_library_exports_solver():
    with open(os.path.join(ROOT, "include", "sigmazero.h")) as f:
        h = f.read()
    assert re.search(r"int\s+sz_set_solver\s*\(\s*sz_engine\s*\*\s*e\s*,\s*int32_t\s+enable\s*,\s*void\s*\*\s*stream\s*\)", h)
    assert re.search(r"int\s+sz_root_proven\s*\(\s*sz_engine\s*\*\s*e\s*,\s*int8_t\s*\*\s*root_dev\s*,\s*int8_t\s*\*\s*child_dev\s*,\s*void\s*\*\s*stream\s*\)", h)
    assert re.search(r"int\s+sz_debug_tree_proven\s*\(", h) and re.search(r"int\s+sz_solver_stats\s*\(\s*sz_engine\s*\*\s*e\s*,\s*uint64_t\s+out\[2\]", h)
    assert "mate distance" in h
    from sigma_zero_amd import _native as N
    L = N.lib()
    for name in ("sz_set_solver", "sz_root_proven", "sz_debug_tree_proven", "sz_solver_stats"):
        assert hasattr(L, name) and name in N.EXPORTS
    assert (N.SZ_PROVEN_UNKNOWN, N.SZ_PROVEN_WIN, N.SZ_PROVEN_DRAW, N.SZ_PROVEN_LOSS) == (UNKNOWN, WIN, DRAW, LOSS) == (0, 1, 2, 3)
    # refusals that need no device: a NULL engine
    assert L.sz_set_solver(None, 1, None) == N.SZ_ERR_INVALID
    assert L.sz_root_proven(None, None, None, None) == N.SZ_ERR_INVALID
    n = C.c_int32(-1)
    assert L.sz_debug_tree_proven(None, 0, 0, None, None, C.byref(n), None) == N.SZ_ERR_INVALID
    out = (C.c_uint64 * 2)()
    assert L.sz_solver_stats(None, out, None) == N.SZ_ERR_INVALID
