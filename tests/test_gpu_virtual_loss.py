"""Leaf batching with virtual loss on the GPU (sz_set_leaf_batching, a NON-REFERENCE option): the HIP engine against the plain-Python
restatement tests/vlref.py, bit for bit (whole trees, every network input row, number of network calls), plus the Python surface."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
from hashmodel import HashModel, evaluate_packed, pack_planes
import vlref

pytestmark = pytest.mark.gpu


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
    ct = sz.ChessTensor(chess960=bool(z["c960"][g]), scharnagl=int(z["scharnagl"][g]) if z["c960"][g] else None)
    lo, hi = z["move_off"][g], z["move_off"][g + 1]
    hi = hi if upto is None else min(hi, lo + upto)
    for f, t, p in z["moves"][lo:hi]:
        ct.move_piece(sz.Move(int(f), int(t), int(p) or None))
    return ct


def _groups(games, golden_dir):
    """dyadic fixture cases + a few extra positions at S = 200, grouped by what an engine fixes: (S, learning, chess960) -> [(game, salt)]"""
    out = {}
    for i, case in _cases(_load(golden_dir, "chess_search_traces.npz")):
        if str(case["mode"]) == "dyadic":
            g = int(case["game"])
            out.setdefault((int(case["S"]), bool(case["learning"]), bool(games["c960"][g])), []).append((host_game(games, g, int(case["ply"])), int(case["salt"])))
    for learning in (False, True):
        for g, ply in ((9, 5), (10, 60), (13, 150), (17, 40)):
            out.setdefault((200, learning, bool(games["c960"][g])), []).append((host_game(games, g, ply), g))
    return out


def _engine_vs_ref(items, S, learning, c960, L, lam):
    """one engine, board b = items[b]; every step: pending boards, network rows and step count against the restatement; then whole trees"""
    refs = [vlref.search(ct, S, learning=learning, L=L, lam=lam, mode="dyadic", salt=salt) for ct, salt in items]
    B = len(items)
    eng = SelfPlayEngine(None, {"C": 2, "num_searches": S, "leaves_per_step": L, "virtual_loss": lam}, B, chess960=c960, learning=learning,
                         edges_per_board=S * 64 + 256)
    for b, (ct, _) in enumerate(items):
        eng.upload_game(b, ct)
    eng.begin()
    t = 0
    while True:
        torch.cuda.synchronize()
        status = eng.debug_pending()[4]
        pend = (status & 2) != 0
        assert pend.tolist() == [t < len(r.steps) for r in refs], "step %d: boards waiting for the network" % t
        if not pend.any():
            break
        assert t < S
        planes = pack_planes(eng.planes.float().cpu().numpy())
        pol = np.zeros((B * L, N.SZ_ACTIONS), np.float32)
        val = np.zeros(B * L, np.float32)
        for b in np.nonzero(pend)[0]:
            want = refs[b].steps[t]
            got = planes[b * L:b * L + len(want)]
            assert np.array_equal(got, want), "step %d board %d: network input rows differ" % (t, b)
            for i in range(len(want)):
                pol[b * L + i], val[b * L + i] = evaluate_packed(want[i], "dyadic", items[b][1])
        eng.step(torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda())
        t += 1
    assert t == max(len(r.steps) for r in refs)
    st = eng.check_errors()
    assert st["simulations"] == S * B and st["boards_pending"] == 0
    for b, r in enumerate(refs):
        d, a, v, w, p = eng.debug_tree(b)
        rd, ra, rv, rw, rp = r.tree()
        tag = "board %d S=%d L=%d lam=%g learning=%d" % (b, S, L, lam, learning)
        assert np.array_equal(d, rd) and np.array_equal(a, ra) and np.array_equal(v, rv), tag
        assert w.tobytes() == rw.tobytes() and p.tobytes() == rp.tobytes(), tag
        assert int(v[0]) == 1 + S
    eng.close()
    return refs


# ------------------------------------------------------------------------------------------------ 1. L = 1 is today's engine
def test_set_leaf_batching_L1_changes_nothing(games, golden_dir):
    items = [it for (S, learning, c960), its in _groups(games, golden_dir).items() if not c960 for it in its][:24]
    snaps = []
    for g in range(int(games["n_games"])):
        if games["c960"][g]:
            continue
        n = int(games["move_off"][g + 1] - games["move_off"][g])
        for ply in range(0, n, 7):
            ct = host_game(games, g, ply)
            if not ct.get_value_and_terminated()[1]:
                snaps.append(ct)
    positions = [ct for ct, _ in items] + snaps[:64]
    assert len(positions) >= 64 + 20
    trees = []
    for call in (False, True):
        eng = SelfPlayEngine(HashModel(), {"C": 2, "num_searches": 48}, len(positions), learning=True)
        if call:
            N.check(N.lib().sz_set_leaf_batching(eng._e, 1, 0.5, eng._stream()), "sz_set_leaf_batching")
        for b, ct in enumerate(positions):
            eng.upload_game(b, ct)
        eng.search()
        eng.check_errors()
        assert eng.last_steps == 48
        trees.append([eng.debug_tree(b) for b in range(len(positions))])
        eng.close()
    for b in range(len(positions)):
        for x, y in zip(trees[0][b], trees[1][b]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "board %d" % b       # bitwise: a prior may be NaN (policy 0 on every move)


# ------------------------------------------------------------------------------------------------ 2. engine == restatement
@pytest.mark.parametrize("L", [2, 7, 32])
@pytest.mark.parametrize("lam", [1.0, 0.5, 0.0])
def test_engine_matches_restatement(games, golden_dir, L, lam):
    n = 0
    for (S, learning, c960), items in sorted(_groups(games, golden_dir).items(), key=lambda kv: kv[0]):
        _engine_vs_ref(items, S, learning, c960, L, lam)
        n += len(items)
    assert n >= 30 + 8


# ------------------------------------------------------------------------------------------------ 3. boards are independent
def test_many_boards_search_as_if_alone(games):
    S, L, lam = 48, 8, 1.0
    args = {"C": 2, "num_searches": S, "leaves_per_step": L, "virtual_loss": lam}
    live, terminal = [], []
    for g in range(int(games["n_games"])):
        if games["c960"][g]:
            continue
        n = int(games["move_off"][g + 1] - games["move_off"][g])
        end = host_game(games, g)
        if end.get_value_and_terminated()[1]:
            terminal.append(end)
        for ply in range(0, n, 11):
            ct = host_game(games, g, ply)
            if not ct.get_value_and_terminated()[1]:
                live.append(ct)
    positions = (live[:86] + terminal[:4] * 3)[:96]
    B = len(positions)
    active = np.array([0 if b % 13 == 5 else 1 for b in range(B)], np.uint8)
    eng = SelfPlayEngine(HashModel(), args, B, learning=True)
    for b, ct in enumerate(positions):
        eng.upload_game(b, ct)
    eng.set_active(active)
    n_live = eng.compact()
    assert n_live == int(active.sum())
    eng.search()
    st = eng.check_errors()
    assert st["boards_pending"] == 0 and eng.last_steps <= S
    n_term = 0
    one = SelfPlayEngine(HashModel(), args, 1, learning=True)          # one single-board engine, each position uploaded in turn
    for b, ct in enumerate(positions):
        d, a, v, w, p = eng.debug_tree(b)
        if not active[b]:
            assert len(d) == 0
            continue
        one.upload_game(0, ct)
        one.search()
        one.check_errors()
        for x, y in zip((d, a, v, w, p), one.debug_tree(0)):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "board %d" % b
        if ct.get_value_and_terminated()[1]:
            assert len(d) == 1 and int(v[0]) == 1 + S
            n_term += 1
    assert n_term >= 3
    one.close()
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. MCTS0 front-end
def test_mcts0_leaves_per_step(games):
    ct = host_game(games, 10, 60)
    m = sz.MCTS0(game=ct, args={"C": 2, "num_searches": 200, "leaves_per_step": 16}, model=HashModel())
    probs = m.search(ct.board, verbose=False, learning=False)
    r = vlref.search(ct, 200, learning=False, L=16, lam=1.0, mode="dyadic", salt=0)
    acts, vis = r.root_children()
    want = {ct.move_from_index(int(x)): int(n) / int(vis.sum()) for x, n in zip(acts, vis)}
    assert list(probs.keys()) == list(want.keys()) and list(probs.values()) == list(want.values())
    from sigma_zero_amd.fastnet import FastPolicyNet
    torch.manual_seed(0)
    fast = FastPolicyNet(sz.policyNN({}).cuda().eval())
    for g, ply in ((10, 60), (0, 3)):
        ct = host_game(games, g, ply)
        m = sz.MCTS0(game=ct, args={"C": 2, "num_searches": 64, "leaves_per_step": 16}, model=fast)
        probs = m.search(ct.board, verbose=False, learning=False)
        legal = {(x.from_square, x.to_square, x.promotion or 0) for x in ct.get_moves()}
        assert {(x.from_square, x.to_square, x.promotion or 0) for x in probs} == legal
        assert abs(sum(probs.values()) - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------------ 5. self-play with compaction
class _IntHashNet:
    """a deterministic network stand-in on the GPU: integer arithmetic only, so its output does not depend on the batch size or row order"""

    def __init__(self):
        gen = torch.Generator().manual_seed(7)
        self.m = torch.randint(1, 1 << 20, (119 * 64,), generator=gen, dtype=torch.int64).cuda()
        self.a = torch.randint(1, 1 << 15, (N.SZ_ACTIONS,), generator=gen, dtype=torch.int64).cuda()
        self.c = torch.randint(0, 1 << 30, (N.SZ_ACTIONS,), generator=gen, dtype=torch.int64).cuda()
        self._p = torch.zeros(1, device="cuda")

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def parameters(self):
        yield self._p

    def __call__(self, x, inference=True):
        key = (x.reshape(x.shape[0], -1).to(torch.int64) * self.m).sum(1)
        h = (key[:, None] * self.a + self.c) >> 9
        return ((h & 63) + 1).float() / 1024.0, (((key % 201) - 100).float() / 128.0).view(-1, 1)


def test_play_games_with_leaf_batching_compact_on_off():
    from sigma_zero_amd.sim import play_games
    net = _IntHashNet()
    args = {"C": 2, "num_searches": 16, "leaves_per_step": 8}
    u = lambda g, ply: ((g * 7919 + ply * 104729) % 997) / 997.0
    runs = [play_games(net, args, 5, uniforms=u, n_boards=2, compact=c, max_plies=3000) for c in (True, False)]
    for g in range(5):
        a, b = runs[0][g], runs[1][g]
        assert a["result"] is not None, "game %d did not end" % g
        assert a["result"] == b["result"] and a["rewards"] == b["rewards"] and a["colours"] == b["colours"]
        assert [list(x.items()) for x in a["actions"]] == [list(x.items()) for x in b["actions"]]
        assert all(np.array_equal(x, y) for x, y in zip(a["packed_states"], b["packed_states"]))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    lib = N.lib()
    eng = SelfPlayEngine(HashModel(), {"C": 2, "num_searches": 8}, 2, learning=False)
    s = eng._stream()
    for L, lam in ((0, 1.0), (257, 1.0), (-3, 1.0), (2, -1.0), (2, float("nan")), (2, float("inf")), (2, -0.5)):
        assert lib.sz_set_leaf_batching(eng._e, L, lam, s) == N.SZ_ERR_INVALID, (L, lam)
    eng.new_games([-1, -1])
    eng.begin()
    assert lib.sz_set_leaf_batching(eng._e, 1, 1.0, s) == N.SZ_ERR_STATE          # in the middle of a search
    assert eng.pending_boards() == 2
    eng.search()
    eng.check_errors()
    assert eng.pending_boards() == 0
    assert lib.sz_set_leaf_batching(eng._e, 1, 1.0, s) == N.SZ_OK                 # between searches
    eng.close()
    reuse = SelfPlayEngine(None, {"C": 2, "num_searches": 8, "reuse_subtree": True}, 2, learning=False)
    assert lib.sz_set_leaf_batching(reuse._e, 2, 1.0, reuse._stream()) == N.SZ_ERR_INVALID
    assert lib.sz_set_leaf_batching(reuse._e, 1, 1.0, reuse._stream()) == N.SZ_OK
    reuse.close()
    for bad in ({"leaves_per_step": 0}, {"leaves_per_step": 257}, {"leaves_per_step": 2.5}, {"virtual_loss": -1.0}, {"virtual_loss": float("nan")},
                {"leaves_per_step": 4, "reuse_subtree": True}):
        with pytest.raises(ValueError):
            SelfPlayEngine(None, dict({"C": 2, "num_searches": 8}, **bad), 2)
    # the engine still works after every refusal
    ok = SelfPlayEngine(HashModel(), {"C": 2, "num_searches": 8, "leaves_per_step": 4}, 2, learning=False)
    ok.new_games([-1, -1])
    ok.search()
    assert ok.check_errors()["simulations"] == 16
    ok.close()
