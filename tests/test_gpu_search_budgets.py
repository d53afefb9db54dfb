"""Per-board search budgets with in-search batch shrinking on the GPU (sz_set_search_budgets / sz_compact_searching, a NON-REFERENCE
option).  The specification is exact: a board searched with budget s inside a mixed batch has, bit for bit, the tree it has in an
engine created with num_searches = s; so every check here compares the mixed engine with uniform engines (L = 1) or with the
plain-Python restatement tests/vlref.py run with S = s (leaf batching)."""
import os
import random

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine, search_segments, unpack_bits128
from hashmodel import HashModel, evaluate_packed, pack_planes
import rule_endings
import vlref

pytestmark = pytest.mark.gpu

CAP = 64                      # num_searches of the mixed engine: the capacity
TREE_KEYS = ("depth", "action", "visits", "value_sum", "prior")
COUNTERS = ("simulations", "expansions", "terminal_hits", "sum_depth", "sum_children")


# ------------------------------------------------------------------------------------------------ positions
def _load(golden_dir, name):
    with np.load(os.path.join(golden_dir, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def host_game(z, g, upto=None):
    ct = sz.ChessTensor(chess960=bool(z["c960"][g]), scharnagl=int(z["scharnagl"][g]) if z["c960"][g] else None)
    lo, hi = z["move_off"][g], z["move_off"][g + 1]
    hi = hi if upto is None else min(hi, lo + upto)
    for f, t, p in z["moves"][lo:hi]:
        ct.move_piece(sz.Move(int(f), int(t), int(p) or None))
    return ct


def _ending(name, then=None):
    ct, _ = rule_endings.build(next(c for c in rule_endings.CASES if c[0] == name))
    if then:
        ct.move_piece(sz.Move.from_uci(then))
    return ct


@pytest.fixture(scope="module")
def positions(golden_dir):
    """24 boards for a Chess960 engine: the classical start (Scharnagl 518) and Chess960 starts, positions some plies into scripted Chess960
    games, and constructed endings: one whose every move ends the game (75-move rule: terminal leaves only) and, LAST, a finished game
    (insufficient material: a terminal root)."""
    z = _load(golden_dir, "chess_tensor_games.npz")
    out = [sz.ChessTensor(chess960=True, scharnagl=n) for n in (518, 0, 959, 333, 702)]
    c960 = [g for g in range(int(z["n_games"])) if z["c960"][g]]
    assert len(c960) >= 3
    ply = 3
    while len(out) < 22:
        for g in c960:
            n = int(z["move_off"][g + 1] - z["move_off"][g])
            if ply < n and len(out) < 22:
                ct = host_game(z, g, ply)
                if not ct.get_value_and_terminated()[1]:
                    out.append(ct)
        ply += 7
        assert ply < 400
    out.append(_ending("clock_149"))
    out.append(_ending("kb_v_k_by_capture", then="a1b2"))
    assert out[-1].get_value_and_terminated()[1] and not out[-2].get_value_and_terminated()[1]
    return out


def _budgets(values, n, keep_last=None):
    """n budgets from `values` so that each value occurs and neighbours differ"""
    b = [values[(i * 5 + i // len(values)) % len(values)] for i in range(n)]
    for i in range(1, n):
        if b[i] == b[i - 1]:
            b[i] = values[(values.index(b[i]) + 1) % len(values)]
    if keep_last is not None:
        b[-1] = keep_last
    assert set(b) == set(values) and all(x != y for x, y in zip(b[:-2], b[1:-1]))
    return b


# ------------------------------------------------------------------------------------------------ evaluators
def _to_nchw(planes, dtype):
    if dtype == "bits128":
        planes = unpack_bits128(planes)
    if dtype in ("bits128", "nhwc128"):
        return planes[:, :, :119].transpose(1, 2).reshape(planes.shape[0], 119, 8, 8).float()
    return planes.float()


_NETS = {}


def _net(kind):
    """the network behind an evaluator kind; the MFMA networks are built once (random-init weights, fixed seed)"""
    if kind not in _NETS:
        if kind in ("dyadic", "rational"):
            _NETS[kind] = HashModel(mode=kind, salt=11)
        else:
            from sigma_zero_amd.fastnet import FastPolicyNet, SplitPolicyNet
            torch.manual_seed(0)
            base = sz.policyNN({}).cuda().eval()
            _NETS["fast16"] = FastPolicyNet(base, operands="fp16")
            _NETS["split"] = SplitPolicyNet(base)
    return _NETS[kind]


class Recorder:
    """evaluator(planes) -> (policy, value) that keeps every batch it was handed"""

    def __init__(self, kind, dtype):
        self.net, self.kind, self.dtype, self.calls = _net(kind), kind, dtype, []

    def __call__(self, planes):
        self.calls.append(planes.clone())
        x = _to_nchw(planes, self.dtype) if self.kind in ("dyadic", "rational") else planes
        with torch.no_grad():
            policy, value = self.net(x, inference=True)
        return policy.float().contiguous(), value.float().reshape(-1).contiguous()


def _dtype_for(kind):
    return torch.float32 if kind in ("dyadic", "rational") else "bits128"


def _tree(eng, b):
    return tuple(x.tobytes() for x in eng.debug_tree(b))


def _roots(eng):
    action, visits, n_child, prior, wsum = eng.root_children()
    return [tuple(x[b].tobytes() for x in (action, visits, prior, wsum)) + (int(n_child[b]),) for b in range(eng.B)]


def _ply_records(eng, boards):
    rec = eng.fetch_ply()
    out = []
    for b in boards:
        pos, ply = eng.debug_position(b)
        out.append(tuple(rec[k][b].tobytes() for k in sorted(rec)) + (pos.tobytes(), ply))
    return out


# ------------------------------------------------------------------------------------------------ the two sides
_UNIFORM = {}


def uniform_run(pos_list, key, s, kind, dtype, L=1, lam=1.0, play_u=None):
    """an engine created with num_searches = s on these positions, stepped by hand: per board its tree, root children, the network
    rows it wrote at each of ITS steps (raw, in the engine's layout), optionally its ply record; and the engine's counters"""
    ck = (key, s, kind, str(dtype), L, lam, play_u)
    if ck in _UNIFORM:
        return _UNIFORM[ck]
    B = len(pos_list)
    args = {"C": 2, "num_searches": s}
    if L > 1:
        args.update(leaves_per_step=L, virtual_loss=lam)
    eng = SelfPlayEngine(None, args, B, chess960=True, learning=True, planes_dtype=dtype)
    for b, ct in enumerate(pos_list):
        eng.upload_game(b, ct)
    ev = Recorder(kind, dtype)
    rows = [[] for _ in range(B)]
    eng.begin()
    for t in range(s + 1):
        torch.cuda.synchronize()
        pend = (eng.debug_pending()[4] & 2) != 0
        if not pend.any():
            break
        assert t < s
        for b in np.nonzero(pend)[0]:
            rows[b].append(eng.planes[b * L:(b + 1) * L].clone())
        eng.step(*ev(eng.planes))
    st = eng.check_errors() if s != 1 or play_u is None else eng.stats()
    out = dict(trees=[_tree(eng, b) for b in range(B)], roots=_roots(eng), rows=rows, stats=st)
    if play_u is not None:
        eng.play([play_u] * B)
        out["ply"] = _ply_records(eng, range(B))
    eng.close()
    _UNIFORM[ck] = out
    return out


def mixed_engine(positions, kind, dtype, L=1, lam=1.0, max_shrinks=4, inactive=()):
    args = {"C": 2, "num_searches": CAP, "max_shrinks": max_shrinks}
    if L > 1:
        args.update(leaves_per_step=L, virtual_loss=lam)
    eng = SelfPlayEngine(None, args, len(positions), chess960=True, learning=True, planes_dtype=dtype)
    for b, ct in enumerate(positions):
        eng.upload_game(b, ct)
    if inactive:
        eng.set_active([0 if b in inactive else 1 for b in range(len(positions))])
        assert eng.compact() == len(positions) - len(inactive)
    return eng


def references(positions, budgets, kind, dtype, skip=(), **kw):
    """per board of the mixed batch: (uniform run of its budget, its index in that run)"""
    ref = {}
    for s in sorted(set(budgets)):
        idx = [b for b in range(len(positions)) if budgets[b] == s and b not in skip]
        if idx:
            run = uniform_run([positions[b] for b in idx], tuple(idx), s, kind, dtype, **kw)
            for i, b in enumerate(idx):
                ref[b] = (run, i)
    return ref


def check_rows(eng, rec, budgets, ref, L=1):
    """test 5: what the evaluator was handed, call by call, against the uniform engines' own rows"""
    segs = search_segments(eng.budgets, L, eng.max_shrinks)
    starts = np.concatenate([[0], np.cumsum(segs)]).tolist()
    t, total = 0, 0
    for i, n in enumerate(segs):
        # boards that still searched when the segment began, in board order: their uniform search had more than starts[i] steps
        live = [b for b in sorted(ref) if len(ref[b][0]["rows"][ref[b][1]]) > starts[i]]
        assert len(live) <= sum(1 for b in ref if -(-budgets[b] // L) > starts[i])                 # the issue's condition: at most the boards whose budget exceeds the segment end
        for k in range(n):
            if t >= len(rec.calls):
                break                                        # every board was done at a shrink: the search stopped there
            got = rec.calls[t]
            assert got.shape[0] == len(live) * L, "call %d (segment %d): %d rows for %d live boards" % (t, i, got.shape[0], len(live))
            for r, b in enumerate(live):
                mine = ref[b][0]["rows"][ref[b][1]]
                if t < len(mine):                            # the board still waits for the network at this step of ITS search
                    assert torch.equal(got[r * L:(r + 1) * L], mine[t]), "call %d: row %d is not board %d's network input" % (t, r, b)
            total += got.shape[0]
            t += 1
    assert total == sum(c.shape[0] for c in rec.calls[:t])
    return t, total


# ------------------------------------------------------------------------------------------------ 4. exactness, L = 1
@pytest.mark.parametrize("kind", ["dyadic", "rational", "fast16", "split"])
def test_mixed_batch_equals_uniform_engines(positions, kind):
    dtype = _dtype_for(kind)
    B = len(positions)
    budgets = _budgets([0, 1, 2, 5, 16, 64], B, keep_last=16)           # the terminal root gets a budget that is neither 0 nor the capacity
    ref = references(positions, budgets, kind, dtype)
    eng = mixed_engine(positions, kind, dtype)
    eng.set_budgets(budgets)
    rec = Recorder(kind, dtype)
    eng.search(rec)
    st = eng.check_errors()
    roots = _roots(eng)
    for b in range(B):
        run, i = ref[b]
        assert _tree(eng, b) == run["trees"][i], "board %d (budget %d): tree" % (b, budgets[b])
        assert roots[b] == run["roots"][i], "board %d (budget %d): root children" % (b, budgets[b])
        visits = np.frombuffer(run["trees"][i][2], np.int32)
        assert int(visits[0]) == 1 + budgets[b]
    runs = {id(r): r for r, _ in ref.values()}.values()
    for k in COUNTERS:
        assert st[k] == sum(r["stats"][k] for r in runs), k
    assert st["max_edges_used"] == max(r["stats"]["max_edges_used"] for r in runs)
    assert st["simulations"] == sum(budgets) and st["boards_pending"] == 0
    # test 5 on this run: rows shrink and move; last_rows is what the evaluator saw
    n_calls, total = check_rows(eng, rec, budgets, ref)
    assert n_calls == len(rec.calls) == eng.last_steps == CAP and eng.last_rows == total
    assert rec.calls[0].shape[0] <= sum(1 for b in range(B - 1) if budgets[b] > 0)        # budget 0 and the terminal root never take a row
    assert 0 < rec.calls[-1].shape[0] <= sum(1 for b in range(B - 2) if budgets[b] == 64) < rec.calls[0].shape[0]
    eng.close()

    # second run: budgets that can be played (1 makes sz_play flag SZ_ERR_ZERO_VISITS, a terminal root has nothing to play), then one ply
    live = positions[:-1]
    budgets = _budgets([2, 5, 16, 64], len(live))
    u = 0.37
    ref = references(live, budgets, kind, dtype, play_u=u)
    eng = mixed_engine(live, kind, dtype)
    eng.set_budgets(budgets)
    eng.search(Recorder(kind, dtype))
    eng.check_errors()
    trees = [_tree(eng, b) for b in range(len(live))]
    eng.play([u] * len(live))
    eng.check_errors()
    ply = _ply_records(eng, range(len(live)))
    for b in range(len(live)):
        run, i = ref[b]
        assert trees[b] == run["trees"][i] and ply[b] == run["ply"][i], "board %d (budget %d)" % (b, budgets[b])
    eng.close()


def test_budget_one_is_num_searches_one(positions):
    """sz_play after a search with budget 1 flags SZ_ERR_ZERO_VISITS on that board, as num_searches = 1 does (mcts.py:118-120)"""
    for budgets in ([1, 16], None):
        eng = SelfPlayEngine(HashModel(), {"C": 2, "num_searches": CAP if budgets else 1}, 2, chess960=True, learning=True)
        for b in range(2):
            eng.upload_game(b, positions[b])
        if budgets:
            eng.set_budgets(budgets)
        eng.search()
        eng.check_errors()
        eng.play([0.5, 0.5])
        st = eng.stats()
        assert st["boards_error"] == (1 if budgets else 2) and st["first_error"] == N.SZ_ERR_ZERO_VISITS
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. rows shrink and move, every layout
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, "nhwc128", "bits128"], ids=["f32", "bf16", "nhwc128", "bits128"])
@pytest.mark.parametrize("mapping", ["identity", "compacted"])
def test_rows_shrink_and_move(positions, dtype, mapping):
    B = len(positions)
    # every second board drops out at each shrink: a live board's new row is another live board's old row
    budgets = [(64, 2, 16, 5)[b % 4] for b in range(B)]
    inactive = (1, 4, 5, 12, 23) if mapping == "compacted" else ()
    ref = references(positions, budgets, "dyadic", dtype, skip=inactive)
    eng = mixed_engine(positions, "dyadic", dtype, inactive=inactive)
    eng.set_budgets(budgets)
    rec = Recorder("dyadic", dtype)
    eng.search(rec)
    eng.check_errors()
    n_calls, total = check_rows(eng, rec, [0 if b in inactive else budgets[b] for b in range(B)], ref)
    assert n_calls == len(rec.calls) == eng.last_steps == CAP and eng.last_rows == total
    assert rec.calls[1].shape[0] == rec.calls[0].shape[0] <= len(ref) and rec.calls[2].shape[0] < rec.calls[0].shape[0]
    for b in range(B):
        if b in inactive:
            assert len(eng.debug_tree(b)[0]) == 0
        else:
            assert _tree(eng, b) == ref[b][0]["trees"][ref[b][1]], "board %d" % b
    # the mapping of the caller comes back for the next search: same rows, same trees
    eng.set_budgets(None)
    rec2 = Recorder("dyadic", dtype)
    eng.search(rec2)
    eng.check_errors()
    assert [c.shape[0] for c in rec2.calls] == [B - len(inactive)] * CAP and eng.last_rows == CAP * (B - len(inactive))
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. exactness with leaf batching
@pytest.mark.parametrize("L", [2, 7])
@pytest.mark.parametrize("lam", [1.0, 0.5])
def test_budgets_with_leaf_batching_match_restatement(positions, L, lam):
    items = positions[:6] + positions[10:13] + positions[-2:]
    B = len(items)
    budgets = [(3, 7, 32, 64)[(b * 3 + b // 4) % 4] for b in range(B)]
    assert set(budgets) == {3, 7, 32, 64}
    refs = [vlref.search(ct, s, learning=True, L=L, lam=lam, mode="dyadic", salt=5) for ct, s in zip(items, budgets)]
    args = {"C": 2, "num_searches": CAP, "leaves_per_step": L, "virtual_loss": lam}
    eng = SelfPlayEngine(None, args, B, chess960=True, learning=True)
    for b, ct in enumerate(items):
        eng.upload_game(b, ct)
    eng.set_budgets(budgets)
    # by hand, identity rows: every step's pending boards (= each board's own step count) and network input rows against the restatement
    eng.begin()
    t = 0
    while True:
        torch.cuda.synchronize()
        pend = (eng.debug_pending()[4] & 2) != 0
        assert pend.tolist() == [t < len(r.steps) for r in refs], "step %d: boards waiting for the network" % t
        if not pend.any():
            break
        planes = pack_planes(eng.planes.float().cpu().numpy())
        pol, val = np.zeros((B * L, N.SZ_ACTIONS), np.float32), np.zeros(B * L, np.float32)
        for b in np.nonzero(pend)[0]:
            want = refs[b].steps[t]
            assert np.array_equal(planes[b * L:b * L + len(want)], want), "step %d board %d: network input rows differ" % (t, b)
            for i in range(len(want)):
                pol[b * L + i], val[b * L + i] = evaluate_packed(want[i], "dyadic", 5)
        eng.step(torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda())
        t += 1

    def check_trees():
        st = eng.check_errors()
        assert st["boards_pending"] == 0
        for b, r in enumerate(refs):
            d, a, v, w, p = eng.debug_tree(b)
            rd, ra, rv, rw, rp = r.tree()
            assert np.array_equal(d, rd) and np.array_equal(a, ra) and np.array_equal(v, rv), "board %d" % b
            assert w.tobytes() == rw.tobytes() and p.tobytes() == rp.tobytes(), "board %d" % b
            assert int(v[0]) == 1 + budgets[b]
        return st

    s0 = check_trees()
    assert s0["simulations"] == sum(budgets)
    # and through search(): segments, shrinking rows (L rows per board move), the data-dependent tail
    rec = Recorder("dyadic", torch.float32)
    rec.net = HashModel(mode="dyadic", salt=5)
    eng.search(rec)
    s1 = check_trees()
    assert s1["simulations"] - s0["simulations"] == sum(budgets)
    segs = search_segments(budgets, L, eng.max_shrinks)
    assert eng.last_steps == len(rec.calls) == max(max(len(r.steps) for r in refs), sum(segs))
    assert eng.last_rows == sum(c.shape[0] for c in rec.calls)
    t, live = 0, []
    for i, n in enumerate(segs + [len(rec.calls) - sum(segs)]):
        if i < len(segs):
            live = [b for b in range(B) if len(refs[b].steps) > t]              # boards still searching when the segment began; the tail shrinks no more
        for _ in range(n):
            assert rec.calls[t].shape[0] == len(live) * L
            got = pack_planes(rec.calls[t].cpu().numpy())
            for r, b in enumerate(live):
                if t < len(refs[b].steps):
                    want = refs[b].steps[t]
                    assert np.array_equal(got[r * L:r * L + len(want)], want), "call %d: rows of board %d" % (t, b)
            t += 1
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. unset is the engine without the option
def test_unset_budgets_change_nothing(positions):
    B = len(positions)
    trees = {}
    for name in ("never", "none_after_budgeted", "all_capacity"):
        eng = mixed_engine(positions, "dyadic", torch.float32)
        rec = Recorder("dyadic", torch.float32)
        if name == "none_after_budgeted":
            eng.set_budgets(_budgets([0, 2, 5, 16, 64], B))
            eng.search(rec)
            eng.check_errors()
            for b, ct in enumerate(positions):
                eng.upload_game(b, ct)
            eng.set_budgets(None)
            rec = Recorder("dyadic", torch.float32)
        elif name == "all_capacity":
            eng.set_budgets([CAP] * B)
        eng.search(rec)
        st = eng.check_errors()
        assert eng.last_steps == CAP and st["boards_pending"] == 0
        if name != "all_capacity":
            assert [c.shape[0] for c in rec.calls] == [B] * CAP and eng.last_rows == B * CAP
        else:
            assert [c.shape[0] for c in rec.calls] == [B - 1] * CAP              # only the terminal root never takes a row
        trees[name] = [_tree(eng, b) for b in range(B)]
        eng.close()
    assert trees["never"] == trees["none_after_budgeted"] == trees["all_capacity"]
    run = uniform_run(positions, "all", CAP, "dyadic", torch.float32)
    assert trees["never"] == run["trees"]


# ------------------------------------------------------------------------------------------------ 8. self-play with a playout cap
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


def _same_games(a, b):
    assert set(a) == set(b)
    assert a["result"] == b["result"] and a["rewards"] == b["rewards"] and a["colours"] == b["colours"]
    assert a["sample_plies"] == b["sample_plies"] and a["chosen_actions"] == b["chosen_actions"]
    assert [list(x.items()) for x in a["actions"]] == [list(x.items()) for x in b["actions"]]
    assert len(a["states"]) == len(b["states"]) and all(torch.equal(x, y) for x, y in zip(a["states"], b["states"]))
    assert len(a["packed_states"]) == len(b["packed_states"]) and all(np.array_equal(x, y) for x, y in zip(a["packed_states"], b["packed_states"]))


def test_play_games_with_playout_cap(monkeypatch):
    from sigma_zero_amd import sim
    net = _IntHashNet()
    S, fast, G, plies = 16, 4, 6, 8
    sch = [518, 0, 959, 333, 702, 100]
    u = lambda g, ply: ((g * 7919 + ply * 104729) % 997) / 997.0
    args = {"C": 2, "num_searches": S}
    capped = dict(args, playout_cap={"fast": fast, "p_full": 0.25})
    kw = dict(c960=True, scharnagl=sch, uniforms=u, max_plies=plies)
    off = sim.play_games(net, args, G, **kw)
    st_full = {}
    all_full = sim.play_games(net, capped, G, full_search=lambda g, p: True, stats=st_full, **kw)
    for g in range(G):
        _same_games(off[g], all_full[g])
        assert off[g]["sample_plies"] == list(range(len(off[g]["actions"])))
    assert st_full["fast_plies"] == 0 and st_full["full_plies"] == sum(len(g["chosen_actions"]) for g in all_full)

    choose = lambda g, p: (g + p) % 3 == 0
    st = {}
    games = sim.play_games(net, capped, G, full_search=choose, stats=st, **kw)
    third_not_only = False
    for g, rec in enumerate(games):
        n = len(rec["chosen_actions"])
        assert n == plies or rec["result"] is not None                         # every ply is played, sampled or not
        assert rec["sample_plies"] == [p for p in range(n) if choose(g, p)]
        assert len(rec["states"]) == len(rec["actions"]) == len(rec["colours"]) == len(rec["packed_states"]) == len(rec["rewards"]) == len(rec["sample_plies"])
        ct = sz.ChessTensor(chess960=True, scharnagl=sch[g])                    # host mirror, replayed along the moves the game chose
        i = 0
        for p in range(n):
            if i < len(rec["sample_plies"]) and rec["sample_plies"][i] == p:
                assert np.array_equal(pack_planes(ct.get_representation().numpy()), rec["packed_states"][i]), "game %d ply %d" % (g, p)
                assert np.array_equal(rec["states"][i].numpy().astype(np.uint8), ct.get_representation().numpy().astype(np.uint8))
                assert rec["colours"][i] == (p % 2 == 0)
                vals = np.array(list(rec["actions"][i].values()), np.float64)
                assert abs(vals.sum() - 1.0) < 1e-12
                k = vals * (S - 1)                                              # a full search: S - 1 visits below the root
                assert np.abs(k - np.round(k)).max() < 1e-9 and int(np.round(k).sum()) == S - 1
                k3 = vals * (fast - 1)
                third_not_only |= bool(np.abs(k3 - np.round(k3)).max() > 1e-6)
                assert len(vals) == len(ct.legal_action_indices())
                i += 1
            assert rec["chosen_actions"][p] in ct.legal_action_indices()
            ct.push_action(rec["chosen_actions"][p])
        assert i == len(rec["sample_plies"])
    assert third_not_only, "no sample has a visit fraction that fast - 1 = 3 visits could not produce: were fast plies recorded?"
    total = sum(len(g["chosen_actions"]) for g in games)
    assert st["plies"] == max(len(g["chosen_actions"]) for g in games) == plies
    assert st["full_plies"] + st["fast_plies"] == total and st["full_plies"] == sum(len(g["sample_plies"]) for g in games)
    assert st["sims"] == S * st["full_plies"] + fast * st["fast_plies"]
    assert st["nn_rows"] < S * total and st["nn_rows"] >= S * st["full_plies"] + fast * st["fast_plies"]
    # the moves of a game do not depend on which plies were sampled only if the budgets are equal; here they differ, so only compact on / off is compared
    again = sim.play_games(net, capped, G, full_search=choose, compact=False, **kw)
    for g in range(G):
        _same_games(games[g], again[g])

    # rewards follow the ply a sample was taken at: every game is declared won by White after its 5th ply (a stubbed result)
    class Decided(SelfPlayEngine):
        n_fetch = 0

        def fetch_ply(self):
            rec = super().fetch_ply()
            self.n_fetch += 1
            if self.n_fetch == 5:
                rec["game_over"][:] = 1
                rec["result"][:] = 1
            return rec

    monkeypatch.setattr(sim, "SelfPlayEngine", Decided)
    decided = sim.play_games(net, capped, G, full_search=choose, **kw)
    monkeypatch.undo()
    for g, rec in enumerate(decided):
        assert rec["result"] == "1-0" and len(rec["chosen_actions"]) == 5           # also when the last ply was a fast one
        assert rec["sample_plies"] == [p for p in range(5) if choose(g, p)]
        assert rec["rewards"] == [(-1) ** p for p in rec["sample_plies"]]
    assert decided[2]["rewards"] == [-1, 1]                                         # plies 1 and 4: the parity of the sample INDEX would give [1, -1]

    # the default full / fast draw leaves the global RNGs alone
    np.random.seed(123)
    random.seed(123)
    s_np, s_py = np.random.get_state(), random.getstate()
    st = {}
    sim.play_games(net, capped, G, stats=st, **kw)
    t_np = np.random.get_state()
    assert s_np[0] == t_np[0] and np.array_equal(s_np[1], t_np[1]) and s_np[2:] == t_np[2:] and random.getstate() == s_py
    assert st["full_plies"] + st["fast_plies"] == G * plies or any(g["result"] for g in games)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(positions):
    import ctypes as C
    lib = N.lib()
    B = 4
    pos = positions[:B]
    want = uniform_run(pos, "refusals", CAP, "dyadic", torch.float32)["trees"]
    eng = SelfPlayEngine(HashModel(mode="dyadic", salt=11), {"C": 2, "num_searches": CAP}, B, chess960=True, learning=True)
    arr = lambda xs: np.asarray(xs, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    n = C.c_int32(-7)

    def usable():
        for b, ct in enumerate(pos):
            eng.upload_game(b, ct)
        eng.search()
        eng.check_errors()
        assert [_tree(eng, b) for b in range(B)] == want

    for bad in ([-1, 4, 4, 4], [4, 4, 4, CAP + 1]):
        assert lib.sz_set_search_budgets(eng._e, arr(bad), eng._stream()) == N.SZ_ERR_INVALID
        with pytest.raises(N.NativeError):
            eng.set_budgets(bad)
        assert eng.budgets is None
        usable()
    with pytest.raises(ValueError):
        eng.set_budgets([4] * (B + 1))
    for b, ct in enumerate(pos):
        eng.upload_game(b, ct)
    assert lib.sz_compact_searching(eng._e, eng.planes.data_ptr(), C.byref(n), eng._stream()) == N.SZ_ERR_STATE      # before begin
    with pytest.raises(N.NativeError):
        eng.compact_searching()
    eng.begin()
    for t in range(CAP):
        assert lib.sz_set_search_budgets(eng._e, arr([4] * B), eng._stream()) == N.SZ_ERR_STATE                        # between begin and the last step
        if t in (0, 17, CAP - 1):
            assert eng.compact_searching() == B                                                                         # valid here; drops nothing
        eng.step(*eng.evaluate(eng.planes))
    eng.check_errors()
    assert lib.sz_compact_searching(eng._e, eng.planes.data_ptr(), C.byref(n), eng._stream()) == N.SZ_ERR_STATE      # the search has ended
    assert n.value == -7
    assert [_tree(eng, b) for b in range(B)] == want
    assert lib.sz_set_search_budgets(eng._e, arr([4] * B), eng._stream()) == N.SZ_OK
    assert lib.sz_set_search_budgets(eng._e, None, eng._stream()) == N.SZ_OK
    usable()
    eng.close()
    reuse = SelfPlayEngine(HashModel(), {"C": 2, "num_searches": 8, "reuse_subtree": True}, 2, learning=False)
    assert lib.sz_set_search_budgets(reuse._e, arr([4, 4]), reuse._stream()) == N.SZ_ERR_INVALID
    assert lib.sz_set_search_budgets(reuse._e, None, reuse._stream()) == N.SZ_OK
    reuse.new_games([-1, -1])
    reuse.search()
    assert reuse.check_errors()["simulations"] == 16
    reuse.close()
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 8, "max_shrinks": -1}, 2)
