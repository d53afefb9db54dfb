"""Leaf batching with virtual loss (args["leaves_per_step"], sz_set_leaf_batching): what it buys and what it costs, on the GPU.

  1. wall time of one 800-search MCTS0.search of a single position, per L, for the f16, bf16 and split MFMA networks;
  2. time per step of the tree kernel alone (sz_search_step with a fixed policy, device events), per L: the serial gathering cost;
  3. self-play search throughput (simulations/s) with 64, 128 and 210 live boards, L = 1 against L = 4, 8, 16 (f16 network);
  4. how far the root visit distribution moves from L = 1 (argmax agreement, total-variation distance) on 64 positions, fp32 network.

    python tools/leaf_batch_bench.py --out profiles/leaf_batching.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sigma_zero_amd as sz                                      # noqa: E402
from sigma_zero_amd.fastnet import FastPolicyNet, SplitPolicyNet   # noqa: E402
from sigma_zero_amd.selfplay import SelfPlayEngine               # noqa: E402


def positions(n, seed=0, plies=(4, 30)):
    """n positions reached by random legal play from the start (host rules), none terminal"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        ct = sz.ChessTensor()
        for _ in range(int(rng.integers(*plies))):
            moves = ct.get_moves()
            if not moves:
                break
            ct.move_piece(moves[int(rng.integers(len(moves)))])
        if not ct.get_value_and_terminated()[1]:
            out.append(ct)
    return out


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def single_position(nets, Ls, S, reps, pos):
    res = {}
    for name, net in nets.items():
        for L in Ls:
            m = sz.MCTS0(game=pos, args={"C": 2, "num_searches": S, "leaves_per_step": L}, model=net)
            m.search(pos.board, verbose=False)                   # warm-up: engine, buffers, code objects
            ts = [sync_time(lambda: m.search(pos.board, verbose=False)) for _ in range(reps)]
            eng = m._tree_engine
            res["%s L=%d" % (name, L)] = dict(ms_median=1e3 * float(np.median(ts)), ms_min=1e3 * min(ts), network_calls=eng.last_steps)
            print("single position %-6s L=%-3d %8.1f ms  (%d network calls)" % (name, L, 1e3 * float(np.median(ts)), eng.last_steps), flush=True)
    return res


def tree_step_time(Ls, S, boards):
    """device time of sz_search_step alone per step (fixed uniform policy, value 0)"""
    res = {}
    for B in boards:
        for L in Ls:
            eng = SelfPlayEngine(None, {"C": 2, "num_searches": S, "leaves_per_step": L}, B, learning=False)
            eng.new_games([-1] * B)
            pol = torch.full((B * L, sz._native.SZ_ACTIONS), 1.0 / 4672, device="cuda")
            val = torch.zeros(B * L, device="cuda")
            for rep in range(2):                                # the second search is timed
                eng.begin()
                evs = []
                for _ in range(S):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); eng.step(pol, val); e1.record()
                    evs.append((e0, e1))
                    if eng.pending_boards() == 0:
                        break
            torch.cuda.synchronize()
            ms = [a.elapsed_time(b) for a, b in evs]
            res["B=%d L=%d" % (B, L)] = dict(steps=len(ms), us_per_step_median=1e3 * float(np.median(ms)), us_total=1e3 * float(sum(ms)),
                                              us_per_leaf=1e3 * float(sum(ms)) / (B * S))
            print("tree kernel B=%-4d L=%-3d %4d steps  %8.1f us/step  %8.1f us total  %6.2f us/simulation" %
                  (B, L, len(ms), 1e3 * float(np.median(ms)), 1e3 * sum(ms), 1e3 * sum(ms) / (B * S)), flush=True)
            eng.close()
    return res


def selfplay_throughput(net, Ls, S, boards):
    res = {}
    for B in boards:
        for L in Ls:
            eng = SelfPlayEngine(net, {"C": 2, "num_searches": S, "leaves_per_step": L}, B, learning=True, planes_dtype="bits128")
            eng.new_games([-1] * B)
            eng.search(); eng.check_errors()                    # warm-up
            eng.new_games([-1] * B)
            t = sync_time(eng.search)
            eng.check_errors()
            res["B=%d L=%d" % (B, L)] = dict(seconds=t, sims_per_s=B * S / t, network_calls=eng.last_steps)
            print("self-play B=%-4d L=%-3d %7.3f s  %9.0f simulations/s  (%d network calls)" % (B, L, t, B * S / t, eng.last_steps), flush=True)
            eng.close()
    return res


def drift(net, Ls, S, pos):
    B = len(pos)
    dist = {}
    for L in Ls:
        eng = SelfPlayEngine(net, {"C": 2, "num_searches": S, "leaves_per_step": L}, B, learning=False)
        for b, ct in enumerate(pos):
            eng.upload_game(b, ct)
        eng.search(); eng.check_errors()
        action, visits, n_child, _, _ = eng.root_children()
        dist[L] = [(action[b, :n_child[b]].copy(), visits[b, :n_child[b]].astype(np.float64) / visits[b, :n_child[b]].sum()) for b in range(B)]
        eng.close()
    res = {}
    for L in Ls:
        if L == 1:
            continue
        agree, tv = [], []
        for (a1, p1), (aL, pL) in zip(dist[1], dist[L]):
            assert np.array_equal(a1, aL)
            agree.append(int(np.argmax(p1) == np.argmax(pL)))
            tv.append(0.5 * float(np.abs(p1 - pL).sum()))
        res["L=%d" % L] = dict(argmax_agreement=float(np.mean(agree)), tv_mean=float(np.mean(tv)), tv_max=float(np.max(tv)))
        print("drift vs L=1, L=%-3d argmax agreement %.3f  TV mean %.4f max %.4f" % (L, np.mean(agree), np.mean(tv), np.max(tv)), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--searches", type=int, default=800)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parts", default="single,tree,selfplay,drift")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.manual_seed(0)
    ref = sz.policyNN({}).cuda().eval()                          # random-init weights: no trained weights exist here
    parts = a.parts.split(",")
    out = dict(device=torch.cuda.get_device_name(0), searches=a.searches)
    if "single" in parts:
        nets = {"f16": FastPolicyNet(ref, operands="fp16"), "bf16": FastPolicyNet(ref), "split": SplitPolicyNet(ref)}
        out["single_position_ms"] = single_position(nets, [1, 4, 16, 32, 64, 128], a.searches, a.reps, positions(1, seed=3)[0])
    if "tree" in parts:
        out["tree_step"] = tree_step_time([1, 4, 16, 32, 64, 128], a.searches, [1, 128])
    if "selfplay" in parts:
        out["selfplay"] = selfplay_throughput(FastPolicyNet(ref, operands="fp16"), [1, 4, 8, 16], a.searches, [64, 128, 210])
    if "drift" in parts:
        out["drift_fp32"] = drift(ref, [1, 4, 16, 32], a.searches, positions(64, seed=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
