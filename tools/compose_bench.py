"""What leaf batching, the solver and subtree reuse cost and save together (sz_set_search_options / args["combine_options"]); results are
kept in profiles/compose.{json,txt}.  One process per configuration, like tools/leaf_batch_bench.py.

  python tools/compose_bench.py                 every configuration in a child process of its own, results to profiles/compose.json
  python tools/compose_bench.py search L solver reuse     one 800-search MCTS0.search of the standard start, f16 network: median ms of 5
  python tools/compose_bench.py game all|batching         one greedy arena-style game of 40 plies at S = 800, L = 32: seconds

Nothing is gated on these numbers; the effect of any combination on playing strength is unmeasured."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _net():
    import torch
    import sigma_zero_amd as sz
    from sigma_zero_amd.fastnet import FastPolicyNet
    torch.manual_seed(0)
    return FastPolicyNet(sz.policyNN({}).cuda().eval(), operands="fp16")


def _args(L, solver, reuse, S=800):
    args = {"C": 2, "num_searches": S, "combine_options": True}
    if L > 1:
        args.update(leaves_per_step=L, virtual_loss=1.0)
    if solver:
        args["solver"] = True
    if reuse:
        args["reuse_subtree"] = True
    return args


def search(L, solver, reuse, repeats=5):
    import torch
    import sigma_zero_amd as sz
    ct = sz.ChessTensor()
    m = sz.MCTS0(game=ct, args=_args(L, solver, reuse), model=_net())
    times = []
    for _ in range(repeats + 1):                                     # the first search warms up
        torch.cuda.synchronize()
        t = time.perf_counter()
        m.search(ct.board, verbose=False, learning=False)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    times = sorted(times[1:])
    return dict(kind="search", L=L, solver=solver, reuse=reuse, ms_median=times[len(times) // 2], ms_min=times[0], ms_max=times[-1])


def game(which, plies=40, L=32):
    import numpy as np
    import torch
    from sigma_zero_amd.selfplay import SelfPlayEngine
    all3 = which == "all"
    eng = SelfPlayEngine(_net(), _args(L, all3, all3), 1, learning=False, planes_dtype="bits128")
    eng.new_games([-1])
    torch.cuda.synchronize()
    t, n, steps = time.perf_counter(), 0, 0
    for _ in range(plies):
        eng.search()
        eng.check_errors()
        steps += eng.last_steps
        eng.play(np.full(1, -1.0))
        n += 1
        if eng.fetch_ply()["game_over"][0]:
            break
    torch.cuda.synchronize()
    out = dict(kind="game", options="batching+solver+reuse" if all3 else "batching", L=L, plies=n, seconds=time.perf_counter() - t, network_calls=steps)
    eng.close()
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "search":
        print(json.dumps(search(int(sys.argv[2]), bool(int(sys.argv[3])), bool(int(sys.argv[4])))))
    elif len(sys.argv) > 1 and sys.argv[1] == "game":
        print(json.dumps(game(sys.argv[2])))
    else:
        jobs = [["search", str(L), str(s), str(r)] for L in (1, 32) for s in (0, 1) for r in (0, 1)] + [["game", "batching"], ["game", "all"]]
        results = []
        for job in jobs:
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + job, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit("configuration %s failed (%d): %s" % (job, p.returncode, p.stderr[-400:]))
            results.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(results[-1], flush=True)
        with open(os.path.join(ROOT, "profiles", "compose.json"), "w") as f:
            json.dump(results, f, indent=1)
