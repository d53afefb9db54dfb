"""The Gumbel root search (args["gumbel"], sz_set_gumbel): what the option costs per search step, on the GPU.  4096 boards from the start
position, bf16 MFMA network with random-init weights, one search of 64 and one of 800 simulations per run.  Legs: the option off and on
(seeded Gumbel draws), `tree` = on with the completed-Q selection below the root as well (args["gumbel_tree"], sz_set_gumbel_tree), and, with
--parent-tree DIR (a checkout of the parent commit with its library built), the default path of that
checkout, so that "no default kernel changed" is also a measurement.  The legs run alternately (off, on, tree[, parent], off, on, ...), one fresh
process per run under its own time limit, all in one session on one GPU; the first run that fails ends the tool.  Reported per run:

  ms per step       wall time of the search (begin + num_searches network calls and tree steps, synchronised) / num_searches
  mean leaf depth   sz_stats sum_depth / simulations

and per leg the spread of its repeats.  Nothing is gated.  With random-init weights this says nothing about playing strength.

    python tools/gumbel_bench.py --out profiles/gumbel_bench.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(leg, root, boards, searches, m):
    import numpy as np
    import torch
    sys.path.insert(0, root)
    import sigma_zero_amd as sz
    from sigma_zero_amd.fastnet import FastPolicyNet
    from sigma_zero_amd.selfplay import SelfPlayEngine
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.manual_seed(0)
    net = FastPolicyNet(sz.policyNN({}).cuda().eval(), operands="bf16")
    args = {"C": 2, "num_searches": searches}
    if leg in ("on", "tree"):
        args["gumbel"] = {"m": m}
    if leg == "tree":
        args["gumbel_tree"] = True
    eng = SelfPlayEngine(net, args, boards, learning=True, planes_dtype="bits128")
    rng = np.random.default_rng(0)
    out = []
    for rep in range(3):                                     # the first search is the warm-up (code objects, buffers) and is not reported
        eng.new_games([-1] * boards)
        if leg in ("on", "tree"):
            eng.set_gumbel(eng.gumbel, -np.log(-np.log(rng.random((boards, 218)))))
        st0 = eng.stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.search()
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        st = eng.check_errors()
        assert st["boards_pending"] == 0 and st["boards_done"] == boards
        sims = int(st["simulations"] - st0["simulations"])
        if rep:
            out.append(dict(seconds=seconds, ms_per_step=1e3 * seconds / searches, simulations=sims,
                            mean_leaf_depth=float(st["sum_depth"] - st0["sum_depth"]) / max(sims, 1)))
    fallbacks = eng.gumbel_stats()[1] if leg in ("on", "tree") else 0
    tree_selections = eng.gumbel_tree_stats() if leg == "tree" else 0      # over the three searches of the process
    eng.close()
    print("RESULT " + json.dumps(dict(leg=leg, boards=boards, searches=searches, m=m, runs=out, fallbacks=fallbacks, tree_selections=tree_selections,
                                      device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--searches", default="64,800", help="simulations per search, one set of legs for each")
    ap.add_argument("--m", type=int, default=16, help="args['gumbel']['m'] of the `on` legs")
    ap.add_argument("--rounds", type=int, default=2, help="rounds of the legs, run alternately")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: adds the `parent` leg")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.root, a.boards, int(a.searches), a.m)
    legs = ["off", "on", "tree"] + (["parent"] if a.parent_tree else [])
    lines, device = [], None
    for searches in [int(x) for x in a.searches.split(",")]:
        per_leg = {leg: [] for leg in legs}
        for rnd in range(a.rounds):
            for leg in legs:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--boards", str(a.boards), "--searches", str(searches), "--m", str(a.m),
                       "--root", os.path.abspath(a.parent_tree) if leg == "parent" else ROOT]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)      # the parent never opens the GPU
                res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not res:
                    print(p.stdout[-4000:])
                    raise SystemExit("leg %s of round %d failed (exit status %d): stopping here" % (leg, rnd, p.returncode))
                r = json.loads(res[-1][len("RESULT "):])
                device = r["device"]
                for k, run in enumerate(r["runs"]):
                    per_leg[leg].append(run["ms_per_step"])
                    lines.append("%4d simulations  round %d run %d  %-6s  %8.4f ms per step   %9d simulations in %7.3f s   mean leaf depth %6.3f%s"
                                 % (searches, rnd, k, leg, run["ms_per_step"], run["simulations"], run["seconds"], run["mean_leaf_depth"],
                                    "   fall-back selections %d" % r["fallbacks"] if leg in ("on", "tree") else ""))
                    print(lines[-1], flush=True)
        for leg in legs:
            v = per_leg[leg]
            lines.append("%4d simulations  %-6s  mean %8.4f ms per step over %d runs, min %8.4f, max %8.4f (spread %.2f %%)"
                         % (searches, leg, sum(v) / len(v), len(v), min(v), max(v), 100.0 * (max(v) - min(v)) / min(v)))
            print(lines[-1], flush=True)
    head = ("tools/gumbel_bench.py on %s: %d boards from the start position, bf16 network, random-init weights, learning engine; gumbel = {\"m\": %d}\n"
            "with seeded draws on the `on` and `tree` legs (`tree` = with gumbel_tree as well)%s; legs run alternately in one session, one process per run, the first search of a\n"
            "process not reported.  ms per step = wall time of a whole search / num_searches.  Nothing is gated; random-init weights say nothing about\n"
            "playing strength, which is unmeasured.\n"
            % (device, a.boards, a.m, "; `parent` = the default path of a checkout of the parent commit" if a.parent_tree else ""))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
