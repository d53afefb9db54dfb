"""Per-board search budgets with in-search batch shrinking (args["playout_cap"], sz_set_search_budgets / sz_compact_searching):
what one self-play ply costs, on the GPU.  f16 MFMA network, random-init weights, start positions, one process per configuration
(a fresh child under its own time limit; the first child that fails ends the run):

  a  every board num_searches, budgets unset: the engine without the option
  b  budgets set to num_searches everywhere: the option's overhead (the budget upload, one compaction that drops nothing)
  c  fast / full budgets at p_full with max_shrinks = 0: unequal budgets on a batch that never shrinks
  d  the same with shrinking: the network runs on the full-search boards only once the fast ones are done

Reported per configuration: seconds per ply (median of the timed plies), network calls and rows, simulations/s and training samples/s
(a ply's samples are its full-search boards; in a and b every board).

    python tools/playout_cap_bench.py --out profiles/playout_cap.json        # also writes profiles/playout_cap.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("a", "b", "c", "d")


def child(cfg, boards, full, fast, p_full, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import sigma_zero_amd as sz
    from sigma_zero_amd.fastnet import FastPolicyNet
    from sigma_zero_amd.selfplay import SelfPlayEngine
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.manual_seed(0)
    net = FastPolicyNet(sz.policyNN({}).cuda().eval(), operands="fp16")
    args = {"C": 2, "num_searches": full, "max_shrinks": 0 if cfg == "c" else 4}
    eng = SelfPlayEngine(net, args, boards, learning=True, planes_dtype="bits128")
    rng = np.random.default_rng(0)
    is_full = rng.random(boards) < p_full
    budgets = None if cfg == "a" else np.full(boards, full) if cfg == "b" else np.where(is_full, full, fast)
    samples = boards if cfg in "ab" else int(is_full.sum())
    sims = boards * full if budgets is None else int(budgets.sum())

    def ply():
        eng.new_games([-1] * boards)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if budgets is not None:
            eng.set_budgets(budgets)
        eng.search()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    ply()                                                    # warm-up: code objects, buffers, the staging buffer of the row move
    ts = [ply() for _ in range(reps)]
    st = eng.check_errors()
    assert st["boards_pending"] == 0
    t = float(np.median(ts))
    out = dict(config=cfg, boards=boards, full=full, fast=fast, p_full=p_full, seconds_per_ply=t, seconds_all=ts, network_calls=eng.last_steps,
               network_rows=eng.last_rows, simulations=sims, simulations_per_s=sims / t, samples=samples, samples_per_s=samples / t,
               device=torch.cuda.get_device_name(0))
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="4096:800:100,512:100:25", help="boards:full:fast, comma separated")
    ap.add_argument("--p-full", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        cfg, boards, full, fast = a.child.split(":")
        return child(cfg, int(boards), int(full), int(fast), a.p_full, a.reps)
    results, lines = [], []
    for shape in a.shapes.split(","):
        for cfg in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "%s:%s" % (cfg, shape), "--p-full", str(a.p_full), "--reps", str(a.reps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)      # the parent never opens the GPU
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                print(p.stdout[-4000:])
                raise SystemExit("configuration %s %s failed (exit status %d): stopping here" % (cfg, shape, p.returncode))
            r = json.loads(res[-1][len("RESULT "):])
            results.append(r)
            lines.append("%-2s %5d boards  %4d / %-4d p_full %.2f  %7.3f s/ply  %4d network calls  %9d rows  %10.0f simulations/s  %8.1f samples/s"
                         % (cfg, r["boards"], r["fast"] if cfg in "cd" else r["full"], r["full"], r["p_full"] if cfg in "cd" else 1.0, r["seconds_per_ply"],
                            r["network_calls"], r["network_rows"], r["simulations_per_s"], r["samples_per_s"]))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=results[0]["device"], results=results), f, indent=1)
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
            f.write("tools/playout_cap_bench.py on %s: one self-play ply, f16 network, random-init weights, start positions\n" % results[0]["device"])
            f.write("a = budgets unset, b = budgets = full everywhere, c = fast / full without shrinking, d = with shrinking\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
