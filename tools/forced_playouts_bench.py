"""Forced playouts and policy-target pruning (args["forced_playouts"], sz_set_forced_playouts): what the option does to a self-play search
and what it costs, on the GPU.  A few hundred boards at 800 searches with Dirichlet root noise, the first plies of self-play from the start
position, f16 MFMA network with random-init weights, moves sampled from the recorded visit counts.  Two legs, the option off and on, with
the same seeds for the Gamma draws and the sampling uniforms, run alternately (off, on, off, on, ...), one fresh process per run under its
own time limit; the first run that fails ends the tool.  Reported per leg:

  simulations per second       new simulations / wall time of the searches (sz_play and the record fetch are outside the timed part)
  forced selections            sz_forced_stats out[0] as a share of the root selections ((num_searches - 1) per board and ply)
  pruned visits                sz_forced_stats out[1] as a share of the root's child visits (the same number)
  entropy of the target        mean over boards and plies of -sum p ln p, p = recorded visits / their sum

Nothing is gated: these are first measurements.  The effect of the option on playing strength is unmeasured.

    python tools/forced_playouts_bench.py --out profiles/forced_playouts_bench.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(on, boards, searches, plies, k, alpha):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import sigma_zero_amd as sz
    from sigma_zero_amd import _native as N
    from sigma_zero_amd.fastnet import FastPolicyNet
    from sigma_zero_amd.selfplay import SelfPlayEngine
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.manual_seed(0)
    net = FastPolicyNet(sz.policyNN({}).cuda().eval(), operands="fp16")
    args = {"C": 2, "num_searches": searches, "root_dirichlet_alpha": alpha}
    if on:
        args["forced_playouts"] = k
    eng = SelfPlayEngine(net, args, boards, learning=True, planes_dtype="bits128")
    gam, uni = np.random.default_rng(0), np.random.default_rng(1)
    eng.new_games([-1] * boards)
    eng.search()                                             # warm-up on a throw-away search: code objects, buffers
    eng.check_errors()
    eng.new_games([-1] * boards)
    st0, f0 = eng.stats(), eng.forced_stats()
    seconds, entropy, visits = 0.0, [], 0
    for ply in range(plies):
        eng.next_gamma = torch.from_numpy(gam.standard_gamma(alpha, size=(boards, N.SZ_MAX_MOVES)).astype(np.float32)).cuda()
        u = uni.random(boards)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.search()
        torch.cuda.synchronize()
        seconds += time.perf_counter() - t0
        st = eng.check_errors()
        assert st["boards_pending"] == 0
        visits += int(eng.root_children()[1].sum())          # the counted visits of the root's children, before sz_play
        eng.play(u)
        rec = eng.fetch_ply()
        v = rec["visits"][rec["active"].astype(bool)].astype(np.float64)
        p = v / v.sum(axis=1, keepdims=True)
        entropy += (-(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)).sum(axis=1)).tolist()
    f1 = eng.forced_stats()
    out = dict(on=bool(on), boards=boards, searches=searches, plies=plies, k=k, alpha=alpha, seconds=seconds,
               simulations=int(st["simulations"] - st0["simulations"]), root_selections=(searches - 1) * boards * plies, root_child_visits=visits,
               forced_selections=f1[0] - f0[0], pruned_visits=f1[1] - f0[1], mean_target_entropy=float(np.mean(entropy)), device=torch.cuda.get_device_name(0))
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--boards", type=int, default=256)
    ap.add_argument("--searches", type=int, default=800)
    ap.add_argument("--plies", type=int, default=2)
    ap.add_argument("--k", type=float, default=2.0)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=2, help="off / on pairs, run alternately")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child == "on", a.boards, a.searches, a.plies, a.k, a.alpha)
    results, lines = [], []
    for rnd in range(a.rounds):
        for leg in ("off", "on"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--boards", str(a.boards), "--searches", str(a.searches), "--plies", str(a.plies),
                   "--k", str(a.k), "--alpha", str(a.alpha)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)      # the parent never opens the GPU
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                print(p.stdout[-4000:])
                raise SystemExit("leg %s of round %d failed (exit status %d): stopping here" % (leg, rnd, p.returncode))
            r = json.loads(res[-1][len("RESULT "):])
            results.append(r)
            lines.append("round %d  %-3s  %9d simulations in %7.3f s = %9.0f simulations/s   forced selections %8d = %5.2f %% of %d root selections   "
                         "pruned visits %8d = %5.2f %% of %d root child visits   mean target entropy %.4f nat"
                         % (rnd, leg, r["simulations"], r["seconds"], r["simulations"] / r["seconds"], r["forced_selections"],
                            100.0 * r["forced_selections"] / r["root_selections"], r["root_selections"], r["pruned_visits"],
                            100.0 * r["pruned_visits"] / max(r["root_child_visits"], 1), r["root_child_visits"], r["mean_target_entropy"]))
            print(lines[-1], flush=True)
    head = ("tools/forced_playouts_bench.py on %s: %d boards x %d searches x %d plies from the start position, Dirichlet(%g) root noise, f16 network,\n"
            "random-init weights, sampled moves; forced_playouts = %g on the `on` legs; legs run alternately in one session, same seeds.\n"
            "Nothing is gated; the effect on playing strength is unmeasured.\n" % (results[0]["device"], a.boards, a.searches, a.plies, a.alpha, a.k))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
