"""First-play urgency for unvisited children (args["fpu"], sz_set_fpu): what the option does to the shape of a self-play search and what it
costs, on the GPU.  A few hundred boards with Dirichlet root noise, the first plies of self-play from the start position, f16 MFMA network
with random-init weights, moves sampled from the recorded visit counts.  Two legs, the option off and on, with the same seeds for the Gamma
draws and the sampling uniforms, run alternately (off, on, off, on, ...), one fresh process per run under its own time limit; the first run
that fails ends the tool.  Reported per leg:

  simulations per second       new simulations / wall time of the searches (sz_play and the record fetch are outside the timed part)
  mean leaf depth              sz_stats sum_depth / simulations: how deep a simulation ends
  root children visited        mean over boards and plies of the number of root children with at least one counted visit, beside the mean
                               number of root children

Nothing is gated: these are first measurements.  With random-init weights they say nothing about a trained network's search; the effect of
the option on playing strength is unmeasured.

    python tools/fpu_bench.py --out profiles/fpu_bench.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(on, boards, searches, plies, fpu, alpha):
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
        args["fpu"] = fpu
    eng = SelfPlayEngine(net, args, boards, learning=True, planes_dtype="bits128")
    gam, uni = np.random.default_rng(0), np.random.default_rng(1)
    eng.new_games([-1] * boards)
    eng.search()                                             # warm-up on a throw-away search: code objects, buffers
    eng.check_errors()
    eng.new_games([-1] * boards)
    st0 = eng.stats()
    seconds, visited, children = 0.0, [], []
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
        _, vis, n_child, _, _ = eng.root_children()
        visited += (vis > 0).sum(axis=1).tolist()
        children += n_child.tolist()
        eng.play(u)
        eng.fetch_ply()
    sims = int(st["simulations"] - st0["simulations"])
    out = dict(on=bool(on), boards=boards, searches=searches, plies=plies, fpu=fpu if on else None, alpha=alpha, seconds=seconds, simulations=sims,
               mean_leaf_depth=float(st["sum_depth"] - st0["sum_depth"]) / max(sims, 1), root_children_visited=float(np.mean(visited)),
               root_children=float(np.mean(children)), device=torch.cuda.get_device_name(0))
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--boards", type=int, default=256)
    ap.add_argument("--searches", type=int, default=100, help="a fast ply of playout_cap: where the option matters most")
    ap.add_argument("--plies", type=int, default=4)
    ap.add_argument("--fpu", default='{"mode": "reduction", "value": 0.33, "root_mode": "absolute", "root_value": 1.0}', help="args['fpu'] of the `on` legs, as JSON")
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=2, help="off / on pairs, run alternately")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    fpu = json.loads(a.fpu)
    if a.child:
        return child(a.child == "on", a.boards, a.searches, a.plies, fpu, a.alpha)
    results, lines = [], []
    for rnd in range(a.rounds):
        for leg in ("off", "on"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--boards", str(a.boards), "--searches", str(a.searches), "--plies", str(a.plies),
                   "--fpu", a.fpu, "--alpha", str(a.alpha)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)      # the parent never opens the GPU
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                print(p.stdout[-4000:])
                raise SystemExit("leg %s of round %d failed (exit status %d): stopping here" % (leg, rnd, p.returncode))
            r = json.loads(res[-1][len("RESULT "):])
            results.append(r)
            lines.append("round %d  %-3s  %9d simulations in %7.3f s = %9.0f simulations/s   mean leaf depth %6.3f   root children visited %6.2f of %6.2f"
                         % (rnd, leg, r["simulations"], r["seconds"], r["simulations"] / r["seconds"], r["mean_leaf_depth"], r["root_children_visited"],
                            r["root_children"]))
            print(lines[-1], flush=True)
    head = ("tools/fpu_bench.py on %s: %d boards x %d searches x %d plies from the start position, Dirichlet(%g) root noise, f16 network,\n"
            "random-init weights, sampled moves; fpu = %s on the `on` legs; legs run alternately in one session, same seeds.\n"
            "Nothing is gated; random-init weights say nothing about a trained network's search; the effect on playing strength is unmeasured.\n"
            % (results[0]["device"], a.boards, a.searches, a.plies, a.alpha, json.dumps(fpu)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
