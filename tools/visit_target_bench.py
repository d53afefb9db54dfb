"""Subtree reuse as a self-play configuration (args["visit_targets"], sz_set_visit_targets / sz_search_goals): network rows and seconds per
ply over the first plies of self-play from the start positions, on the GPU.  f16 MFMA network, random-init weights, moves sampled from the
visit counts, one process per configuration (a fresh child under its own time limit; the first child that fails ends the run):

  reuse    reuse_subtree alone (visit_targets off): every ply makes num_searches NEW simulations on top of what it kept
  cap      no reuse, playout_cap budgets fast / full at p_full (sz_set_search_budgets): the option visit targets are the counterpart of
  targets  reuse_subtree + visit_targets, the same fast / full draw as `cap` read as root visit targets: kept visits count

The draw of full / fast per board and ply and the sampling uniforms come from the same seeded generators in every configuration; the games
differ all the same once the trees do.  Reported per configuration and ply: seconds, network calls, network rows, new simulations, boards
that needed no new simulation; and the totals.  The saving is reported, not gated; its effect on playing strength is unmeasured.

    python tools/visit_target_bench.py --out profiles/visit_targets.json        # also writes profiles/visit_targets.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("reuse", "cap", "targets")


def child(cfg, boards, full, fast, p_full, plies):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import sigma_zero_amd as sz
    from sigma_zero_amd.fastnet import FastPolicyNet
    from sigma_zero_amd.selfplay import SelfPlayEngine
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.manual_seed(0)
    net = FastPolicyNet(sz.policyNN({}).cuda().eval(), operands="fp16")
    args = {"C": 2, "num_searches": full}
    if cfg != "cap":
        args["reuse_subtree"] = True
    if cfg == "targets":
        args["visit_targets"] = True
    eng = SelfPlayEngine(net, args, boards, learning=True, planes_dtype="bits128")
    draw, uni = np.random.default_rng(0), np.random.default_rng(1)
    eng.new_games([-1] * boards)
    eng.search()                                             # warm-up on a throw-away search: code objects, buffers, the staging buffer of the row move
    eng.check_errors()
    eng.new_games([-1] * boards)
    sims0 = eng.stats()["simulations"]
    rows = []
    for ply in range(plies):
        is_full = draw.random(boards) < p_full
        u = uni.random(boards)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if cfg == "cap":
            eng.set_budgets(np.where(is_full, full, fast))
        elif cfg == "targets":
            eng.set_visit_targets(np.where(is_full, full, fast))
        eng.search()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = eng.check_errors()
        assert st["boards_pending"] == 0
        idle = int((eng.last_goals == 0).sum()) if eng.last_goals is not None else 0
        rows.append(dict(ply=ply, seconds=dt, network_calls=eng.last_steps, network_rows=eng.last_rows, new_simulations=int(st["simulations"] - sims0),
                         full_boards=int(is_full.sum()), boards_without_new_simulations=idle))
        sims0 = st["simulations"]
        eng.play(u)
        eng.fetch_ply()
    out = dict(config=cfg, boards=boards, full=full, fast=fast, p_full=p_full, plies=rows, seconds=sum(r["seconds"] for r in rows),
               network_rows=sum(r["network_rows"] for r in rows), new_simulations=sum(r["new_simulations"] for r in rows), device=torch.cuda.get_device_name(0))
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="4096:800:100,512:100:25", help="boards:full:fast, comma separated")
    ap.add_argument("--p-full", type=float, default=0.25)
    ap.add_argument("--plies", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        cfg, boards, full, fast = a.child.split(":")
        return child(cfg, int(boards), int(full), int(fast), a.p_full, a.plies)
    results, lines = [], []
    for shape in a.shapes.split(","):
        for cfg in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "%s:%s" % (cfg, shape), "--p-full", str(a.p_full), "--plies", str(a.plies)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)      # the parent never opens the GPU
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                print(p.stdout[-4000:])
                raise SystemExit("configuration %s %s failed (exit status %d): stopping here" % (cfg, shape, p.returncode))
            r = json.loads(res[-1][len("RESULT "):])
            results.append(r)
            lines.append("%-7s %5d boards  %4d / %-4d p_full %.2f  %d plies  %7.3f s  %9d network rows  %9d new simulations"
                         % (cfg, r["boards"], r["fast"], r["full"], r["p_full"], len(r["plies"]), r["seconds"], r["network_rows"], r["new_simulations"]))
            for q in r["plies"]:
                lines.append("          ply %d  %7.3f s  %4d network calls  %9d rows  %9d new simulations  %5d full boards  %5d boards without a new simulation"
                             % (q["ply"], q["seconds"], q["network_calls"], q["network_rows"], q["new_simulations"], q["full_boards"], q["boards_without_new_simulations"]))
            print("\n".join(lines[-1 - len(r["plies"]):]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=results[0]["device"], results=results), f, indent=1)
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
            f.write("tools/visit_target_bench.py on %s: the first plies of self-play, f16 network, random-init weights, start positions, sampled moves\n" % results[0]["device"])
            f.write("reuse = reuse_subtree alone, cap = playout_cap budgets without reuse, targets = reuse_subtree + visit_targets (the same fast / full draw)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
