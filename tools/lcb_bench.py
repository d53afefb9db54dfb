"""The value spread and LCB move selection (args["lcb"], sz_set_lcb): what one k_search_step and one sz_play cost with the option off and on,
on the GPU.  4096 boards from the start position, bf16 MFMA network with random-init weights, searches of 64 simulations.  Legs: the option
off, on (every backup also adds sv * sv into the edge's Q, 8 bytes per edge beside the tree's 32, and k_play forms one bound per root child
and two butterflies per board) and, with --parent-tree DIR (a checkout of the parent commit with its library built), the default path of that
checkout, so that "no default kernel changed" is also a measurement.  The legs run alternately (off, on[, parent], off, ...), one fresh
process per run under its own time limit, all in one session on one GPU; the first run that fails ends the tool.  Reported per process:

  ms per search step   GPU time between two events around each sz_search_step launch of a whole search (the tree kernel alone: the network's
                       evaluation lies outside the interval), averaged over the steps; the first search of a process is the warm-up and is
                       not reported
  ms per sz_play       GPU time between two events around SelfPlayEngine.play (the 32 KiB upload of the uniforms and the launch), every play
                       greedy so that the rule decides on every board of the `on` leg

and per leg the median and the spread of its repeats.  Nothing is known about this cost in advance: nothing is gated.

    python tools/lcb_bench.py --parent-tree PARENT_TREE        (profiles/lcb.txt, section 3, holds such a run)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(leg, root, boards, searches, plays):
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
    if leg == "on":
        args["lcb"] = {"stdevs": 5.0, "min_visit_prop": 0.15}
    eng = SelfPlayEngine(net, args, boards, learning=True, planes_dtype="bits128")
    eng.new_games([-1] * boards)
    step_ms, play_ms = [], []
    for rep in range(plays + 1):                             # the first search and play are the warm-up (code objects, buffers) and are not reported
        eng.begin()
        pairs = []
        with torch.no_grad():
            for _ in range(searches):                        # the network's evaluation lies outside the timed interval
                policy, value = eng.evaluate(eng.planes)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                eng.step(policy, value)
                t1.record()
                pairs.append((t0, t1))
        torch.cuda.synchronize()
        st = eng.check_errors()
        assert st["boards_pending"] == 0
        p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        p0.record()
        eng.play(np.full(boards, -1.0))
        p1.record()
        torch.cuda.synchronize()
        if rep:
            step_ms.append(sum(a.elapsed_time(b) for a, b in pairs) / searches)
            play_ms.append(p0.elapsed_time(p1))
    assert not eng.check_errors()["boards_error"]
    stats, n_played = (0, 0, 0), 0
    if leg == "on":
        stats, got, rec = eng.lcb_stats(), eng.fetch_lcb(), eng.fetch_ply()
        assert ((got["move"] >= 0) == rec["active"].astype(bool)).all(), "a choice for exactly the boards that played"
        n_played = int((got["move"] >= 0).sum())
    eng.close()
    print("RESULT " + json.dumps(dict(leg=leg, boards=boards, searches=searches, step_ms=step_ms, play_ms=play_ms, stats=stats, n_played=n_played,
                                      device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--searches", type=int, default=64)
    ap.add_argument("--plays", type=int, default=5, help="timed searches and plays per process")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the legs, run alternately")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: adds the `parent` leg")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child")
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.root, a.boards, a.searches, a.plays)
    legs = ["off", "on"] + (["parent"] if a.parent_tree else [])
    lines, device = [], None
    per_leg = {leg: dict(step_ms=[], play_ms=[]) for leg in legs}
    for rnd in range(a.rounds):
        for leg in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "off" if leg == "parent" else leg, "--boards", str(a.boards), "--searches", str(a.searches),
                   "--plays", str(a.plays), "--root", os.path.abspath(a.parent_tree) if leg == "parent" else ROOT]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)      # the parent never opens the GPU
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                print(p.stdout[-4000:])
                raise SystemExit("leg %s of round %d failed (exit status %d): stopping here" % (leg, rnd, p.returncode))
            r = json.loads(res[-1][len("RESULT "):])
            device = r["device"]
            for k in ("step_ms", "play_ms"):
                per_leg[leg][k] += r[k]
            lines.append("round %d  %-6s  ms per search step: %s   ms per sz_play: %s%s" % (
                rnd, leg, "  ".join("%.4f" % x for x in r["step_ms"]), "  ".join("%.4f" % x for x in r["play_ms"]),
                "   plays decided, moves other than c*, bad ssqrt arguments = %s; boards that played the last ply: %d" % (tuple(r["stats"]), r["n_played"]) if leg == "on" else ""))
            print(lines[-1], flush=True)
    for what, key in (("search step", "step_ms"), ("sz_play", "play_ms")):
        for leg in legs:
            v = sorted(per_leg[leg][key])
            lines.append("%-6s  median %.4f ms per %s over %d, mean %.4f, min %.4f, max %.4f (spread %.1f %% of the median)"
                         % (leg, v[len(v) // 2], what, len(v), sum(v) / len(v), v[0], v[-1], 100.0 * (v[-1] - v[0]) / v[len(v) // 2]))
            print(lines[-1], flush=True)
    lines.append("extra bytes per edge with the option on: 8 (one f64 beside EdgeStat's 16 and EdgeMeta's 16), allocated by the first enabling call")
    head = ("tools/lcb_bench.py on %s: %d boards from the start position, bf16 network, random-init weights, learning engine, searches of %d\n"
            "simulations; `on` = args[\"lcb\"] = {\"stdevs\": 5.0, \"min_visit_prop\": 0.15}%s; legs run alternately in one session,\n"
            "one process per run, the first search and play of a process not reported.  Nothing is gated.\n"
            % (device, a.boards, a.searches, "; `parent` = the default path of a checkout of the parent commit" if a.parent_tree else ""))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
