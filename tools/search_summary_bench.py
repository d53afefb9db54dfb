"""The search summary (args["search_targets"], sz_set_search_summary): what one sz_play costs with the option off and on, on the GPU.  4096
boards from the start position, bf16 MFMA network with random-init weights, searches of 64 simulations; after each search one sz_play with
seeded uniforms is timed.  Legs: the option off, on (sz_play launches k_summary_pre before k_play and k_summary_post after it: two waves' worth
of at most 218 f64 terms per board) and, with --parent-tree DIR (a checkout of the parent commit with its library built), the default path of
that checkout, so that "no default kernel changed" is also a measurement.  The legs run alternately (off, on[, parent], off, ...), one fresh
process per run under its own time limit, all in one session on one GPU; the first run that fails ends the tool.  Reported per play:

  ms per sz_play    GPU time between two events around SelfPlayEngine.play (the 32 KiB upload of the uniforms and the launches)

and per leg the spread of its repeats.  sz_play runs once per ply against num_searches search steps: nothing is gated.

    python tools/search_summary_bench.py --parent-tree PARENT_TREE        (profiles/search_summary.txt, section 3, holds such a run)
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
        args["search_targets"] = {"q_ratio": 0.5, "surprise_fraction": 0.5}
    eng = SelfPlayEngine(net, args, boards, learning=True, planes_dtype="bits128")
    rng = np.random.default_rng(0)
    eng.new_games([-1] * boards)
    out = []
    for rep in range(plays + 1):                             # the first play is the warm-up (code objects, buffers) and is not reported
        eng.search()
        st = eng.check_errors()
        assert st["boards_pending"] == 0
        u = rng.random(boards)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        eng.play(u)
        t1.record()
        torch.cuda.synchronize()
        if rep:
            out.append(t0.elapsed_time(t1))
    assert not eng.check_errors()["boards_error"]
    stats, mean, n_valid = (0, 0), None, 0
    if leg == "on":
        stats, s, rec = eng.search_summary_stats(), eng.fetch_search_summary(), eng.fetch_ply()
        ok = s["valid"].astype(bool)
        assert (ok == rec["active"].astype(bool)).all(), "a summary for exactly the boards that played (a board whose game is over sits out)"
        n_valid = int(ok.sum())
        mean = [float(s[k][ok].mean()) for k in ("root_q", "best_q", "surprise")]
    eng.close()
    print("RESULT " + json.dumps(dict(leg=leg, boards=boards, searches=searches, ms=out, stats=stats, mean=mean, n_valid=n_valid, device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--searches", type=int, default=64)
    ap.add_argument("--plays", type=int, default=6, help="timed plies per process")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the legs, run alternately")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: adds the `parent` leg")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child")
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.root, a.boards, a.searches, a.plays)
    legs = ["off", "on"] + (["parent"] if a.parent_tree else [])
    lines, device, per_leg = [], None, {leg: [] for leg in legs}
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
            per_leg[leg] += r["ms"]
            lines.append("round %d  %-6s  ms per sz_play: %s%s" % (rnd, leg, "  ".join("%.4f" % x for x in r["ms"]),
                                                                  "   summaries made, terms dropped = %s; boards that played the last ply: %d; their mean root_q, best_q, surprise = %s"
                                                                  % (tuple(r["stats"]), r["n_valid"], tuple(round(x, 6) for x in r["mean"])) if leg == "on" else ""))
            print(lines[-1], flush=True)
    for leg in legs:
        v = sorted(per_leg[leg])
        lines.append("%-6s  median %.4f ms per sz_play over %d plays, mean %.4f, min %.4f, max %.4f (spread %.1f %% of the median)"
                     % (leg, v[len(v) // 2], len(v), sum(v) / len(v), v[0], v[-1], 100.0 * (v[-1] - v[0]) / v[len(v) // 2]))
        print(lines[-1], flush=True)
    head = ("tools/search_summary_bench.py on %s: %d boards from the start position, bf16 network, random-init weights, learning engine, searches of %d\n"
            "simulations; `on` = args[\"search_targets\"] = {\"q_ratio\": 0.5, \"surprise_fraction\": 0.5}%s; legs run alternately in one session, one\n"
            "process per run, the first play of a process not reported.  Nothing is gated.\n"
            % (device, a.boards, a.searches, "; `parent` = the default path of a checkout of the parent commit" if a.parent_tree else ""))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
