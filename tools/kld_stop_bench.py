"""KLD-gain early stopping (args["kld_stop"], sz_set_kld_stop): what a search costs with the option off and on, on the GPU.
4096 boards from the start position, bf16 MFMA network with random-init weights, a learning engine; whole searches of --searches simulations
are timed.  Legs: the option off, on (lc0's training values, {"min_gain": 5e-6, "interval": 100}, the interval capped at --searches) and, with
--parent-tree DIR (a checkout of the parent commit with its library built), the default path of that checkout, so that "no default kernel
changed" is also a measurement: the off leg is compared with the parent, never with itself.  The legs run alternately (off, parent, on, off,
...), one fresh process per run under its own time limit, all in one session on one GPU; the first run that fails ends the tool.  Reported
per search:

  ms per step       wall time of SelfPlayEngine.search (network call + tree step, every step of the search) / its number of steps
  ms per search     that wall time; with the option on it holds the checks and the batch shrinks (one stream synchronisation each)
  simulations       new simulations made per board (sz_stats), and network rows evaluated per board (SelfPlayEngine.last_rows)
  shrinks           calls of sz_compact_searching in the search, each a stream synchronisation

and per leg the spread of its repeats.  Nothing is gated.  With random-init weights the figures say nothing about a trained network's
positions, where the visit distribution settles much sooner; the effect of the option on playing strength is unmeasured.

    python tools/kld_stop_bench.py --searches 800 --out profiles/kld_stop_800.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON = {"min_gain": 5e-6, "interval": 100}


def child(leg, root, boards, searches, plies, min_gain):
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
        args["kld_stop"] = {"min_gain": min_gain, "interval": min(ON["interval"], searches)}
    eng = SelfPlayEngine(net, args, boards, learning=True, planes_dtype="bits128")
    warm = SelfPlayEngine(net, dict(args, num_searches=8, kld_stop=None), boards, learning=True, planes_dtype="bits128")
    warm.new_games([-1] * boards)
    warm.search()                                            # warm-up on a throw-away engine: code objects, buffers, the network's first calls
    warm.check_errors()
    warm.close()
    shrinks = [0]
    inner = eng._compact_searching

    def counted():
        shrinks[0] += 1
        return inner()
    eng._compact_searching = counted
    eng.new_games([-1] * boards)
    ms, total, sims, rows, nshr = [], [], [], [], []
    for ply in range(plies):
        st0, shrinks[0] = eng.stats(), 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.search()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = eng.check_errors()
        assert st["boards_pending"] == 0 and eng.last_steps > 0
        ms.append(1000.0 * dt / eng.last_steps)
        total.append(1000.0 * dt)
        sims.append(float(st["simulations"] - st0["simulations"]) / boards)
        rows.append(float(eng.last_rows) / boards)
        nshr.append(shrinks[0])
        eng.play([-1.0] * boards)
    stopped = list(eng.kld_stop_stats()) if leg == "on" else None
    eng.close()
    print("RESULT " + json.dumps(dict(leg=leg, boards=boards, searches=searches, ms=ms, total=total, sims=sims, rows=rows, shrinks=nshr, stopped=stopped,
                                      device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--searches", type=int, default=800)
    ap.add_argument("--plies", type=int, default=2, help="timed searches per process")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the legs, run alternately")
    ap.add_argument("--min-gain", type=float, default=ON["min_gain"], help="the on leg's threshold")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: adds the `parent` leg")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child")
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.root, a.boards, a.searches, a.plies, a.min_gain)
    legs = ["off"] + (["parent"] if a.parent_tree else []) + ["on"]
    lines, device, per_leg, stopped = [], None, {leg: [] for leg in legs}, None
    for rnd in range(a.rounds):
        for leg in legs:
            # the parent leg runs THIS file's child on the parent's package: the option's key is never set there
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "off" if leg == "parent" else leg, "--boards", str(a.boards), "--searches", str(a.searches),
                   "--plies", str(a.plies), "--min-gain", repr(a.min_gain), "--root", os.path.abspath(a.parent_tree) if leg == "parent" else ROOT]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)      # the parent never opens the GPU
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                print(p.stdout[-4000:])
                raise SystemExit("leg %s of round %d failed (exit status %d): stopping here" % (leg, rnd, p.returncode))
            r = json.loads(res[-1][len("RESULT "):])
            device = r["device"]
            per_leg[leg] += r["ms"]
            stopped = r["stopped"] or stopped
            f = lambda key, fmt: "  ".join(fmt % x for x in r[key])
            lines.append("round %d  %-6s  ms per step: %s   ms per search: %s   simulations per board: %s   network rows per board: %s   shrinks: %s"
                         % (rnd, leg, f("ms", "%.4f"), f("total", "%.1f"), f("sims", "%.1f"), f("rows", "%.1f"), f("shrinks", "%d")))
            print(lines[-1], flush=True)
    for leg in legs:
        v = sorted(per_leg[leg])
        lines.append("%-6s  median %.4f ms per step over %d searches, mean %.4f, min %.4f, max %.4f (spread %.1f %% of the median)"
                     % (leg, v[len(v) // 2], len(v), sum(v) / len(v), v[0], v[-1], 100.0 * (v[-1] - v[0]) / v[len(v) // 2]))
        print(lines[-1], flush=True)
    if stopped:
        lines.append("on      sz_kld_stop_stats of the last run: %d board searches stopped early, %d checks evaluated, %d simulations not made" % tuple(stopped))
        print(lines[-1], flush=True)
    head = ("tools/kld_stop_bench.py on %s: %d boards from the start position, bf16 network, random-init weights, learning engine, searches of %d\n"
            "simulations; `on` = args[\"kld_stop\"] = {\"min_gain\": %r, \"interval\": %d}%s; legs run alternately in one session, one process per\n"
            "run, after a warm-up search on a throw-away engine.  Nothing is gated.\n"
            % (device, a.boards, a.searches, a.min_gain, min(ON["interval"], a.searches),
               "; `parent` = the default path of a checkout of the parent commit" if a.parent_tree else ""))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
