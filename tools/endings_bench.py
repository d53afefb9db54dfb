"""Resignation and adjudicated game endings (args["endings"], sz_set_endings): what the option does to a self-play cycle, on the GPU.
The same seeded play_games twice, the option off and on: the same Chess960 starts, the same sampling uniforms per (game, ply), the same
holdout games, f16 MFMA network with random-init weights, every game cut at --max-plies.  One fresh process per leg under its own time
limit; the first leg that fails ends the tool.  Reported per leg:

  plies            game plies searched, summed over the games, and the longest game (what bounds a cycle from below)
  lock-step plies  search / play rounds of the engine
  simulations, network rows, wall time of play_games
  how the games ended, and the holdout report (sim.ending_report)

Nothing is gated: these are first measurements against the option-off leg of the same code.  What the option saves depends on the network:
a random-init network's values say nothing about who wins, so the numbers show the mechanism and its cost, not the saving of a trained run.
The effect of the option on playing strength is unmeasured.

    python tools/endings_bench.py --out profiles/endings.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(on, a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import sigma_zero_amd as sz
    from sigma_zero_amd.fastnet import FastPolicyNet
    from sigma_zero_amd.sim import play_games, ending_report
    from sigma_zero_amd import build
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.manual_seed(0)
    net = FastPolicyNet(sz.policyNN({}).cuda().eval(), operands="fp16")
    args = {"C": 2, "num_searches": a.searches}
    if a.solver:
        args["solver"] = True
    if on:
        args["endings"] = {"resign_value": a.resign_value, "resign_patience": a.resign_patience, "resign_min_ply": a.resign_min_ply,
                           "draw_value": a.draw_value, "draw_patience": a.draw_patience, "draw_min_ply": a.draw_min_ply, "proven": bool(a.solver),
                           "holdout": a.holdout}
    rng = np.random.default_rng(7)
    starts = rng.integers(0, 960, size=a.games).tolist()
    held = (rng.random(a.games) < a.holdout).tolist()
    uniforms = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    play_games(net, {"C": 2, "num_searches": 8}, 2, c960=True, scharnagl=[0, 1], uniforms=uniforms, max_plies=2, learning=True)      # warm-up: code objects, buffers
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    games = play_games(net, args, a.games, c960=True, scharnagl=starts, uniforms=uniforms, max_plies=a.max_plies, learning=True, n_boards=a.boards,
                       stats=stats, holdout=(lambda g: held[g]) if on else None)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    plies = [len(g["chosen_actions"]) for g in games]
    out = dict(on=bool(on), games=a.games, boards=a.boards, searches=a.searches, max_plies=a.max_plies, seconds=seconds, game_plies=int(sum(plies)),
               longest_game=int(max(plies)), lockstep_plies=stats["plies"], simulations=stats["sims"], network_rows=stats["nn_rows"],
               samples=int(sum(len(g["actions"]) for g in games)), report=ending_report(games), endings=args.get("endings"),
               source_hash=build.source_hash("all"), device=torch.cuda.get_device_name(0))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="", help="what to name the code by in the report (the tool itself records the kernel sources' hash)")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--boards", type=int, default=256)
    ap.add_argument("--searches", type=int, default=128)
    ap.add_argument("--max-plies", type=int, default=300)
    ap.add_argument("--solver", action="store_true", help="the solver on both legs, and `proven` on the on leg")
    ap.add_argument("--resign-value", type=float, default=-0.8)
    ap.add_argument("--resign-patience", type=int, default=3)
    ap.add_argument("--resign-min-ply", type=int, default=10)
    ap.add_argument("--draw-value", type=float, default=0.02)
    ap.add_argument("--draw-patience", type=int, default=10)
    ap.add_argument("--draw-min-ply", type=int, default=60)
    ap.add_argument("--holdout", type=float, default=0.1)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child == "on", a)
    passed = [x for x in sys.argv[1:]]
    results, lines = [], []
    for leg in ("off", "on"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", leg] + passed
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)      # the parent never opens the GPU
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(p.stdout[-4000:])
            raise SystemExit("leg %s failed (exit status %d): stopping here" % (leg, p.returncode))
        r = json.loads(res[-1][len("RESULT "):])
        results.append(r)
        rep = r["report"]
        lines.append("%-3s  %7d game plies  longest game %4d  %5d lock-step plies  %10d simulations  %9d network rows  %6d samples  %8.2f s\n"
                     "     ended by: rules %d, max_plies %d, resign %d, draw adjudicated %d, proven %d; holdout games %d, marks %d "
                     "(resign %d, of which wrong %d; draw %d, of which wrong %d)"
                     % (leg, r["game_plies"], r["longest_game"], r["lockstep_plies"], r["simulations"], r["network_rows"], r["samples"], r["seconds"],
                        rep["rules"], rep["max_plies"], rep["resigned"], rep["adjudicated_draws"], rep["adjudicated_proven"], rep["holdout_games"],
                        rep["holdout_marks"], rep["resign_marks"], rep["resign_false_positives"], rep["draw_marks"], rep["draw_false_positives"]))
        print(lines[-1], flush=True)
    off, on = results
    ratio = lambda k: "%.3f" % (on[k] / off[k]) if off[k] else "n/a"
    tail = ("on / off: game plies %s, longest game %s, lock-step plies %s, simulations %s, network rows %s, wall time %s"
            % tuple(ratio(k) for k in ("game_plies", "longest_game", "lockstep_plies", "simulations", "network_rows", "seconds")))
    print(tail)
    head = ("tools/endings_bench.py %s\non %s, code %s (kernel sources %s)\n"
            "%d Chess960 games on %d boards x %d searches, cut at %d plies, f16 network, RANDOM-INIT weights, sampled moves; the two legs share the starts,\n"
            "the uniforms per (game, ply) and the holdout games.  endings on the `on` leg: %s\n"
            % (" ".join(passed), off["device"], a.commit or "unnamed", off["source_hash"], a.games, a.boards, a.searches, a.max_plies, json.dumps(on["endings"])))
    note = ("What this shows: the mechanism end to end at self-play scale, its cost per ply (one extra host copy) and how many plies the chosen\n"
            "thresholds take out of THIS run.  What it does not show: the saving of a trained run.  A random-init network's values carry no\n"
            "information about the result, so which games end early here, and whether the holdout marks are right, says nothing about a trained\n"
            "network; no target was fixed in advance.  One run per leg: the wall times are single measurements.  Strength effect: unmeasured.\n")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(head + "\n" + "\n".join(lines) + "\n" + tail + "\n\n" + note)


if __name__ == "__main__":
    main()
