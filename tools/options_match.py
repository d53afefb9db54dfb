"""Search configuration A against search configuration B on the GPU (arena.play_options_match over sz_play_moves): two engines in one
process on one GPU play colour-swapped pairs of Chess960 games against each other with the same network, and the result is scored in pairs
(arena.match_stats: score, pentanomial counts, Elo with a 95 % interval).

    python tools/options_match.py --a solver=true --b solver=false --pairs 32 --searches 64 --out profiles/options_match.txt

--a / --b take key=value engine args on top of the shared ones (C = 2, num_searches = --searches); values are read as JSON where they
parse (true, 4, 0.5, {"resign_value": -0.9}) and as strings otherwise.  Prints one JSON line.  The defaults (32 pairs, 64 searches, games
cut at 160 plies) finish in a few minutes.  A side that plays greedy moves takes lower-confidence-bound move selection through its engine:
--a 'lcb={"stdevs": 5.0, "min_visit_prop": 0.15}' (selfplay.lcb_options_of).

With the random-init weights this tool makes, the only ones the project has, the number says NOTHING about the strength of a trained
configuration: a random network's values carry no information about who wins, so the match measures how two searches differ when both are
steered by noise.  It shows that the instrument works and what it costs per ply."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_args(pairs):
    out = {}
    for kv in pairs or []:
        if "=" not in kv:
            raise SystemExit("expected key=value, got %r" % kv)
        k, v = kv.split("=", 1)
        try:
            out[k] = json.loads(v)
        except ValueError:
            out[k] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", nargs="*", default=[], metavar="KEY=VALUE", help="engine args of configuration A")
    ap.add_argument("--b", nargs="*", default=[], metavar="KEY=VALUE", help="engine args of configuration B")
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--searches", type=int, default=64)
    ap.add_argument("--max-plies", type=int, default=160)
    ap.add_argument("--sample-plies", type=int, default=4, help="each side's first moves sampled from the visits: the games of different pairs differ")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--classical", action="store_true", help="the classical start in place of Chess960 starts")
    ap.add_argument("--check-positions", action="store_true")
    ap.add_argument("--out", default=None, help="also write the line, with its caveat, to this file")
    a = ap.parse_args()
    if not 1 <= a.pairs <= 4096:
        raise SystemExit("--pairs must be in 1..4096")
    import torch
    sys.path.insert(0, ROOT)
    import sigma_zero_amd as sz
    from sigma_zero_amd import build
    from sigma_zero_amd.arena import play_options_match
    from sigma_zero_amd.fastnet import FastPolicyNet
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.manual_seed(0)
    net = FastPolicyNet(sz.policyNN({}).cuda().eval(), operands="fp16")
    shared = {"C": 2, "num_searches": a.searches}
    args_a, args_b = dict(shared, **parse_args(a.a)), dict(shared, **parse_args(a.b))
    timing = {}
    t0 = time.perf_counter()
    res = play_options_match(net, args_a, args_b, a.pairs, chess960=not a.classical, sample_plies=a.sample_plies, seed=a.seed, max_plies=a.max_plies,
                             check_positions=a.check_positions, timing=timing)
    seconds = time.perf_counter() - t0
    timing.pop("final_positions", None)
    res.pop("results", None)
    out = dict(args_a=args_a, args_b=args_b, n_pairs=a.pairs, max_plies=a.max_plies, sample_plies=a.sample_plies, seed=a.seed, seconds=seconds,
               weights="random-init", source_hash=build.source_hash("all"), device=torch.cuda.get_device_name(0), **timing, **res)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            shown = "--a %s --b %s --pairs %d --searches %d --max-plies %d --sample-plies %d --seed %d%s" % (
                " ".join(a.a), " ".join(a.b), a.pairs, a.searches, a.max_plies, a.sample_plies, a.seed, " --classical" if a.classical else "")
            f.write("tools/options_match.py %s\n\n%s\n\n" % (shown, line))
            f.write("seconds per searched ply: A %.4f, B %.4f (search + play + fetch of one engine, %d and %d searched plies); whole match %.1f s.\n"
                    % (timing["seconds_per_ply_a"], timing["seconds_per_ply_b"], timing["searched_plies_a"], timing["searched_plies_b"], seconds))
            f.write("RANDOM-INIT weights, the only ones that exist here: this number says nothing about the strength of either configuration under a\n"
                    "trained network.  A random network's values carry no information about the result of a game, so the match compares two searches\n"
                    "steered by noise.  One run, one seed.  It shows that the instrument runs end to end and what a ply costs; the strength effect of\n"
                    "every option stays unmeasured.\n")


if __name__ == "__main__":
    main()
