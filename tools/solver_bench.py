"""Cost and self-play figures of proven-result propagation (sz_set_solver); results are kept in profiles/solver.txt.

  python tools/solver_bench.py step [--solver] [--parent-abi]    mean time of k_search_step over one search, 4096 boards x 100 searches,
                                                                 HIP events around every sz_search_step (policies prepared beforehand)
  python tools/solver_bench.py selfplay                          64 games from the standard start at S = 100, solver off and on, same uniforms

--parent-abi: the library named by SIGMAZERO_LIB was built from the parent commit and lacks the solver's entry points."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sigma_zero_amd import _native as N

if "--parent-abi" in sys.argv:
    for name in ("sz_set_solver", "sz_root_proven", "sz_debug_tree_proven", "sz_solver_stats"):
        N.EXPORTS.pop(name)
from sigma_zero_amd.selfplay import SelfPlayEngine


def step_time(solver, B=4096, S=100, repeats=2):
    args = {"C": 2, "num_searches": S}
    if solver:
        args["solver"] = True
    g = torch.Generator(device="cuda").manual_seed(0)
    policies = [torch.softmax(torch.randn(B, N.SZ_ACTIONS, generator=g, device="cuda"), 1).contiguous() for _ in range(8)]
    value = (torch.rand(B, generator=g, device="cuda") * 2 - 1).contiguous()
    out = []
    for _ in range(repeats + 1):                                     # the first search warms up
        eng = SelfPlayEngine(None, args, B, chess960=False, learning=True, planes_dtype="bits128")
        eng.new_games([-1] * B)
        eng.begin()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(S)]
        for i in range(S):
            ev[i][0].record()
            eng.step(policies[i % 8], value)
            ev[i][1].record()
        torch.cuda.synchronize()
        eng.check_errors()
        out.append(float(np.mean([a.elapsed_time(b) for a, b in ev])) * 1e3)
        eng.close()
    return out[1:]


def selfplay(solver, n=64, S=100, max_plies=1000):
    import sigma_zero_amd as sz
    from sigma_zero_amd.fastnet import FastPolicyNet
    torch.manual_seed(0)
    net = FastPolicyNet(sz.policyNN({}).cuda().eval(), operands="fp16")
    args = {"C": 2, "num_searches": S}
    if solver:
        args["solver"] = True
    eng = SelfPlayEngine(net, args, n, learning=True, planes_dtype="bits128")
    eng.new_games([-1] * n)
    live, plies = np.ones(n, bool), np.zeros(n, np.int64)
    proven_plies = total_plies = 0
    results = np.zeros(n, np.int64)
    rng = np.random.default_rng(7)
    uniforms = rng.random((max_plies, n))
    for ply in range(max_plies):
        eng.set_active(live.astype(np.uint8))
        eng.compact()
        eng.search()
        eng.check_errors()
        if solver:
            proven_plies += int((eng.root_proven()[0][live] != 0).sum())
        total_plies += int(live.sum())
        eng.play(uniforms[ply])
        rec = eng.fetch_ply()
        eng.check_errors()
        plies[live] += 1
        over = live & (rec["game_over"] != 0)
        results[over] = rec["result"][over]
        live &= ~over
        if not live.any():
            break
    st = eng.stats()
    stops = eng.solver_stats()[0] if solver else 0
    eng.close()
    return dict(solver=solver, games=n, unfinished=int(live.sum()), mean_plies=float(plies.mean()), max_plies=int(plies.max()),
                decisive=int((results != 0).sum()), share_sims_on_proven_nodes=stops / max(1, st["simulations"]),
                share_plies_with_proven_root=proven_plies / max(1, total_plies))


if __name__ == "__main__":
    if sys.argv[1] == "step":
        solver = "--solver" in sys.argv
        print("k_search_step mean us per step, 4096 boards x 100 searches, solver %s, lib %s: %s"
              % ("on" if solver else "off", os.path.basename(os.environ.get("SIGMAZERO_LIB", "default")), ["%.1f" % x for x in step_time(solver)]))
    else:
        for solver in (False, True):
            print(selfplay(solver))
