"""The record behind profiles/softmax_range.txt: the probability rows of every softmax site on the probe cases of tests/softmaxref.py against fp64 (worst error / bound
per zone, wrongly zero entries), torch on the device on the same logits, and one SplitPolicyNet forward at 4096 boards.  SIGMAZERO_LIB=<other .so> measures another
build of the library (build.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import build as B
from sigma_zero_amd.fastnet import SplitPolicyNet

import test_gpu_softmax_range as T

print("library %s" % os.path.relpath(B.LIB, ROOT))
print("\n".join(T.record_table()))
torch.manual_seed(0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
split = SplitPolicyNet(sz.policyNN({}).eval(), device="cuda")
planes = torch.randint(0, 256, (n, 1024), dtype=torch.uint8, device="cuda")
for rep in range(2):
    for _ in range(3):
        split(planes)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(10):
        split(planes)
    ev[1].record()
    torch.cuda.synchronize()
    print("SplitPolicyNet forward, %d boards: %.3f ms" % (n, ev[0].elapsed_time(ev[1]) / 10), flush=True)
