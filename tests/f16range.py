"""Inputs for tests of the f16 networks' range (FastPolicyNet(operands="fp16") stores activations as f16: |v| >= 65520 rounds to inf), checked on the CPU by
test_nnref.py so that a GPU test can rely on them: a healthy policyNN (activations O(1)), four random boards (0 / 1 planes at density 0.12), and per site a copy
of the network that reaches 0.9 x 65504 (in range) or 2 x 65504 (out of range) THERE and nowhere else first (nnref.site_net).  Built once per process."""
import functools

import torch

import sigma_zero_amd as sz
import nnref

SITES = ("stem", "block9.t", "block15.out", "block18.out", "p1")
F16_MAX = 65504.0
IN_RANGE, OUT_OF_RANGE = 0.9 * F16_MAX, 2 * F16_MAX
N_BOARDS = 4


@functools.lru_cache(maxsize=None)
def base_net(k=None):
    torch.manual_seed(5)
    net = nnref.benign_stats(sz.policyNN({}).eval(), 5)
    return net if k is None else nnref.truncated(net, k)


@functools.lru_cache(maxsize=None)
def boards():
    return nnref.random_planes(N_BOARDS, 1)


@functools.lru_cache(maxsize=None)
def net_at(site, target):
    return nnref.site_net(base_net(), site, target, boards())


@functools.lru_cache(maxsize=None)
def stem_net_at(target):
    """stem-only network (truncated tower, k = 0) whose largest stem value on the four boards, as the f16 KERNEL computes it (f16-rounded weights, exact
    sum), is `target` to 1e-5: the two sides of the rounding-to-inf point, 65400 and 65650"""
    net, reached = nnref.scale_site(base_net(0), "stem", target, boards(), operands="fp16", rtol=1e-5)
    return net, reached


@functools.lru_cache(maxsize=None)
def one_bad_board(site="block9.t"):
    """(net, bad board index, peak of the bad board, peak of the runner-up): the network scaled at `site` so that the rounding-to-inf point 65520 lies at the
    geometric mean of the largest and the second largest board's peak there (f16-rounded weights): ONE of the four boards overflows"""
    x = boards()
    p = nnref.Emulated(base_net(), "fp16").site_maxima(x)[site]
    order = torch.argsort(p, descending=True)
    top, second = float(p[order[0]]), float(p[order[1]])
    net = nnref.site_net(base_net(), site, nnref.F16_INF_FROM * (top / second) ** 0.5, x, operands="fp16", rtol=1e-4)
    q = nnref.Emulated(net, "fp16").site_maxima(x)
    return net, int(order[0]), q
