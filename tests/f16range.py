"""Inputs for tests of the f16 networks' range (FastPolicyNet(operands="fp16") stores activations as f16: |v| >= 65520 rounds to inf), checked on the CPU by
test_nnref.py so that a GPU test can rely on them: a healthy policyNN (activations O(1)), four random boards (0 / 1 planes at density 0.12), and per site a copy
of the network that reaches 0.9 x 65504 (in range) or 2 x 65504 (out of range) THERE and nowhere else first (nnref.site_net).  Built once per process."""
import copy
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


def site_values(net, site, x, operands="fp16"):
    """the values handed to the rounding at `site`, WITH their sign: [B, 256, 8, 8] double (site_maxima gives each board's largest magnitude of these)"""
    em = nnref.Emulated(net, operands)
    inp, res = nnref._site_input(em, x, site)
    conv, bn, pad = nnref._site_layer(net, site)
    w, b = nnref.fold_bn(conv.weight, bn, f32=operands is not None)
    v = nnref.conv2d(inp, nnref.round_to(w, operands), b, padding=pad)
    return v if res is None else v + res


@functools.lru_cache(maxsize=None)
def one_bad_board(site="block9.t"):
    """(net, bad board index, per-site peaks of the net): the network scaled at `site` so that the rounding-to-inf point 65520 lies at the geometric mean of the
    largest and the second largest board's peak there (f16-rounded weights): ONE of the four boards overflows, and it overflows to +inf.  (A peak of -65520
    or below packs to -inf and the ReLU makes the 0 of it that the exact value gives too: such a board is healthy.  Where the largest board's peak is negative,
    the site's BatchNorm gamma and beta change sign first: every magnitude at the site stays, every sign flips.)"""
    x = boards()
    base = base_net()
    p = nnref.Emulated(base, "fp16").site_maxima(x)[site]
    order = torch.argsort(p, descending=True)
    top, second = float(p[order[0]]), float(p[order[1]])
    if float(site_values(base, site, x)[order[0]].max()) < top:              # the peak of the largest board is a negative value
        base = copy.deepcopy(base)
        bn = nnref._site_layer(base, site)[1]
        with torch.no_grad():
            bn.weight.neg_(); bn.bias.neg_()
    net = nnref.site_net(base, site, nnref.F16_INF_FROM * (top / second) ** 0.5, x, operands="fp16", rtol=1e-4)
    q = nnref.Emulated(net, "fp16").site_maxima(x)
    return net, int(order[0]), q


# ---- the same for SplitPolicyNet(operands="fp16") ----------------------------------------------------------------------------------------------------------------
# Its constructor refuses a folded weight of 64 or more (weights are packed times 2^10 into f16), and net_at() reaches its target from O(1) activations with ONE
# layer: folded weights of 2e3 .. 1e4 at every site.  Here the magnitude is reached in two layers: the site in front is lifted to SPLIT_LIFT, then the site itself
# to the target (folded weights of 10 .. 50 each).  The stem has no layer in front (its input is the 0 / 1 planes: 59000 from at most 1071 of them needs
# weights of 55 on average): there is no such net for it.  The split kernels take the ReLU in f32 and pack then: only a value of +65520 or more overflows.
SPLIT_LIFT = 512.0
SPLIT_SITES = SITES[1:]
SPLIT_W_LIMIT = 65520.0 / 1024.0


@functools.lru_cache(maxsize=None)
def split_net_at(site, target):
    names = nnref.site_names(19)
    x = boards()
    lifted, _ = nnref.scale_site(base_net(), names[names.index(site) - 1], SPLIT_LIFT, x)
    net = nnref.site_net(lifted, site, target, x)
    # the value head reads the tower output, which here is 400 .. 59000 behind the lifted layer, and computes in f32: it is turned down like every other layer
    # behind the site (v_norm's gamma and beta times a factor), to conv_v1 outputs of at most 1, so that its absolute error can be held to the O(1) bound
    em = nnref.Emulated(net, None)
    m = float(nnref.conv2d(em.tower(x), em.wv, em.bv).abs().max())
    if m > 1:
        with torch.no_grad():
            net.v_norm.weight.mul_(1 / m); net.v_norm.bias.mul_(1 / m)
    return net


def largest_folded_weight(net):
    """what SplitPolicyNet's construction checks against SPLIT_W_LIMIT: the largest |folded weight| of the tower, conv_p1 and conv_p2"""
    em = nnref.Emulated(net, None)
    ws = [em.stem[0]] + [w for blk in em.blocks for w in (blk[0], blk[2])] + [em.p1[0], em.wp2]
    return max(float(w.abs().max()) for w in ws)
