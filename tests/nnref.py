"""fp64 emulation of FastPolicyNet (sigma_zero_amd/fastnet.py, csrc/sz_nn.hip) for the tests: policyNN evaluated in double, rounded to the MFMA operand
type (bf16 or f16) at exactly the points where the shipped kernels round, so that the kernels can be compared with it element by element.

Rounding points, as the kernels have them:
  folding    fastnet._fold_bn computes scale / weight / bias in double and casts to f32; the packers then round the f32 weight to the operand type with
             round-to-nearest-even (ElemBF16::from_float / ElemF16::from_float, sz_nn_common.h); biases stay f32 (the accumulators start at them).
  input      the 119 planes are exact 0 / 1 in either type; channels 119..127 of the stem's K dimension are zero.
  stem       x = round(relu(conv + b))                         (k_tower16_bf16 -> acc_tile_to_lds16, sz_nn.hip: pack2 then relu on the packed pair)
  block      t = round(relu(conv1(x) + b1))                    (acc_tile_to_lds16)
             x = relu(round(conv2(t) + b2 + x))                (acc_tile_residual16 / EpiResidual16: f32 add of the stored x, ONE rounding, then relu)
  heads      t = round(relu(conv_p1(x) + bp1))                 (k_heads16_bf16: conv_kloop16 on the folded p1 weights, acc_to_lds16)
             logits = conv_p2(t) on the ROUNDED raw conv_p2 weight (sz_nn_pack_head16[_f16]) + bp2 in f32; softmax over the 4672 logits
             value: conv_v1 with f32 folded weights (wv_f32) on the rounded tower output + bv, relu, then fc_v1 / relu / fc_v2 / tanh in f32
relu(round(v)) == round(relu(v)) for round-to-nearest (round is monotone and keeps the sign), so the order of the two does not matter here.

`operands=None` switches every rounding off: the helper is then policyNN in double.
"""
import numpy as np
import torch
import torch.nn.functional as F

# significand bits (with the implicit one), smallest normal exponent, largest finite value
_FORMATS = {"bf16": (8, -126, float.fromhex("0x1.fep127")), "fp16": (11, -14, 65504.0)}
REPETITION_PLANES = [14 * t + k for t in range(8) for k in (12, 13)]      # sz_hist_plane k = 12, 13 of the 8 history slots
CASTLING_PLANES = [114, 115, 116, 117]                                     # sz_aux_plane j = 2..5


def round_to(x, operands):
    """round f32 values (given in any float dtype) to bf16 / f16 with round-to-nearest-even, subnormals and overflow to inf included; returns double.
    Written from the format's definition (not with Tensor.to) so that the tests can hold it against torch's conversion."""
    if operands is None:
        return x.double()
    bits, emin, fmax = _FORMATS[operands]
    x = x.float().double()                                    # the kernels round f32 values: double -> f32 -> 16 bit, both steps RNE
    _, e = torch.frexp(x)                                     # x = m * 2^e, 0.5 <= |m| < 1
    e = torch.clamp(e - 1, min=emin)                          # exponent of the leading bit; below the normal range the quantum stays 2^(emin - bits + 1)
    q = torch.ldexp(torch.ones_like(x), e - (bits - 1))
    r = torch.round(x / q) * q                                # torch.round: half to even; x / q is exact (power of two)
    return torch.where(r.abs() > fmax, torch.copysign(torch.full_like(r, float("inf")), x), r)      # r is a multiple of the top quantum: > fmax means overflow


def fold_bn(conv_w, bn, conv_b=None, f32=True):
    """fastnet._fold_bn restated: double, then f32 (weights [co, ci, k, k], bias [co]); returned as double tensors holding f32 values (f32=False: kept in double)"""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    w = conv_w.detach().double() * scale.view(-1, 1, 1, 1)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    if conv_b is not None:
        b = b + conv_b.detach().double() * scale
    return (w.float().double(), b.float().double()) if f32 else (w, b)


def folded_convs(net, operands=None):
    """the 39 folded 3x3 convolutions (stem, then conv1 / conv2 of every block) with their weights rounded as the packers store them: [(w, b)]"""
    f32 = operands is not None
    convs = [fold_bn(net.conv1.weight, net.norm_layer, f32=f32)]
    for blk in net.resnet_blocks:
        convs += [fold_bn(blk.conv1.weight, blk.bn1, f32=f32), fold_bn(blk.conv2.weight, blk.bn2, f32=f32)]
    return [(round_to(w, operands), b) for w, b in convs]


def conv2d(x, w, b, padding=0):
    """F.conv2d in double; on the CPU as unfold + one matrix product (torch's direct fp64 convolution takes 3-4x as long there (measured: 128 vs 37 ms for 256 -> 256 channels on 4 boards), and the CPU tests walk 39 of them per network)"""
    if x.is_cuda:
        return F.conv2d(x, w, b, padding=padding)
    B, co = x.shape[0], w.shape[0]
    y = w.reshape(co, -1) @ F.unfold(x, w.shape[2], padding=padding)
    return (y if b is None else y + b.view(1, co, 1)).view(B, co, x.shape[2], x.shape[3])


def _peak(peaks, site, v):
    if peaks is not None:
        peaks[site] = v.abs().flatten(1).max(1).values
    return v


class Emulated:
    """policyNN `net` in double with FastPolicyNet's rounding points for `operands` (None, "bf16", "fp16"); n_blocks < 19 truncates the tower as
    net.resnet_blocks[:n_blocks] does.  Tensors are on `device` (fp64 convolutions: keep the batch to a few hundred boards)."""

    def __init__(self, net, operands=None, n_blocks=None, device="cpu"):
        self.op, self.dev = operands, torch.device(device)
        d = lambda t: t.to(self.dev)
        convs = folded_convs(net, operands)
        n = len(net.resnet_blocks) if n_blocks is None else n_blocks
        self.stem = tuple(map(d, convs[0]))
        self.blocks = [tuple(map(d, convs[1 + 2 * k] + convs[2 + 2 * k])) for k in range(n)]
        f32 = operands is not None
        wp1, bp1 = fold_bn(net.conv_p1.weight, net.p_norm1, f32=f32)
        self.p1 = (d(round_to(wp1, operands)), d(bp1))
        self.wp2 = d(round_to(net.conv_p2.weight.detach(), operands))            # [73, 256, 1, 1]: the raw weight, rounded by sz_nn_pack_head16[_f16]
        self.bp2 = d(net.conv_p2.bias.detach().double())
        wv, bv = fold_bn(net.conv_v1.weight, net.v_norm, f32=f32)
        self.wv, self.bv = d(wv), d(bv)                                                   # f32, not rounded (wv_f32 / bv_f)
        self.fc = [d(t.detach().double()) for t in (net.fc_v1.weight, net.fc_v1.bias, net.fc_v2.weight, net.fc_v2.bias)]

    def r(self, x):
        return round_to(x, self.op)

    def tower(self, planes, peaks=None):
        """planes [B, 119, 8, 8] (0 / 1, any dtype) -> tower output [B, 256, 8, 8] double (values of the operand type when rounding).
        peaks: a dict that receives, per site, each board's largest |value handed to the rounding| (see site_maxima)"""
        x = planes.to(self.dev).double()
        w, b = self.stem
        x = self.r(torch.relu(_peak(peaks, "stem", conv2d(x, w, b, padding=1))))
        for k, (w1, b1, w2, b2) in enumerate(self.blocks):
            t = self.r(torch.relu(_peak(peaks, "block%d.t" % k, conv2d(x, w1, b1, padding=1))))
            x = torch.relu(self.r(_peak(peaks, "block%d.out" % k, conv2d(t, w2, b2, padding=1) + x)))
        return x

    def site_maxima(self, planes):
        """{site: [B] largest |v| of each board} over every value the kernels hand to a 16-bit pack, BEFORE the rounding and before the ReLU (the kernels pack, then
        take the ReLU on the packed pair: a value <= -65520 becomes -inf at the pack too), in the order the kernels compute them: stem, block0.t, block0.out, ...,
        p1 (the policy head's stored intermediate).  f16 rounds to inf from 65520 on: the first site whose maximum reaches it is where the first inf is created."""
        peaks = {}
        self.heads(self.tower(planes, peaks), peaks=peaks)
        return peaks

    def heads(self, x, inference=False, peaks=None):
        """tower output [B, 256, 8, 8] -> (logits or policy [B, 4672], value [B, 1]) as k_heads16_bf16 + k_value_head compute them"""
        x = x.to(self.dev).double()
        t = self.r(torch.relu(_peak(peaks, "p1", conv2d(x, self.p1[0], self.p1[1]))))
        logits = torch.flatten(F.conv2d(t, self.wp2, self.bp2), 1)
        policy = torch.softmax(logits, 1) if inference else logits
        v = torch.relu(torch.flatten(F.conv2d(x, self.wv, self.bv), 1))
        w1, b1, w2, b2 = self.fc
        value = torch.tanh(torch.relu(v @ w1.t() + b1) @ w2.t() + b2)
        return policy, value

    def __call__(self, planes, inference=False):
        return self.heads(self.tower(planes), inference)


def truncated(net, k):
    """a copy of policyNN `net` whose tower is its first k blocks (FastPolicyNet / SplitPolicyNet built on it run the tower kernels with n_blocks = k)"""
    import copy
    t = copy.deepcopy(net)
    t.resnet_blocks = torch.nn.Sequential(*list(t.resnet_blocks)[:k])
    return t


@torch.no_grad()
def trained_regime(net, seed, verbose=True):
    """BatchNorm statistics and weights as a trained network has them, in place on policyNN `net` (eval mode):
      gamma log-uniform in [1e-3, 3] with ~10 % negative and ~4 % exactly zero; beta N(0, 0.2) with ~4 % of the channels at -5 .. -2 (dead after the ReLU);
      running_var log-uniform in [1e-3, 10], the conv weights of each output channel scaled by sqrt(running_var) (the statistics match the data's scale);
      four stem channels that read only the repetition and castling planes, with running_var 1e-4 (folded weights O(100));
      the second convolution of every block scaled so that the residual stream grows to O(100) by block 19.
    Prints the largest folded weight and activation per layer when verbose."""
    g = torch.Generator().manual_seed(seed)
    U = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    dev = next(net.parameters()).device

    def bn_stats(bn, conv_w, gain=1.0):
        n = bn.num_features
        var = 10 ** (U(n) * 4 - 3)                                    # 1e-3 .. 10
        gamma = 10 ** (U(n) * np.log10(3e3) - 3)                      # 1e-3 .. 3
        gamma = torch.where(U(n) < 0.1, -gamma, gamma)
        gamma = torch.where(U(n) < 0.04, torch.zeros_like(gamma), gamma)
        beta = torch.randn(n, generator=g, dtype=torch.float64) * 0.2
        beta = torch.where(U(n) < 0.04, -2 - 3 * U(n), beta)
        mean = torch.randn(n, generator=g, dtype=torch.float64) * var.sqrt() * 0.3
        bn.running_var.copy_(var); bn.weight.copy_(gamma * gain); bn.bias.copy_(beta); bn.running_mean.copy_(mean)
        if conv_w is not None:
            conv_w.mul_(var.sqrt().view(-1, *([1] * (conv_w.dim() - 1))).to(conv_w))

    bn_stats(net.norm_layer, net.conv1.weight)
    for blk in net.resnet_blocks:
        bn_stats(blk.bn1, blk.conv1.weight)
        bn_stats(blk.bn2, blk.conv2.weight, gain=0.6)
    bn_stats(net.p_norm1, net.conv_p1.weight)
    net.v_norm.running_var.fill_(0.5); net.v_norm.weight.fill_(0.8); net.v_norm.bias.fill_(0.1); net.v_norm.running_mean.zero_()
    # stem channels on the rarely-set planes: 3x3 weights of O(1) on the repetition / castling planes only, running_var 1e-4 -> folded O(100)
    rare = REPETITION_PLANES + CASTLING_PLANES
    for c in range(4):
        w = torch.zeros(net.conv1.weight.shape[1:], dtype=torch.float64)
        w[rare] = (U(len(rare), 3, 3) * 2 - 1) * 1.0
        net.conv1.weight[c] = w.to(net.conv1.weight)
        net.norm_layer.running_var[c] = 1e-4; net.norm_layer.weight[c] = 1.0; net.norm_layer.bias[c] = 0.0; net.norm_layer.running_mean[c] = 0.0
    if verbose:
        report(net)
    return net


@torch.no_grad()
def report(net, planes=None):
    """print max |folded weight| per layer and, for `planes` (default: 16 random boards), max |activation| after the stem and each block"""
    convs = folded_convs(net)
    if planes is None:
        g = torch.Generator().manual_seed(0)
        planes = (torch.rand(16, 119, 8, 8, generator=g) < 0.12).double()
    em = Emulated(net, None)
    x = planes.double()
    w, b = em.stem
    x = torch.relu(F.conv2d(x, w, b, padding=1))
    lines = ["stem      max|w| %9.3g  max|x| %9.3g" % (float(convs[0][0].abs().max()), float(x.abs().max()))]
    for k, (w1, b1, w2, b2) in enumerate(em.blocks):
        t = torch.relu(F.conv2d(x, w1, b1, padding=1))
        x = torch.relu(F.conv2d(t, w2, b2, padding=1) + x)
        lines.append("block %2d  max|w| %9.3g %9.3g  max|t| %9.3g  max|x| %9.3g" % (k, float(w1.abs().max()), float(w2.abs().max()), float(t.abs().max()), float(x.abs().max())))
    print("\n".join(lines))
    return float(x.abs().max())


# ---- networks that reach a chosen magnitude at a chosen place (tests of f16's range) -------------------------------------------------------------------------
F16_INF_FROM = 65520.0                                     # f32 -> f16 (round to nearest even) gives inf from 65504 + half a quantum (32 / 2) on


def site_names(n_blocks):
    return ["stem"] + [s % k for k in range(n_blocks) for s in ("block%d.t", "block%d.out")] + ["p1"]


def _site_layer(net, site):
    """(convolution, BatchNorm, padding) that produce `site`"""
    if site == "stem":
        return net.conv1, net.norm_layer, 1
    if site == "p1":
        return net.conv_p1, net.p_norm1, 0
    blk, which = site.split(".")
    blk = net.resnet_blocks[int(blk[5:])]
    return (blk.conv1, blk.bn1, 1) if which == "t" else (blk.conv2, blk.bn2, 1)


def _site_input(em, x, site):
    """(input of the site's convolution, residual added behind it or None) under emulation `em`: what the layers in front of the site hand it"""
    x = em.r(torch.relu(conv2d(x.to(em.dev).double(), *em.stem, padding=1))) if site != "stem" else x.to(em.dev).double()
    if site == "stem":
        return x, None
    for k, (w1, b1, w2, b2) in enumerate(em.blocks):
        if site == "block%d.t" % k:
            return x, None
        t = em.r(torch.relu(conv2d(x, w1, b1, padding=1)))
        if site == "block%d.out" % k:
            return t, x
        x = torch.relu(em.r(conv2d(t, w2, b2, padding=1) + x))
    assert site == "p1", site
    return x, None


@torch.no_grad()
def scale_site(net, site, target, x, operands=None, rtol=0.01):
    """a copy of policyNN `net` in which ONE BatchNorm's gamma and beta (the one that produces `site`) are multiplied by a common factor, found by bisection on
    Emulated(net, operands), such that the largest |value handed to the rounding| at `site` over the boards `x` [B, 119, 8, 8] is within `rtol` of `target`.
    The layers in front of the site do not change, so their output is computed once and each probe is the site's own convolution.  Returns (net, reached)."""
    import copy
    net = copy.deepcopy(net)
    conv, bn, pad = _site_layer(net, site)
    inp, res = _site_input(Emulated(net, operands), x, site)
    g0, b0 = bn.weight.detach().double().clone(), bn.bias.detach().double().clone()

    def peak(s):
        bn.weight.copy_(g0 * s); bn.bias.copy_(b0 * s)
        w, b = fold_bn(conv.weight, bn, f32=operands is not None)
        v = conv2d(inp, round_to(w, operands).to(inp.device), b.to(inp.device), padding=pad)
        return float((v if res is None else v + res).abs().max())

    s = target / peak(1.0)                                 # exact where the site is its convolution alone (no residual), up to the roundings
    m = peak(s)
    if abs(m / target - 1) > rtol:
        lo = hi = s
        while peak(lo) > target:
            lo /= 4
        while peak(hi) < target:
            hi *= 4
        for _ in range(200):
            s = (lo * hi) ** 0.5
            m = peak(s)
            if abs(m / target - 1) <= rtol:
                break
            lo, hi = (s, hi) if m < target else (lo, s)
    assert abs(m / target - 1) <= rtol, (site, target, m)
    return net, m


@torch.no_grad()
def site_net(net, site, target, x, quiet=1000.0, operands=None, rtol=0.01):
    """scale_site(net, site, target, x, operands, rtol), then every layer BEHIND the site is turned down (its BatchNorm's gamma and beta times a factor < 1, in fp64 on
    Emulated(net, None)) so that the site is the one place where the network is that large: a later `t` or `p1` that exceeds `quiet` is scaled to `quiet`; a later
    convolution into the residual stream is scaled so that it moves the stream by at most target / 1000 (19 blocks: 2 %), since the stream itself carries the
    site's magnitude to the end of the tower when the site is the stem or a block's output.  Returns the new net."""
    net, _ = scale_site(net, site, target, x, operands, rtol)
    names = site_names(len(net.resnet_blocks))
    em = Emulated(net, None)
    x = x.double()
    cur, t = None, None
    for name in names:
        conv, bn, pad = _site_layer(net, name)
        w, b = fold_bn(conv.weight, bn, f32=False)
        is_out = name.endswith(".out")
        inp = x if name == "stem" else (t if is_out else cur)
        v = conv2d(inp, w, b, padding=pad)
        if names.index(name) > names.index(site):
            m, cap = float(v.abs().max()), (target / 1000 if is_out else quiet)
            if m > cap:
                bn.weight.mul_(cap / m); bn.bias.mul_(cap / m)
                v = v * (cap / m)
        if is_out:
            cur = torch.relu(v + cur)
        elif name == "stem":
            cur = torch.relu(v)
        else:
            t = torch.relu(v)
    return net


@torch.no_grad()
def benign_stats(net, seed):
    """BatchNorm statistics of a healthy network (activations O(1) everywhere), in place: the starting point of the range tests"""
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(torch.randn(n, generator=g) * 0.05); m.running_var.copy_(0.5 + torch.rand(n, generator=g))
            m.weight.copy_(0.7 + 0.6 * torch.rand(n, generator=g)); m.bias.copy_(torch.randn(n, generator=g) * 0.05)
    net.conv_p2.bias.copy_(torch.randn(net.conv_p2.bias.shape, generator=g) * 0.5)
    return net


def random_planes(n, seed, density=0.12):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 119, 8, 8, generator=g) < density).double()
