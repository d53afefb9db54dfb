"""The shipped inference kernels (csrc/sz_nn.hip k_tower16_bf16 + k_heads16_bf16, FastPolicyNet bf16 / f16 operands) against tests/nnref.py: policyNN in fp64,
rounded to the operand type exactly where the kernels round.  Truncated towers (0, 1, 2 blocks) compare element by element in units of the operand type's last
place; the full network compares in relative L2; the heads compare on the kernel's own tower output.  A bound that "rounds differently" passes and "computes
something else" fails: test_bounds_have_teeth runs the same metrics against plausible bugs, injected on the reference side.
Then the trained regime (nnref.trained_regime: dead and negative BatchNorm channels, running_var down to 1e-4, folded weights O(100)) for the bf16, f16 and
split-precision networks, and the range checks a number format that cannot hold a network has to raise at construction."""
import random

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.fastnet import FastPolicyNet, SplitPolicyNet
from sigma_zero_amd.selfplay import SelfPlayEngine, unpack_bits128

from nnref import Emulated, round_to, trained_regime, truncated

pytestmark = pytest.mark.gpu


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _batches():
    n = _n_cu()
    return sorted({1, 2, 3, n - 1, n, n + 1, 2 * n, 2 * n + 1, 2 * n + n // 3 + 3})


def _benign_net(seed):
    torch.manual_seed(seed)
    net = sz.policyNN({}).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.05); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.7, 1.3); m.bias.normal_(0, 0.05)
        net.conv_p2.bias.normal_(0, 0.5)
    return net


_POS = {}


def _positions():
    """bit-packed engine planes of 2n + n/3 + 3 real positions (Chess960 starts, a few plies of a 2-search self-play), board 1 all zero"""
    if "bits" not in _POS:
        B = max(_batches())
        net = sz.policyNN({}).cuda().eval()
        fast = FastPolicyNet(net)
        eng = SelfPlayEngine(fast, {"C": 2, "num_searches": 2}, B, chess960=True, planes_dtype="bits128")
        rr = random.Random(7)
        eng.new_games([rr.randrange(960) for _ in range(B)])
        urng = np.random.RandomState(7)
        for _ in range(5):
            eng.search(); eng.play(urng.random_sample(B)); eng.fetch_ply()
        eng.begin()
        bits = eng.planes.clone()
        eng.close()
        bits[1] = 0
        img = unpack_bits128(bits)
        _POS["bits"], _POS["img"] = bits, img
        _POS["nchw"] = img[:, :, :119].float().transpose(1, 2).reshape(B, 119, 8, 8).contiguous()
    return _POS["bits"], _POS["img"], _POS["nchw"]


def _dt(operands):
    return torch.float16 if operands == "fp16" else torch.bfloat16


def _tower_bits(fast, planes, operands):
    """kernel tower output as [B, 256, 8, 8] int32 of the operand type's bit patterns (all >= +0 after the ReLU)"""
    B = planes.shape[0]
    y = fast.tower(planes)[0].view(torch.int16)
    return y.view(B, 8, 8, 256).permute(0, 3, 1, 2).to(torch.int32)


def _ref_bits(y64, operands):
    """emulated tower output (values of the operand type) -> the same int32 bit patterns; -0 -> +0 as the kernel's integer ReLU does"""
    return (round_to(y64, operands) + 0.0).abs().to(_dt(operands)).view(torch.int16).to(torch.int32)


def _ulps(got_bits, ref_bits, operands):
    """(max ulp distance, bit-identical fraction of the worst board, excess of the worst board) over [B, 256, 8, 8]: a board's excess is the largest
    (|got - ref| - 1 ulp of ref)+ over its elements divided by the board's max |ref| — the error beyond one rounding at the board's scale (an element near zero
    after cancellation carries the f32 accumulation error of the large terms, many of its own ulps).  Per board, so that one wrong board in a batch of 600 shows."""
    d = (got_bits - ref_bits).abs()
    dt = _dt(operands)
    got, ref = (t.to(torch.int16).view(dt).double() for t in (got_bits, ref_bits))
    bits, emin = (8, -126) if operands == "bf16" else (11, -14)
    _, e = torch.frexp(ref)
    ulp = torch.ldexp(torch.ones_like(ref), torch.clamp(e - 1, min=emin) - (bits - 1))
    B = ref.shape[0]
    over = ((got - ref).abs() - ulp).clamp_min(0).reshape(B, -1).max(1).values
    excess = float((over / ref.abs().reshape(B, -1).max(1).values.clamp_min(1e-30)).max())
    ident = float((d == 0).reshape(B, -1).double().mean(1).min())
    return int(d.max()), ident, excess


def _tower_vals(fast, planes, operands):
    B = planes.shape[0]
    y = fast.tower(planes)[0].view(_dt(operands))
    return y.double().view(B, 8, 8, 256).permute(0, 3, 1, 2)


rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
cen = lambda t: t - t.mean(1, keepdim=True)

# element-by-element bounds of the truncated towers: bit-identical fraction, and the error beyond one ulp relative to the output's maximum.
# Measured on MI355X: see the docstring of test_truncated_tower_is_the_emulation_to_one_ulp
# A one-ulp element bound does not hold beyond the stem: where the kernel's f32 accumulation and the fp64 one straddle a rounding boundary of t, the two t differ by
# one ulp and conv2 carries that difference into every neighbour.  Both metrics are taken per board, the worst board counts.  Measured on MI355X (benign
# statistics, k <= 2, all batches / formats / forms): worst-board bit-identical fraction 0.916 (bf16) / 0.892 (f16), excess 2.6e-3 (bf16) / 3.2e-4 (f16); trained
# regime 0.965 / 0.939 and 8e-5 / 2e-5.  The injected bugs of test_bounds_have_teeth fail them (see its print).
MIN_IDENTICAL = {"bf16": 0.85, "fp16": 0.8}
MAX_EXCESS = {"bf16": 8e-3, "fp16": 1e-3}


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_truncated_tower_is_the_emulation_to_one_ulp(operands):
    """stem + k = 0, 1, 2 blocks against the fp64 emulation element by element: the bit-identical fraction and the error beyond one ulp (MIN_IDENTICAL /
    MAX_EXCESS, measured values there); both input formats (engine bits128, nhwc128), the automatic form choice (one- / two-board workgroups, last round in the
    one-board form) and both forced forms; batches 1, 2, 3, n-1, n, n+1, 2n, 2n+1, 2n+n/3+3 for n CUs."""
    net = _benign_net(21)
    bits, img, nchw = _positions()
    worst = {}
    for k in (0, 1, 2):
        tnet = truncated(net, k)
        fast = FastPolicyNet(tnet, operands=operands)
        with torch.no_grad():
            ref = _ref_bits(Emulated(tnet, operands, device="cuda").tower(nchw), operands)
        for B in _batches():
            for fmt, planes in (("bits128", bits), ("nhwc128", img)):
                for form, flag in (("auto", 0), ("wgb1", N.SZ_NN_TOWER_WGB1), ("wgb2", N.SZ_NN_TOWER_WGB2)):
                    fast.force_wgb = flag
                    mu, ident, ex = _ulps(_tower_bits(fast, planes[:B].contiguous(), operands), ref[:B], operands)
                    worst[(k, B, fmt, form)] = (mu, ident, ex)
            fast.force_wgb = 0
    print("%s truncated towers: max ulp %d, smallest bit-identical fraction %.6f, largest excess %.2e" % (operands, max(v[0] for v in worst.values()),
          min(v[1] for v in worst.values()), max(v[2] for v in worst.values())))
    for key, (mu, ident, ex) in worst.items():
        assert ident >= MIN_IDENTICAL[operands] and ex <= MAX_EXCESS[operands], (operands, key, mu, ident, ex)


# full-network bounds against the emulation (relative L2; value: max absolute).  Measured on MI355X (benign statistics, 300 positions): bf16 tower 5.5e-3, logits
# 1.3e-3, value 2.3e-4; f16 7.0e-4, 1.6e-4, 2.3e-5 (another seed, test_bounds_have_teeth: value 1.0e-3 / 1.2e-4: the max over 300 boards varies).  The fp32-relative bounds of test_gpu_network.py are 0.04 (bf16) / 3e-3 (f16) on the logits
FULL = {"bf16": {"tower": 1.6e-2, "logits": 4e-3, "value": 3e-3}, "fp16": {"tower": 2e-3, "logits": 3e-4, "value": 4e-4}}


def _full_metrics(fast, em, planes, nchw, operands):
    B = planes.shape[0]
    with torch.no_grad():
        p, v = (t.clone() for t in fast(planes, inference=False))
        y = _tower_vals(fast, planes, operands)
        y64 = em.tower(nchw[:B])
        p64, v64 = em.heads(y64)
    return {"tower": rel(y, y64), "logits": rel(cen(p), cen(p64)), "value": float((v.double().view(-1) - v64.view(-1)).abs().max())}


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_full_network_against_the_emulation(operands):
    """19 blocks + fused heads on 300 real positions (one all-zero board) against the fp64 emulation with the kernels' rounding points: tower output and centred
    logits in relative L2, the value in absolute terms, within FULL (measured values there; bounds 2-4x)."""
    net = _benign_net(22)
    bits, img, nchw = _positions()
    fast = FastPolicyNet(net, operands=operands)
    em = Emulated(net, operands, device="cuda")
    for planes in (bits[:300].contiguous(), img[:300].contiguous()):
        m = _full_metrics(fast, em, planes, nchw, operands)
        print(operands, "full network vs emulation:", m)
        for key, bound in FULL[operands].items():
            assert m[key] < bound, (operands, key, m[key], bound)


# Measured on MI355X (B = 1, 37): logits 0.059 (bf16) / 0.076 (f16) operand ulps of the accumulated magnitude (one-ulp differences of the rounded t), value 8e-9,
# softmax 2.3e-4 (bf16) / 3.0e-5 (f16) relative
HEADS_LOGIT_ULPS = 0.25
HEADS_SOFTMAX = {"bf16": 7e-4, "fp16": 1e-4}


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_fused_heads_on_the_kernels_tower_output(operands):
    """k_heads16_bf16 + k_value_head on one tower output (the kernel's own) against the emulated heads on the same values: logits element by element within
    HEADS_LOGIT_ULPS operand ulps of the accumulated magnitude sum |t w| + |b| (the kernel's t rounds on its own f32 sums: one-ulp flips against the emulation),
    value within 1e-6, softmax within HEADS_SOFTMAX relative."""
    net = _benign_net(23)
    bits, _, _ = _positions()
    fast = FastPolicyNet(net, operands=operands)
    em = Emulated(net, operands, device="cuda")
    for B in (1, 37, 300):
        planes = bits[:B].contiguous()
        with torch.no_grad():
            logits, v = (t.clone() for t in fast(planes, inference=False))
            pi, vi = (t.clone() for t in fast(planes, inference=True))
            y = _tower_vals(fast, planes, operands)
            l64, v64 = em.heads(y)
            pi64, _ = em.heads(y, inference=True)
            t = round_to(torch.relu(torch.nn.functional.conv2d(y, em.p1[0], em.p1[1])), operands)
            mag = torch.flatten(torch.nn.functional.conv2d(t, em.wp2.abs()), 1) + em.bp2.abs().repeat_interleave(64)
        ulp = ((logits.double() - l64).abs() / (mag * 2.0 ** -(8 if operands == "bf16" else 11))).max()      # in operand ulps of the accumulated magnitude
        dv = float((v.double().view(-1) - v64.view(-1)).abs().max())
        dpi = float(((pi.double() - pi64).abs() / pi64).max())
        print("%s heads B=%d: logits %.4f operand ulps of the accumulated magnitude, value %.2e, softmax rel %.2e" % (operands, B, float(ulp), dv, dpi))
        assert float(ulp) < HEADS_LOGIT_ULPS and dv < 1e-6 and dpi < HEADS_SOFTMAX[operands], (operands, B, float(ulp), dv, dpi)
        assert torch.equal(vi, v)


# ---- teeth: the same metrics against plausible bugs, injected into the reference -----------------------------------------------------------------------
class _Mutant(Emulated):
    def __init__(self, net, operands, bug, n_blocks=None):
        super().__init__(net, operands, n_blocks=n_blocks, device="cuda")
        self.bug = bug
        if bug == "bias_bf16":                                                 # one bias rounded to bf16 (block 0, conv1)
            w1, b1, w2, b2 = self.blocks[0]
            self.blocks[0] = (w1, round_to(b1, "bf16"), w2, b2)
        if bug == "kstep":                                                     # one stale / missing weight k-step: the last block's conv2, centre tap, input channels 64..95
            w1, b1, w2, b2 = self.blocks[-1]
            w2 = w2.clone(); w2[:, 64:96, 1, 1] = 0
            self.blocks[-1] = (w1, b1, w2, b2)
        if bug == "bf16_pack":                                                 # the f16 path's weights packed as bf16
            for i, (w1, b1, w2, b2) in enumerate(self.blocks):
                self.blocks[i] = (round_to(w1, "bf16"), b1, round_to(w2, "bf16"), b2)
            self.stem = (round_to(self.stem[0], "bf16"), self.stem[1])

    def conv(self, x, w, b):
        y = torch.nn.functional.conv2d(x, w, b, padding=1)
        if self.bug == "edge_tap" and w.shape[1] == 256:                       # tap (row 0, col -1) skipped on the right-edge squares of every 256-channel 3x3 conv
            w_tap = torch.zeros_like(w); w_tap[:, :, 1, 0] = w[:, :, 1, 0]
            y[..., 7] -= torch.nn.functional.conv2d(x, w_tap, None, padding=1)[..., 7]
        return y

    def tower(self, planes):
        x = planes.to(self.dev).double()
        w, b = self.stem
        x = self.r(torch.relu(self.conv(x, w, b)))
        for w1, b1, w2, b2 in self.blocks:
            t = self.r(torch.relu(self.conv(x, w1, b1)))
            c = self.conv(t, w2, b2)
            x = torch.relu(self.r(self.r(c) + x)) if self.bug == "round_before_residual" else torch.relu(self.r(c + x))
        return x


def test_bounds_have_teeth():
    """each plausible bug, injected on the reference side (symmetric to the kernel carrying it), fails the element bounds the kernels pass (MIN_IDENTICAL /
    MAX_EXCESS) on a truncated tower (k = 2 blocks) of 300 real positions.  The stale k-step sits in the last block of that tower: at k = 8 the unmutated
    emulation itself falls outside the element bounds (worst board 0.67 identical, excess 9e-3), and in the full network a stale k-step in block 7 moves the
    tower by 1.5e-2 against a bound of 1.6e-2 — the element check is the one that separates it.  The full-network metrics of every bug are printed next to FULL,
    not asserted."""
    net = _benign_net(24)
    bits, _, nchw = _positions()
    planes = bits[:300].contiguous()
    rows = []
    full = {op: (FastPolicyNet(net, operands=op), _full_metrics(FastPolicyNet(net, operands=op), Emulated(net, op, device="cuda"), planes, nchw, op)) for op in ("bf16", "fp16")}
    for operands, bug in (("bf16", "round_before_residual"), ("fp16", "round_before_residual"), ("bf16", "bias_bf16"), ("fp16", "bias_bf16"),
                          ("bf16", "edge_tap"), ("fp16", "edge_tap"), ("fp16", "bf16_pack"), ("bf16", "kstep"), ("fp16", "kstep")):
        k = 2
        tnet = truncated(net, k)
        fast = FastPolicyNet(tnet, operands=operands)
        with torch.no_grad():
            got = _tower_bits(fast, planes, operands)
            _, ident, ex = _ulps(got, _ref_bits(_Mutant(tnet, operands, bug).tower(nchw[:300]), operands), operands)
        fm = _full_metrics(full[operands][0], _Mutant(net, operands, bug), planes, nchw, operands)
        caught = [key for key in ("tower", "logits", "value") if fm[key] > FULL[operands][key]]
        rows.append((operands, bug, "k=%d identical / excess %.4f / %.1e" % (k, ident, ex), "full tower %.1e logits %.1e value %.1e -> %s"
                     % (fm["tower"], fm["logits"], fm["value"], ",".join(caught) or "-")))
        assert ident < MIN_IDENTICAL[operands] or ex > MAX_EXCESS[operands], (operands, bug, ident, ex)
    print("unmutated full network: bf16 %s, fp16 %s" % (full["bf16"][1], full["fp16"][1]))
    print("\n".join("%-5s %-22s %-40s %s" % r for r in rows))


# ---- trained regime -----------------------------------------------------------------------------------------------------------------------------------------
def _regime_net(seed):
    torch.manual_seed(seed)
    net = sz.policyNN({}).cuda().eval()
    trained_regime(net, seed)
    return net


# full network in the trained regime against the emulation.  Measured on MI355X: bf16 tower 7.2e-4, logits 1.7e-3, value 3.2e-3 (the value's absolute error grows
# with the O(1000) activations); f16 1.0e-4, 2.2e-4, 4.6e-4
REGIME_FULL = {"bf16": {"tower": 2.5e-3, "logits": 5e-3, "value": 1e-2}, "fp16": {"tower": 4e-4, "logits": 7e-4, "value": 1.5e-3}}


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_trained_regime_fast_network(operands):
    """FastPolicyNet on a network with trained-looking statistics (folded stem weights O(100), activations O(1000), weights down to f16's subnormals): the
    truncated towers within the MIN_IDENTICAL / MAX_EXCESS bounds and the full network within the REGIME_FULL bounds of the emulation (measured values there), all
    outputs finite."""
    net = _regime_net(31)
    bits, img, nchw = _positions()
    n = _n_cu()
    for k in (0, 1, 2):
        tnet = truncated(net, k)
        fast = FastPolicyNet(tnet, operands=operands)
        with torch.no_grad():
            ref = _ref_bits(Emulated(tnet, operands, device="cuda").tower(nchw), operands)
        for B in (1, n + 1, max(_batches())):
            for planes in (bits, img):
                got = _tower_bits(fast, planes[:B].contiguous(), operands)
                mu, ident, ex = _ulps(got, ref[:B], operands)
                print("%s trained regime k=%d B=%d: max ulp %d, identical %.6f, excess %.2e" % (operands, k, B, mu, ident, ex))
                assert ident >= MIN_IDENTICAL[operands] and ex <= MAX_EXCESS[operands], (operands, k, B, mu, ident, ex)
    fast = FastPolicyNet(net, operands=operands)
    m = _full_metrics(fast, Emulated(net, operands, device="cuda"), bits[:300].contiguous(), nchw, operands)
    print(operands, "trained regime, full network vs emulation:", m)
    with torch.no_grad():
        p, v = fast(bits[:300].contiguous(), inference=True)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all())
    for key, bound in REGIME_FULL[operands].items():
        assert m[key] < bound, (operands, key, m[key], bound)


def test_trained_regime_split_network():
    """SplitPolicyNet bf16 (hi + lo bf16: f32's range) against fp64 at the bounds of test_gpu_network.py (tower and centred logits 5e-5 relative L2; value 5e-5, as
    the value's absolute error grows with the O(1000) activations — measured 1.6e-5);
    SplitPolicyNet fp16 packs weights times 2^10 into f16: folded weights of O(100) do not fit, and construction says so."""
    net = _regime_net(32)
    bits, img, nchw = _positions()
    em = Emulated(net, None, device="cuda")
    split = SplitPolicyNet(net)
    for B in (1, 37, 300):
        with torch.no_grad():
            p, v = (t.clone() for t in split(bits[:B].contiguous(), inference=False))
            y = split.tower(img[:B].contiguous()).clone().view(B, 8, 8, 256).permute(0, 3, 1, 2)
            y64 = em.tower(nchw[:B])
            p64, v64 = em.heads(y64)
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all())
        m = (rel(y, y64), rel(cen(p), cen(p64)), float((v.double().view(-1) - v64.view(-1)).abs().max()))
        print("split bf16x2, trained regime, B=%d: tower %.2e logits %.2e value %.2e" % ((B,) + m))
        assert m[0] < 5e-5 and m[1] < 5e-5 and m[2] < 5e-5, (B, m)          # value: 1.6e-5 measured at B = 1 (activations O(1000)); 1e-5 at benign statistics
    with pytest.raises(ValueError, match="f16"):
        SplitPolicyNet(net, operands="fp16")


def test_number_format_range_is_checked_at_construction():
    """a folded weight beyond what a path's operand format holds is refused when the net is built, never returned as inf / NaN or a finite wrong answer:
    f16 operands hold |w| <= 65504; split f16 packs w * 2^10, so |w| < 2^16 / 2^10 - (half an f16 quantum); bf16 / split bf16 have f32's range"""
    torch.manual_seed(0)
    net = sz.policyNN({}).cuda().eval()
    with torch.no_grad():
        net.norm_layer.running_var[3] = 1e-5                                     # folded scale ~ 1 / sqrt(2e-5) = 224
        net.conv1.weight[3, 113] = 100.0                                          # -> folded 2.2e4: fits f16, not f16 * 2^10
    FastPolicyNet(net, operands="fp16"); FastPolicyNet(net); SplitPolicyNet(net)
    with pytest.raises(ValueError, match="f16"):
        SplitPolicyNet(net, operands="fp16")
    with torch.no_grad():
        net.resnet_blocks[4].conv2.weight[7, 9, 1, 1] = 1e5                       # folded ~1e5 > 65504
    with pytest.raises(ValueError, match="f16"):
        FastPolicyNet(net, operands="fp16")
    FastPolicyNet(net); SplitPolicyNet(net)
