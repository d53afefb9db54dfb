"""The train step's kernels (trainconv.SplitConv3x3, BNAct, ConvBNAct: k_conv3x3_split_f32, k_wgrad3x3_split + k_wgrad_reduce, k_bn_act_fwd / _bwd) held row by
row: every quantity is reduced per scaling unit (board) and per row (output channel, dw row, dw column, BatchNorm channel), never over a whole tensor — a
whole-tensor relative L2 cannot see anything confined to a small-magnitude part.  Three yardsticks:
  exact     integer-valued inputs on which every operand is an f16 and every partial sum an f32: the kernels must EQUAL fp64 in every element;
  emulation tests/trainref.py, the kernels' own stated arithmetic in fp64: the kernels differ from it by f32 accumulation alone, at ANY magnitude
            (EMU_CONV / EMU_WGRAD: 4 x the worst distance measured on an MI355X over all cases of this file; profiles/trainconv_rows.txt);
  fp64      inside the range contract (trainconv.py's docstring): the bounds the suite already uses, 2e-6 per convolution and max(3 x torch fp32's error, 3e-7).
Outside the contract the loss against fp64 is by design (one scale per tensor in the weight gradient); it is printed, not asserted."""
import functools
import os

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd import train_rl
from sigma_zero_amd import trainconv as TC
from sigma_zero_amd.trainconv import BNAct, SplitConv3x3

import trainref as T
from nnref import trained_regime

pytestmark = pytest.mark.gpu

# kernel vs emulation, relative L2 per line (board x output channel for the convolutions, dw row / dw column for the weight gradient): 4 x the worst value
# measured on an MI355X (256 CUs) over every case of this file (profiles/trainconv_rows.txt) — convolution 1.07e-6 (261 boards of mixed magnitude, forward),
# weight gradient 9.54e-7 (a site of the trained-regime step; 5.35e-7 at 261 boards) and, for lines deeper than DEEP_OCTAVES under their tensor's maximum,
# 3.21e-5 (261 boards, columns 2^30 down).  Down to 2^24 the distance does not depend on the depth (3.2e-7 .. 3.9e-7 at 261 boards); from 2^26 on, where
# the hi parts themselves are f16 subnormals, it triples per octave and grows with the number of boards (1.3e-6 / 1.1e-5 / 3.2e-5 at 3 / 37 / 261 boards, 2^30
# down): the matrix cores do not add the products of subnormal operands like f32.  It stays two to three orders under what such a line has lost against fp64.
EMU_CONV = 4.3e-6
EMU_WGRAD = 3.8e-6
EMU_WGRAD_DEEP = 1.3e-4
DEEP_OCTAVES = 20
CONTRACT_OCTAVES = 12                                      # a row whose scale is within 2^12 of the loudest is inside the range contract

_BATCH = {"n/2": lambda n: n // 2, "n/2+1": lambda n: n // 2 + 1, "n+5": lambda n: n + 5}
BATCHES = ["1", "2", "17", "n/2", "n/2+1", "n+5"]


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _batch(name):
    return _BATCH[name](_n_cu()) if name in _BATCH else int(name)


def _run(x, gy, w, want_gx=True):
    """SplitConv3x3 forward + backward: (y, gx or None, gw)"""
    xx, ww = x.clone().requires_grad_(want_gx), w.clone().requires_grad_(True)
    y = SplitConv3x3.apply(xx, ww)
    y.backward(gy)
    return y.detach(), xx.grad, ww.grad


def _wt(w):
    return w.transpose(0, 1).flip(2, 3).contiguous()


def _emu(fails, dist, bound, what):
    """kernel-vs-emulation line distances against their bound (a number or one per line): misses are appended to `fails`; returns the worst distance"""
    bad = ~(dist <= bound)
    if bool(bad.any()):
        fails.append((what, float(dist[bad].max()), int(bad.sum()), bad.nonzero()[:4].tolist()))
    return float(dist.max())


def _depth(t):
    """octaves of each channel's max |t| under the tensor's (inf for an all-zero channel)"""
    m = t.abs().amax(dim=(0, 2, 3)).double()
    return torch.log2(m.max() / m)


def _wgrad_emu(fails, gw, em, gy, x, what):
    """every dw row and column against the emulation, each under the bound of its depth; returns (worst line down to DEEP_OCTAVES, worst deeper line)"""
    worst = [0.0, 0.0]
    for dims, depth, name in (((1, 2, 3), _depth(gy), "rows"), ((0, 2, 3), _depth(x), "columns")):
        d = T.line_rel(gw, em, dims)
        deep = depth > DEEP_OCTAVES
        _emu(fails, d, torch.where(deep, EMU_WGRAD_DEEP, EMU_WGRAD), (what, name))
        worst[0] = max(worst[0], float(d[~deep].max()))
        if bool(deep.any()):
            worst[1] = max(worst[1], float(d[deep].max()))
    return tuple(worst)


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
def test_exact_integer_cases(batch):
    """x, gy integer-valued in [-4, 4] with zero rows, columns and channel tiles, w integer-valued in [-2, 2]: forward, input gradient and weight gradient EQUAL
    the fp64 result in every element.  Why they must: a unit's maximum m in 1 .. 4 is scaled by 2^k, k = 11 - floor(log2 m), so every scaled element is j * 2^k
    with an integer |j| <= 4 — an f16, lo = 0; the weights times 2^10 are i * 2^10 with |i| <= 2, f16 too.  Convolution: a product is at most 8 units of
    2^(k + 10), a sum has at most 9 * 256 = 2304 of them: every partial sum, in any order, is an integer below 2^15 units — an f32 — and the unscaling is exact.
    Weight gradient: a product is at most 16 units of 2^(k_gy + k_x); a dw element sums B * 64 of them, over the board groups and then in the reduction:
    at most B * 1024 units, below 2^24 for every B < 16384 — B <= n + 5 = 261 on 256 CUs stays 2^5 under it — so partial sums, unscaling and reduction are exact.
    Cases per batch: dense; an all-zero board; one-hot weights for each of the 9 taps; one input-channel tile feeding one output-channel tile (first, last,
    first -> last, one inside).  Batches: 1, 2, 17 (sixteen board groups of the weight gradient, the last ones empty), n/2 and n/2 + 1 (the two-workgroups-per-
    board form ends at n/2), n + 5 (the persistent board loop)."""
    B = _batch(batch)
    x, gy, w = T.integer_case(B, 11, device="cuda")
    cases = [("dense", x, gy, w)]
    if B >= 2:
        xz, gz, _ = T.integer_case(B, 12, device="cuda", zero_board=B // 2)
        cases.append(("zero board", xz, gz, w))
    for t in range(9):
        wt = torch.zeros_like(w); wt[:, :, t // 3, t % 3] = w[:, :, t // 3, t % 3]
        cases.append(("tap %d" % t, x, gy, wt))
    for ci, co in ((0, 0), (15, 15), (0, 15), (7, 3)):
        wt = torch.zeros_like(w); wt[16 * co:16 * co + 16, 16 * ci:16 * ci + 16] = w[16 * co:16 * co + 16, 16 * ci:16 * ci + 16]
        cases.append(("tile %d -> %d" % (ci, co), x, gy, wt))
    gw64 = {}
    for name, xx, gg, ww in cases:
        y, gx, gw = _run(xx, gg, ww)
        xd, gd, wd = xx.double(), gg.double(), ww.double()
        if id(xx) not in gw64:
            gw64[id(xx)] = T.wgrad64(gd, xd)
        for what, got, ref in (("forward", y, T.conv64(xd, wd)), ("input gradient", gx, T.conv64(gd, _wt(wd))), ("weight gradient", gw, gw64[id(xx)])):
            bad = got.double() != ref
            assert not bool(bad.any()), (B, name, what, int(bad.sum()), bad.nonzero()[:4].tolist(), float((got.double() - ref).abs().max()))
        if name == "zero board":
            assert float(y[B // 2].abs().max()) == 0.0 and float(gx[B // 2].abs().max()) == 0.0


@pytest.mark.parametrize("batch", ["2", "n+5"])
def test_amax_word_through_the_c_abi(batch):
    """sz_nn_conv3x3_split_f32 leaves the bit pattern of max |x| over the whole tensor in amax_bits, exactly — the weight gradient's scale is read from it — with the
    maximum in the first, a middle or the last board, on a tensor of mixed board magnitudes, and 0 for an all-zero tensor"""
    B = _batch(batch)
    lib = N.lib()
    x, _, w = T.gauss_case(B, 21, device="cuda")
    stream_buf = torch.empty(72 * 2048 * 16, dtype=torch.uint8, device="cuda")
    zero = torch.zeros(256, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty_like(x)
    for where in (0, B // 2, B - 1, None):
        xs = x * T.octave_scales(B, -3, -40, device="cuda").view(-1, 1, 1, 1)
        if where is None:
            xs = torch.zeros_like(x)
        else:
            xs[where, 200, 7, 7] = -1.2345678
        N.check(lib.sz_nn_pack_conv_split_dev(w.data_ptr(), 0, 1, stream_buf.data_ptr(), word.data_ptr(), st), "pack")
        N.check(lib.sz_nn_conv3x3_split_f32(xs.data_ptr(), stream_buf.data_ptr(), zero.data_ptr(), y.data_ptr(), B, 1, word.data_ptr(), st), "conv")
        assert int(word.item()) == T.amax_bits(xs), (B, where, hex(int(word.item())), hex(T.amax_bits(xs)))


# ---- 3. mixed magnitudes inside one launch ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed(B):
    """one Gaussian case per batch size, shared (and left unchanged) by the tests below"""
    return T.gauss_case(B, 100 + B, device="cuda")


def _board_scales(B):
    """2^0 .. 2^-40 over the boards, board 1 all zero"""
    s = T.octave_scales(B, 0, -40, device="cuda")
    s[1] = 0
    return s.view(-1, 1, 1, 1)


@pytest.mark.parametrize("batch", ["3", "37", "n+5"])
def test_boards_of_mixed_magnitude(batch):
    """forward and backward-data on a batch whose boards are scaled 2^0 .. 2^-40 (one of them all zero): the scale is per board, so the faintest board is as close
    to fp64 as the loudest — relative L2 PER BOARD under the 2e-6 of test_gpu_round3.py — and every (board, output channel) line is within EMU_CONV of the
    emulation.  Then the input channels of every board are scaled 2^0 .. 2^-30 on top: per (board, output channel) against the emulation, per board against fp64
    (the sum over all input channels keeps the output in fp32's class: the faint channels' absolute error is 2^-36 of the board's maximum)."""
    B = _batch(batch)
    x, gy, w = _mixed(B)
    bs = _board_scales(B)
    cs = T.octave_scales(256, 0, -30, device="cuda").view(1, -1, 1, 1)
    wd = w.double()
    fails = []
    for name, xs, gs in (("boards", x * bs, gy * bs.flip(0).roll(2, 0)), ("boards x input channels", x * bs * cs, gy * bs * cs.flip(1))):
        y, gx, _ = _run(xs, gs, w)
        rec = []
        for what, got, inp, ww, tr in (("forward", y, xs, wd, False), ("input gradient", gx, gs, _wt(wd), True)):
            ref = T.conv64(inp.double(), ww)
            em = T.conv3x3_split(inp, w, transposed=tr)
            zero = inp.abs().amax(dim=(1, 2, 3)) == 0
            assert int(zero.sum()) == 1 and float(got[zero].abs().max()) == 0.0
            per_board = T.line_rel(got, ref, (1, 2, 3))
            assert float(per_board.max()) < 2e-6, (B, name, what, per_board.max(), int(per_board.argmax()))
            rec.append((what, float(per_board.max()), float(T.line_rel(em, ref, (1, 2, 3)).max()), _emu(fails, T.line_rel(got, em, (2, 3)), EMU_CONV, (B, name, what)),
                        float(T.line_rel(got, em, (1, 2, 3)).max())))
        print("\n".join("B %3d %-24s %-15s worst board vs fp64 %.2e (emulation %.2e); vs emulation: worst (board, channel) %.2e, worst board %.2e" % ((B, name) + r) for r in rec))
    assert not fails, fails


def _wgrad_lines(gw, ref, scaled_dim):
    """relative L2 per line of the scaled dimension (0: dw rows, 1: dw columns) and per line of the other one"""
    other = (0, 2, 3) if scaled_dim == 0 else (1, 2, 3)
    mine = (1, 2, 3) if scaled_dim == 0 else (0, 2, 3)
    return T.line_rel(gw, ref, mine), T.line_rel(gw, ref, other)


@pytest.mark.parametrize("scaled", ["gy per output channel", "x per input channel"])
@pytest.mark.parametrize("batch", ["3", "37", "n+5"])
def test_weight_gradient_rows_of_mixed_magnitude(batch, scaled):
    """the weight gradient with gy scaled per output channel (dw rows) or x per input channel (dw columns) 2^0 .. 2^-30, one scale per TENSOR in the kernel: every
    line of both dimensions is within EMU_WGRAD of the emulation at every scale; inside the contract (lines of the scaled dimension within 2^12 of the loudest, and
    every line of the other dimension — each holds all magnitudes and its error is the loud elements') the distance from fp64 is within
    max(3 x torch fp32's on the same line, 3e-7), the bound form of test_gpu_train_fp64.py.  Without a backward-data pass (max |gy| taken with torch) the result is
    the same, bit for bit.  The loss outside the contract is printed."""
    B = _batch(batch)
    x, gy, w = _mixed(B)
    dim = 0 if scaled.startswith("gy") else 1
    octs = torch.round(torch.linspace(0.0, 30.0, 256)).to(torch.int64).cuda()
    sc = T.octave_scales(256, 0, -30, device="cuda").view(1, -1, 1, 1)
    xs, gs = (x, gy * sc) if dim == 0 else (x * sc, gy)
    _, _, gw = _run(xs, gs, w)
    _, _, gw_alone = _run(xs, gs, w, want_gx=False)
    assert torch.equal(gw, gw_alone)
    ref = T.wgrad64(gs.double(), xs.double())
    em = T.wgrad_split(gs, xs)
    f32 = torch.nn.grad.conv2d_weight(xs, w.shape, gs, padding=1)
    k_mine, k_other = _wgrad_lines(gw, ref, dim)
    t_mine, t_other = _wgrad_lines(f32, ref, dim)
    e_mine, _ = _wgrad_lines(em, ref, dim)
    d_mine, _ = _wgrad_lines(gw, em, dim)
    fails = []
    worst = _wgrad_emu(fails, gw, em, gs, xs, (B, scaled))
    inside = octs <= CONTRACT_OCTAVES
    print("B %3d weight gradient, %s: vs emulation worst line %.2e, deeper than 2^-%d %.2e; inside the contract worst line vs fp64 %.2e (torch fp32 %.2e)" %
          (B, scaled, worst[0], DEEP_OCTAVES, worst[1], float(k_mine[inside].max()), float(t_mine[inside].max())))
    print("\n".join("    2^-%-2d  vs fp64: kernel %.2e  emulation %.2e  torch fp32 %.2e;  kernel vs emulation %.2e" %
                    (o, float(k_mine[octs == o].max()), float(e_mine[octs == o].max()), float(t_mine[octs == o].max()), float(d_mine[octs == o].max())) for o in range(0, 31)))
    assert not fails, fails
    bad = inside & ~(k_mine < torch.maximum(3 * t_mine, torch.full_like(t_mine, 3e-7)))
    assert not bool(bad.any()), (B, scaled, bad.nonzero().flatten().tolist(), k_mine[bad].tolist(), t_mine[bad].tolist())
    bad = ~(k_other < torch.maximum(3 * t_other, torch.full_like(t_other, 3e-7)))
    assert not bool(bad.any()), (B, scaled, "other dimension", bad.nonzero().flatten().tolist(), k_other[bad].tolist(), t_other[bad].tolist())


def test_range_table_on_the_device():
    """the table of tests/test_trainref.py's range test (gy rows scaled 2^0 .. 2^-31, eight dw rows per octave, 8 boards) from the kernel next to the emulation's:
    the kernel follows the emulation through the whole range (EMU_WGRAD per row) and, like it, is flat inside the contract and doubles per octave far outside"""
    x, gy, w = T.gauss_case(8, 2, device="cuda")
    octs = (torch.arange(256) // 8).cuda()
    gs = gy * torch.ldexp(torch.ones(256), -(torch.arange(256) // 8).to(torch.int32)).cuda().view(1, -1, 1, 1)
    _, _, gw = _run(x, gs, w)
    ref, em = T.wgrad64(gs.double(), x.double()), T.wgrad_split(gs, x)
    f32 = torch.nn.grad.conv2d_weight(x, w.shape, gs, padding=1)
    fails = []
    _wgrad_emu(fails, gw, em, gs, x, "range table")
    grp = lambda a, r, o: float((a.double() - r)[octs == o].norm() / r[octs == o].norm())
    rows = [(o, grp(gw, ref, o), grp(em, ref, o), grp(f32, ref, o), grp(gw, em, o)) for o in range(32)]
    print("octave below the maximum: kernel | emulation | torch fp32, rel L2 of the eight dw rows from fp64 | kernel from the emulation; whole tensor kernel vs fp64 %.2e"
          % float((gw.double() - ref).norm() / ref.norm()))
    print("\n".join("  2^-%-2d  %.2e  %.2e  %.2e  %.2e" % r for r in rows))
    assert not fails, fails
    k = {r[0]: r[1] for r in rows}
    assert all(r[1] < max(3 * r[3], 3e-7) for r in rows[:11]), rows[:11]
    for o in range(18, 31):
        assert 1.8 < k[o + 1] / k[o] < 2.2, (o, k[o], k[o + 1])


def test_emulation_bounds_have_teeth():
    """each plausible kernel bug, injected on the emulation's side (symmetric to the kernel carrying it), is further from the kernel than EMU_CONV / EMU_WGRAD on the
    lines it touches — and on no others where it touches only some: the w_hi * x_lo product dropped for one input-channel tile; one board (the faintest) unscaled
    an octave off; one tap read a column off; the weight gradient's tensor scales swapped (gy three octaves above x, so that nothing leaves f16's range; printed
    for it: the least ratio of distance to bound)."""
    B = 5
    x, gy, w = _mixed(B)
    xs = x * T.octave_scales(B, 0, -40, device="cuda").view(-1, 1, 1, 1)
    y, _, _ = _run(xs, gy, w)
    exceeds = lambda d, bound: ~(d <= bound)                    # NaN counts as exceeding
    rows = []
    for bug, kw in (("drop_x_lo_tile", {"tile": 3}), ("board_scale_octave", {"board": B - 1}), ("tap_shift", {"tap": (1, 0)})):
        d = T.line_rel(y, T.conv3x3_split(xs, w, bug=bug, **kw), (2, 3))
        hit = exceeds(d, EMU_CONV)
        touched = torch.zeros_like(hit)
        touched[B - 1 if bug == "board_scale_octave" else slice(None)] = True
        assert torch.equal(hit, touched), (bug, float(d[touched].min()), float(d[~touched].max()) if bool((~touched).any()) else None)
        rows.append(("convolution", bug, float(d[touched].min())))
    cs = T.octave_scales(256, 0, -30, device="cuda").view(1, -1, 1, 1)
    xc = x * cs                                                 # tile 4: input channels 64 .. 79, 2^-8 .. 2^-9 — inside the contract, 2^-17 of the tensor's energy
    col_bound = torch.where(_depth(xc) > DEEP_OCTAVES, EMU_WGRAD_DEEP, EMU_WGRAD)
    _, _, gw = _run(xc, gy, w)
    d = T.line_rel(gw, T.wgrad_split(gy, xc, bug="drop_x_lo_tile", tile=4), (0, 2, 3))
    touched = torch.zeros(256, dtype=torch.bool, device="cuda"); touched[64:80] = True
    assert torch.equal(exceeds(d, col_bound), touched), (float(d[touched].min()), float(d[~touched].max()))
    rows.append(("weight gradient", "drop_x_lo_tile", float(d[touched].min())))
    d = T.line_rel(gw, T.wgrad_split(gy, xc, bug="tap_shift", tap=(1, 0)), (1, 2, 3))
    assert bool(exceeds(d, EMU_WGRAD).all())
    rows.append(("weight gradient", "tap_shift", float(d.min())))
    # gy three octaves ABOVE x (k_gy = k_x - 3 exactly): with the scales swapped x lands three octaves lower — every column whose lo parts are multiples of 2^-24
    # (2^16 and more under the loudest) loses three bits — and gy's maximum in [2^14, 2^15): nothing leaves f16's range
    gq = gy * float(2.0 ** (3 - int(T.scale_exp(xc.abs().amax()) - T.scale_exp(gy.abs().amax()))))
    assert int(T.scale_exp(gq.abs().amax())) == int(T.scale_exp(xc.abs().amax())) - 3
    _, _, gw = _run(xc, gq, w)
    fails = []
    _wgrad_emu(fails, gw, T.wgrad_split(gq, xc), gq, xc, "gy three octaves above x")
    assert not fails, fails
    d = T.line_rel(gw, T.wgrad_split(gq, xc, bug="wrong_tensor_scale"), (0, 2, 3))
    faint = _depth(xc) >= 16
    assert bool(torch.isfinite(d).all()) and bool(exceeds(d[faint], col_bound[faint]).all()), (d[faint] / col_bound[faint]).min()
    rows.append(("weight gradient", "wrong_tensor_scale", float((d[faint] / col_bound[faint]).min())))
    print("\n".join("%-16s %-20s least distance on the lines it touches %.2e" % r for r in rows))


# ---- 4. BatchNorm + skip + ReLU, channel by channel ----------------------------------------------------------------------------------------------------------------
# (data, gamma, beta): data "normal" N(0.3, 1.7), "mean>>std" N(1e3, 1e-2), "var<<eps" N(0.5, 1e-4) (variance 1e-8 under eps = 1e-5), "const" 0.7 everywhere
BN_CHANNELS = [("normal", 1.0, 0.1), ("mean>>std", 1.0, 0.0), ("var<<eps", 1.0, 0.1), ("const", 1.0, 0.2), ("normal", 0.0, 0.1), ("normal", -1.0, 0.0),
               ("normal", 1e-6, 0.0), ("normal", 1e3, 0.0), ("normal", 0.1, -10.0), ("mean>>std", -1.0, 0.0), ("const", 1e3, 0.0), ("var<<eps", 1e3, 0.0)]
BN_DATA = {"normal": (0.3, 1.7), "mean>>std": (1e3, 1e-2), "var<<eps": (0.5, 1e-4), "const": (0.7, 0.0)}


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("B", [1, 3, 256, 257])
def test_batchnorm_skip_relu_channel_by_channel(B, with_res):
    """BNAct (k_bn_act_fwd / k_bn_act_bwd) on ONE tensor whose channels are BN_CHANNELS — mean >> std, variance << eps, a constant channel, gamma 0 / -1 / 1e-6 /
    1e3, a channel the ReLU kills (beta -10) — at 1, 3, 256 (the register cache BN_MAXV) and 257 boards, with and without the skip input: y, dx, dres, dgamma,
    dbeta, running_mean and running_var PER CHANNEL against the plain fp64 formulas (trainref.bn_act_ref), each next to torch fp32's (F.batch_norm) error on the
    same channel; the fp64 and fp32 twins get the device's ReLU mask y > 0.
    Error per channel: tensors, relative L2 over the channel; dgamma / dbeta (sums of signed terms), |difference| over max(|reference|, L2 norm of the summands) —
    the scale of such a sum and of its rounding error; running statistics, relative (momentum 0.5 on zeros: half the batch statistic, nothing hides it).
    Bound per channel: max(3 x torch's error, 3e-7 x (1 + |mean| / std)): x - mean keeps |x - mean| / |mean| of fp32's bits.  The constant channels (std = 0)
    are compared absolutely, against eps's scale: the reference's x - mean is 0, fp32's is a few ulps of the mean, and 1 / sqrt(eps) turns that into xhat — so
    cond = 1 + |mean| / sqrt(eps), y's error is taken over |gamma| * cond + max |y|, dgamma's over cond x the L2 norm of dy', running_var's over eps; the rest as above."""
    C_ = len(BN_CHANNELS)
    g = torch.Generator().manual_seed(40 + B)
    x = torch.stack([torch.randn(B, 8, 8, generator=g, dtype=torch.float64) * BN_DATA[d][1] + BN_DATA[d][0] for d, _, _ in BN_CHANNELS], 1).float().cuda().contiguous()
    gamma = torch.tensor([c[1] for c in BN_CHANNELS], dtype=torch.float32, device="cuda")
    beta = torch.tensor([c[2] for c in BN_CHANNELS], dtype=torch.float32, device="cuda")
    res = torch.randn(B, C_, 8, 8, generator=g).cuda() if with_res else None
    gy = torch.randn(B, C_, 8, 8, generator=g).cuda()
    eps, mom = 1e-5, 0.5
    out, mask = {}, None
    for kind in ("fused", "fp64", "torch"):
        dt = torch.float64 if kind == "fp64" else torch.float32
        xx, gg, bb = (t.to(dt).clone().requires_grad_(True) for t in (x, gamma, beta))
        rr = res.to(dt).clone().requires_grad_(True) if with_res else None
        rm, rv = torch.zeros(C_, dtype=dt, device="cuda"), torch.zeros(C_, dtype=dt, device="cuda")
        if kind == "fused":
            y = BNAct.apply(xx, gg, bb, rr, rm, rv, mom, eps)
            mask = (y.detach() > 0).double()
        elif kind == "fp64":
            y, rm, rv = T.bn_act_ref(xx, gg, bb, rr, rm, rv, mom, eps, mask=mask)
        else:
            pre = torch.nn.functional.batch_norm(xx, rm, rv, gg, bb, True, mom, eps)
            y = (pre if rr is None else pre + rr) * mask.float()
        y.backward(gy.to(dt))
        out[kind] = {"y": y.detach(), "dx": xx.grad, "dgamma": gg.grad, "dbeta": bb.grad, "running_mean": rm, "running_var": rv}
        if with_res:
            out[kind]["dres"] = rr.grad
    x64 = x.double()
    mean, std = x64.mean(dim=(0, 2, 3)), x64.std(dim=(0, 2, 3), unbiased=False)
    const = torch.tensor([c[0] == "const" for c in BN_CHANNELS], device="cuda")
    assert bool((std[const] == 0).all()) and bool((std[~const] > 0).all())
    cond = torch.where(const, 1 + mean.abs() / eps ** 0.5, 1 + mean.abs() / std.clamp_min(1e-300))
    dy = gy.double() * mask
    xhat = (x64 - mean.view(1, -1, 1, 1)) * torch.rsqrt(std * std + eps).view(1, -1, 1, 1)
    l2 = lambda t: t.pow(2).sum(dim=(0, 2, 3)).sqrt()
    ref = out["fp64"]
    lines = []
    for name in ref:
        r = ref[name].double()
        if r.dim() == 4:
            den = l2(r)
            if name == "y":
                den = torch.where(const, (gamma.double().abs() * cond + r.abs().amax(dim=(0, 2, 3))) * (B * 64) ** 0.5, den)
        elif name == "dgamma":
            den = torch.where(const, cond * l2(dy), torch.maximum(r.abs(), l2(dy * xhat)))
        elif name == "dbeta":
            den = torch.maximum(r.abs(), l2(dy))
        else:
            den = torch.where(const & (name == "running_var"), torch.full_like(r, eps), r.abs())
        err = {}
        for kind in ("fused", "torch"):
            a = out[kind][name].double()
            num = l2(a - r) if r.dim() == 4 else (a - r).abs()
            err[kind] = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))
        bound = torch.maximum(3 * err["torch"], torch.where(const, torch.full_like(cond, 3e-7), 3e-7 * cond))
        lines.append("  %-12s " % name + " ".join("%.1e/%.1e" % (float(a), float(b)) for a, b in zip(err["fused"], err["torch"])))
        bad = ~(err["fused"] <= bound)
        assert not bool(bad.any()), (B, with_res, name, [(BN_CHANNELS[i], float(err["fused"][i]), float(err["torch"][i]), float(bound[i])) for i in bad.nonzero().flatten().tolist()])
    print("BNAct B %d %s: error per channel, fused / torch fp32 (channels: %s)" % (B, "residual" if with_res else "plain", ", ".join("%s g=%g" % c[:2] for c in BN_CHANNELS)))
    print("\n".join(lines))
    dead = [i for i, c in enumerate(BN_CHANNELS) if c[2] == -10.0]
    assert float(out["fused"]["y"][:, dead].abs().max()) == 0.0 and float(out["fused"]["dx"][:, dead].abs().max()) == 0.0


# ---- 5. one step in the trained regime: a record ------------------------------------------------------------------------------------------------------------------
def test_trained_regime_step_record(golden_dir):
    """one train step (golden 8-sample batch) of a network with nnref.trained_regime statistics (gamma over 1e-3 .. 3, some exactly zero, dead channels), every
    tower site run as SplitConv3x3 + BNAct (trainconv._conv_bn_act wrapped, as test_gpu_train_fp64.py does; the same kernels as ConvBNAct) so that the
    convolution's input x and output gradient gt can be kept: per site the octave span of the per-channel max |x| and max |gt|, the share of dw rows / columns
    outside the contract (more than 2^12 under the loudest; all-zero lines counted apart), and the worst dw row's distance from fp64 inside and outside it.
    A measurement: asserted only against the emulation (every row and column of every site within EMU_WGRAD)."""
    z = np.load(os.path.join(golden_dir, "train_loss_golden.npz"))
    batch = {"states": torch.from_numpy(z["x"].astype(np.float32)), "actions": torch.from_numpy(z["p_target"]), "rewards": torch.from_numpy(z["v_target"])}
    torch.manual_seed(0)
    net = trained_regime(sz.policyNN({}), 7, verbose=False).cuda().train()
    sites, orig = [], TC._conv_bn_act

    def wrapped(conv, bn, x, residual=None):
        t = SplitConv3x3.apply(x, conv.weight)
        site = {"x": x.detach(), "conv": conv}
        t.register_hook(lambda gt, site=site: site.__setitem__("gt", gt.detach().clone()))
        sites.append(site)
        return TC._bn_act(bn, t, residual)
    TC._conv_bn_act = wrapped
    try:
        with TC.split_convs(net):
            b = {k: v.cuda() for k, v in batch.items()}
            net.zero_grad()
            loss, _, _ = train_rl.loss_fn(net, b, "cuda")
            loss.backward()
    finally:
        TC._conv_bn_act = orig
    assert len(sites) == 38
    span = lambda m: float(torch.log2(m[m > 0].max() / m[m > 0].min())) if bool((m > 0).any()) else 0.0
    print("site: octave span of per-channel max|x|, max|gt|; zero rows/columns; rows, columns outside the contract; worst dw row vs fp64 inside | outside; worst line vs emulation")
    tot_out, tot, fails = 0, 0, []
    for i, s in enumerate(sites):
        x, gt, gw = s["x"], s["gt"], s["conv"].weight.grad
        mx, mg = x.abs().amax(dim=(0, 2, 3)), gt.abs().amax(dim=(0, 2, 3))
        ref, em = T.wgrad64(gt.double(), x.double()), T.wgrad_split(gt, x)
        worst = max(_wgrad_emu(fails, gw, em, gt, x, ("site", i)))
        rows = T.line_rel(gw, ref, (1, 2, 3))
        out_r, out_c = (mg > 0) & (mg < mg.max() * 2.0 ** -CONTRACT_OCTAVES), (mx > 0) & (mx < mx.max() * 2.0 ** -CONTRACT_OCTAVES)
        in_r = (mg > 0) & ~out_r
        tot_out += int(out_r.sum()) + int(out_c.sum()); tot += 512
        print("  %2d  x %4.1f  gt %4.1f  zero %3d/%3d  outside %3d/%3d  dw row vs fp64 %.2e | %s  vs emulation %.2e"
              % (i, span(mx), span(mg), int((mg == 0).sum()), int((mx == 0).sum()), int(out_r.sum()), int(out_c.sum()), float(rows[in_r].max()) if bool(in_r.any()) else 0.0,
                 "%.2e" % float(rows[out_r].max()) if bool(out_r.any()) else "   -    ", worst))
    print("lines outside the contract: %d of %d" % (tot_out, tot))
    assert not fails, fails
