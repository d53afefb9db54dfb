"""tests/trainref.py (the fp64 emulation of the train step's split-precision convolution kernels) held to plain fp64 on the CPU: the scale rule and the split from
their definitions, fp32's class on single-scale inputs, exact results on integer inputs, and the dynamic-range contract the f16 format implies — flat within 2^14
of a scaling unit's maximum, a relative error that doubles per octave below it."""
import math

import pytest
import torch

import trainref as T

B = 8


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_scale_rule():
    """k = 11 - exponent(max), clamped to +-100; 0 for zero, subnormal and non-finite maxima; the scaled maximum lands in [2^11, 2^12)"""
    a = torch.tensor([1.0, 1.99999, 2.0, 4.0, 3.0, 2.0 ** 11, 4095.0, 4096.0, 2.0 ** -40, 1e-7, 1e3, 0.0, float("inf"), float("nan"), 1e-45, 2.0 ** -126, 2.0 ** -120, 2.0 ** 120])
    k = T.scale_exp(a)
    assert k.tolist() == [11, 11, 10, 9, 10, 0, 0, -1, 51, 35, 2, 0, 0, 0, 0, 100, 100, -100]
    g = torch.Generator().manual_seed(0)
    m = torch.exp(torch.rand(1000, generator=g) * 120 - 60).float()
    s = m.double() * torch.ldexp(torch.ones(1000, dtype=torch.float64), T.scale_exp(m))
    assert bool(((s >= 2.0 ** 11) & (s < 2.0 ** 12)).all())
    assert T.amax_bits(torch.tensor([[-3.5, 1.0], [0.25, 2.0]])) == 0x40600000


def test_split_is_hi_plus_lo_from_the_format():
    """hi is the nearest f16 (ties to even), lo the nearest f16 to the f32 residual; over the contract's three regimes the representation error is what RANGE says:
    2^-22 relative down to 2^-3 (2^14 below a maximum of 2^11), 2^-25 absolute below, and everything at or under 2^-25 is flushed to zero"""
    s = torch.tensor([2049.0, 2051.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3000.123])
    hi, lo = T.split(s)
    assert hi.tolist()[:6] == [2048.0, 2052.0, 1.0, 1.0 + 2.0 ** -9, 2.0 ** -24, 0.0]
    assert lo.tolist()[:6] == [1.0, -1.0, 2.0 ** -11, -(2.0 ** -11), 0.0, 0.0]
    assert hi[6] + lo[6] == 2.0 ** -24
    g = torch.Generator().manual_seed(1)
    for e in range(11, -40, -1):
        v = ((1 + torch.rand(4096, generator=g)) * 2.0 ** e).float()
        hi, lo = T.split(v)
        err = (hi + lo - v.double()).abs()
        octaves = 11 - e                                       # below a unit maximum of 2^11
        if octaves <= T.RANGE["full"]:
            assert float((err / v.double()).max()) <= 2.0 ** -22, e
        else:
            assert float(err.max()) <= 2.0 ** -25, e
        if octaves > T.RANGE["zero"]:
            assert float((hi + lo).abs().max()) == 0.0, e
        elif octaves <= T.RANGE["hi_only"]:
            assert float((err / v.double()).max()) <= 2.0 ** -11, e


def _gauss(seed):
    return T.gauss_case(B, seed)


def test_single_scale_inputs_stay_in_the_22_bit_class():
    """on inputs of one scale (every element within 2^14 of its unit's maximum, but for values too small to matter) the emulation is within 2^-21 relative L2 of
    plain fp64 in all three directions — per product the two operands' representation errors (2^-23 each) and the dropped lo * lo term (2^-22) add up to 2^-21 at
    worst, and errors add over a sum no faster than the terms do — at inputs of 1, 1e3 and 1e-7 alike (the scaling is exact); and it is not plain fp64 (> 2^-28)."""
    x, gy, w = _gauss(0)
    xd, gd, wd = x.double(), gy.double(), w.double()
    ref = (T.conv64(xd, wd), T.conv64(gd, wd.transpose(0, 1).flip(2, 3)), T.wgrad64(gd, xd))
    for mag in (1.0, 1e3, 1e-7):
        m = float(torch.tensor(mag).float())
        got = (T.conv3x3_split(x * m, w), T.conv3x3_split(gy * m, w, transposed=True), T.wgrad_split(gy * m, x))
        r = [rel(a, b * m) for a, b in zip(got, ref)]
        print("inputs x %g: emulation vs fp64, forward %.2e, input gradient %.2e, weight gradient %.2e" % ((mag,) + tuple(r)))
        assert all(2.0 ** -28 < v < 2.0 ** -21 for v in r), (mag, r)


def range_table():
    """the weight-gradient emulation on gy rows scaled per output channel 2^0 .. 2^-31 (8 channels per octave), x at one scale: [(octave, rel L2 of those dw rows
    from fp64, the same for an fp32 evaluation)], and the whole tensor's rel L2"""
    x, gy, _ = _gauss(2)
    octs = torch.arange(256) // 8
    gy = gy * torch.ldexp(torch.ones(256), -octs).view(1, 256, 1, 1)
    ref = T.wgrad64(gy.double(), x.double())
    em = T.wgrad_split(gy, x)
    f32 = T.wgrad64(gy, x)
    rows = [(o, rel(em[octs == o], ref[octs == o]), rel(f32[octs == o], ref[octs == o])) for o in range(32)]
    return rows, rel(em, ref)


def test_range_contract_of_the_weight_gradient():
    """one scale per TENSOR: dw rows whose gy is within 2^12 of the loudest row (their elements, up to 2^2.3 below their row's largest, within 2^14 of the maximum) all
    have the same 22-bit error; from 2^16 below, every element's lo part is a multiple of 2^-24, the absolute error is constant and the row's relative error
    doubles with every octave; fp32 has the same error in every row; and the whole-tensor figure sees none of it."""
    rows, whole = range_table()
    print("octave below the maximum: emulation vs fp64 | fp32 vs fp64")
    print("\n".join("  2^-%-2d  %.2e  %.2e" % r for r in rows))
    print("whole tensor %.2e" % whole)
    err = {o: e for o, e, _ in rows}
    flat = [err[o] for o in range(0, 11)]
    assert max(flat) < 2.0 ** -21 and max(flat) / min(flat) < 1.25, flat
    assert whole < 2.0 ** -21
    for o in range(16, 31):
        assert 1.8 < err[o + 1] / err[o] < 2.2, (o, err[o], err[o + 1])
    assert abs(math.log2(err[31] / err[16]) - 15) < 0.5
    f32 = [e for _, _, e in rows]
    assert max(f32) / min(f32) < 1.25 and max(f32) < 2.0 ** -21
    assert err[31] > 1e4 * f32[31]                            # what the per-row reduction is for


@pytest.mark.parametrize("case", ["dense", "zero_board", "one_hot_taps", "tile_pairs"])
def test_exact_integer_inputs_come_out_exactly(case):
    """x, gy integer-valued in [-4, 4], w in [-2, 2]: every scaled operand is an f16 (lo = 0), so the emulation must EQUAL fp64 in every element"""
    x, gy, w = T.integer_case(B, 3, zero_board=2 if case == "zero_board" else None)
    ws = [w]
    if case == "one_hot_taps":
        ws = []
        for t in range(9):
            wt = torch.zeros_like(w); wt[:, :, t // 3, t % 3] = w[:, :, t // 3, t % 3]; ws.append(wt)
    if case == "tile_pairs":
        ws = []
        for ci, co in ((0, 0), (15, 15), (0, 15), (7, 3)):
            wt = torch.zeros_like(w); wt[16 * co:16 * co + 16, 16 * ci:16 * ci + 16] = w[16 * co:16 * co + 16, 16 * ci:16 * ci + 16]; ws.append(wt)
    xd, gd = x.double(), gy.double()
    assert torch.equal(T.wgrad_split(gy, x), T.wgrad64(gd, xd))
    for wt in ws:
        wd = wt.double()
        assert torch.equal(T.conv3x3_split(x, wt), T.conv64(xd, wd))
        assert torch.equal(T.conv3x3_split(gy, wt, transposed=True), T.conv64(gd, wd.transpose(0, 1).flip(2, 3)))
    if case == "zero_board":
        assert float(T.conv3x3_split(x, w)[2].abs().max()) == 0.0


def test_backward_data_and_weight_gradient_are_the_gradients():
    """the transposed + flipped convolution and wgrad64 are autograd's gradients of conv64 (fp64, 1e-13)"""
    x, gy, w = _gauss(4)
    xd, wd = x[:2].double().requires_grad_(), w.double().requires_grad_()
    torch.nn.functional.conv2d(xd, wd, padding=1).backward(gy[:2].double())
    assert rel(T.conv64(gy[:2].double(), wd.detach().transpose(0, 1).flip(2, 3)), xd.grad) < 1e-13
    assert rel(T.wgrad64(gy[:2].double(), xd.detach()), wd.grad) < 1e-13


def test_every_bug_moves_the_emulation():
    """each injected bug changes the rows it touches by far more than f32 accumulation could (1e-6), on the inputs where it can show"""
    x, gy, w = _gauss(5)
    y = T.conv3x3_split(x, w)
    r = rel(T.conv3x3_split(x, w, bug="drop_x_lo_tile"), y)
    assert 1e-5 < r < 1e-3, r
    yb = T.conv3x3_split(x, w, bug="board_scale_octave", board=3)
    assert torch.equal(yb[3] * 2, y[3]) and torch.equal(yb[:3], y[:3])
    assert rel(T.conv3x3_split(x, w, bug="tap_shift"), y) > 0.1
    dw = T.wgrad_split(gy, x)
    d = T.wgrad_split(gy, x, bug="drop_x_lo_tile", tile=2)
    assert 1e-5 < rel(d[:, 32:48], dw[:, 32:48]) < 1e-3 and torch.equal(d[:, :32], dw[:, :32])
    assert rel(T.wgrad_split(gy, x, bug="tap_shift")[:, :, 0, 0], dw[:, :, 0, 0]) > 0.1
    assert torch.equal(T.wgrad_split(gy, x, bug="wrong_tensor_scale"), dw)                 # same exponent: no difference; it needs tensors of different magnitudes
    r = rel(T.wgrad_split(gy * 2.0 ** -16, x, bug="wrong_tensor_scale"), dw * 2.0 ** -16)          # x times gy's scale leaves f16's range: inf, then NaN
    assert not r <= 1e-5, r


def test_bn_act_ref_is_torch_batchnorm_in_double():
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(3, 16, 8, 8, generator=g, dtype=torch.float64) * 1.7 + 0.3).requires_grad_()
    res = torch.randn(3, 16, 8, 8, generator=g, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(16).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(-0.5, 1.5, 16)); bn.bias.copy_(torch.linspace(-0.3, 0.3, 16)); bn.running_mean.fill_(0.1); bn.running_var.fill_(0.8)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    y, rm2, rv2 = T.bn_act_ref(x, bn.weight, bn.bias, res, rm, rv, bn.momentum, bn.eps)
    yt = torch.relu(bn(x) + res)
    assert rel(y.detach(), yt.detach()) < 1e-14 and rel(rm2, bn.running_mean) < 1e-14 and rel(rv2, bn.running_var) < 1e-14
