"""tests/nnref.py — the fp64 emulation of FastPolicyNet's rounding points — held against policyNN, torch's conversions and the native weight packers (CPU only)."""
import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd.fastnet import _fold_bn, _pack

from nnref import Emulated, folded_convs, round_to, trained_regime, truncated


def _net(seed=0, regime=False):
    torch.manual_seed(seed)
    net = sz.policyNN({}).eval()
    if regime:
        trained_regime(net, seed, verbose=False)
    else:
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.normal_(0, 0.05); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.7, 1.3); m.bias.normal_(0, 0.05)
    return net


@pytest.mark.parametrize("regime", [False, True], ids=["benign", "trained"])
def test_emulation_without_rounding_is_policynn_in_double(regime):
    net = _net(1, regime)
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(3, 119, 8, 8, generator=g) < 0.15).double()
    x[2] = 0                                                                  # an all-zero board
    net64 = truncated(net, 19).double()
    with torch.no_grad():
        p64, v64 = net64(x, inference=False)
        y64 = net64.resnet_blocks(torch.relu(net64.norm_layer(net64.conv1(x))))
        em = Emulated(net, None)
        y = em.tower(x)
        p, v = em.heads(y)
        pi, _ = em(x, inference=True)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(y, y64) < 1e-12 and rel(p, p64) < 1e-12 and float((v - v64).abs().max()) < 1e-12, (rel(y, y64), rel(p, p64))
    assert float((pi - torch.softmax(p64, 1)).abs().max()) < 1e-12
    # truncation: n_blocks = k is the network with resnet_blocks[:k]
    t2 = truncated(net, 2).double()
    with torch.no_grad():
        assert rel(Emulated(net, None, n_blocks=2).tower(x), t2.resnet_blocks(torch.relu(t2.norm_layer(t2.conv1(x))))) < 1e-12


@pytest.mark.parametrize("operands,dtype", [("bf16", torch.bfloat16), ("fp16", torch.float16)])
def test_rounding_is_torch_conversion_bit_for_bit(operands, dtype):
    """every f32 exponent, random mantissas, exact ties, subnormals of the target, the overflow boundary"""
    rng = np.random.RandomState(0)
    bits = rng.randint(0, 2 ** 31, size=400000).astype(np.uint32) | (rng.randint(0, 2, size=400000).astype(np.uint32) << 31)
    x = torch.from_numpy(bits.view(np.float32).copy())
    x = x[torch.isfinite(x)]
    keep = 8 if operands == "bf16" else 11
    ties = torch.from_numpy(((bits & ~np.uint32((1 << (24 - keep)) - 1)) | np.uint32(1 << (23 - keep))).view(np.float32).copy())          # exactly half a quantum above a value
    ties = ties[torch.isfinite(ties)]
    sub = torch.ldexp(torch.arange(-3000, 3000, dtype=torch.float32), torch.tensor(-26 if operands == "fp16" else -135))                     # around the target's subnormal range
    fmax = torch.finfo(dtype).max
    edge = torch.tensor([fmax, -fmax, np.nextafter(np.float32(fmax), np.float32(np.inf)), fmax * (1 + 2.0 ** -keep), fmax * (1 + 2.0 ** -keep) * (1 - 2.0 ** -23),
                         fmax * (1 + 2.0 ** -keep) * (1 + 2.0 ** -23), 0.0, -0.0, 1.0, -1.0, 3e38, -3e38], dtype=torch.float32)
    for v in (x, ties, sub, edge, x.double() * (1 + 2.0 ** -30)):          # the last: double inputs take the double -> f32 -> 16 bit path
        got, ref = round_to(v, operands), v.float().to(dtype).double()
        assert torch.equal(torch.isinf(got), torch.isinf(ref))
        fin = torch.isfinite(ref)
        assert torch.equal(got[fin], ref[fin]) and torch.equal(torch.signbit(got), torch.signbit(ref))


def _unpack16(packed, cin_padded, ksize, cin):
    """inverse of pack_weights16_impl (sz_nn.hip): out[t][ks][tile][l][j] with co = tile*16 + (l & 15), ci = ks*32 + 8*(l >> 4) + j -> [256, cin, k, k] uint16 bits"""
    taps, ksteps = ksize * ksize, cin_padded // 32
    a = packed.reshape(taps, ksteps, 16, 4, 16, 8)                           # t, ks, tile, l >> 4, l & 15, j
    w = a.transpose(2, 4, 1, 3, 5, 0).reshape(256, cin_padded, taps)         # co = (tile, l & 15), ci = (ks, l >> 4, j)
    return w[:, :cin].reshape(256, cin, ksize, ksize)


def _bits(t, operands):
    return t.float().to(torch.bfloat16 if operands == "bf16" else torch.float16).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
@pytest.mark.parametrize("regime", [False, True], ids=["benign", "trained"])
def test_folded_weights_are_what_the_packers_store(operands, regime):
    """all 39 tower convolutions and conv_p1, as FastPolicyNet packs them (fastnet._fold_bn + _pack -> sz_nn_pack_weights16[_f16]), unpacked from the MFMA
    fragment order: the emulation's rounded weights bit for bit; the folded f32 biases equal too"""
    net = _net(3, regime)
    f16 = operands == "fp16"
    em = Emulated(net, operands)
    mods = [(net.conv1.weight, net.norm_layer)] + [p for blk in net.resnet_blocks for p in ((blk.conv1.weight, blk.bn1), (blk.conv2.weight, blk.bn2))]
    mods.append((net.conv_p1.weight, net.p_norm1))
    mine = folded_convs(net, operands) + [em.p1]
    assert len(mods) == 40
    for k, ((cw, bn), (w_em, b_em)) in enumerate(zip(mods, mine)):
        w, b = _fold_bn(cw, bn)
        ksize, cin = cw.shape[2], cw.shape[1]
        cin_padded = 128 if cin == 119 else 256
        packed = _pack(w, cin_padded, ksize, "cpu", w16=True, f16=f16).numpy().view(np.uint16)
        assert np.array_equal(_unpack16(packed, cin_padded, ksize, cin), _bits(w_em, operands)), k
        assert not _unpack16(packed, cin_padded, ksize, cin_padded)[:, cin:].any()            # the stem's padding channels 119..127 are zero
        assert torch.equal(b.double(), b_em), k
    if regime:
        assert float(mine[0][0].abs().max()) > 50                           # the stem channels on the rare planes really are O(100)


def test_trained_regime_is_what_it_says():
    net = _net(4, regime=True)
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d) and m.num_features == 256]
    gamma = torch.cat([m.weight.detach() for m in bns])
    var = torch.cat([m.running_var.detach() for m in bns])
    beta = torch.cat([m.bias.detach() for m in bns])
    assert float((gamma == 0).float().mean()) > 0.02 and float((gamma < 0).float().mean()) > 0.05 and float(gamma.abs().max()) > 2
    assert float(var.min()) < 2e-3 and float(var.max()) > 5 and float(beta.min()) < -4
    from nnref import report
    xmax = report(net)
    assert 30 < xmax < 3000, xmax                                             # the residual stream is O(100) after block 19


# ---- the inputs of the f16 range tests (tests/f16range.py): networks that reach f16's rounding-to-inf point at one chosen site -----------------------------------
import f16range as R
from nnref import F16_INF_FROM, scale_site, site_names


@pytest.mark.parametrize("site", R.SITES)
def test_range_nets_reach_their_target_at_their_site_and_nowhere_else_first(site):
    """per site: scale_site's bisection reaches its target to 1 %; the 0.9 x 65504 net stays below f16's rounding-to-inf point 65520 at EVERY site, with f16-rounded
    weights (what the kernels multiply) as without rounding; the 2 x 65504 net has its FIRST excess at the intended site, every site in front of it is O(1)"""
    x = R.boards()
    for target in (R.IN_RANGE, R.OUT_OF_RANGE):
        _, reached = scale_site(R.base_net(), site, target, x)
        assert abs(reached / target - 1) <= 0.01, (site, target, reached)
    names = site_names(19)
    for op in (None, "fp16"):
        peaks = Emulated(R.net_at(site, R.IN_RANGE), op).site_maxima(x)
        assert list(peaks) == names
        worst = max(float(v.max()) for v in peaks.values())
        assert abs(float(peaks[site].max()) / R.IN_RANGE - 1) <= 0.011 and worst < F16_INF_FROM * 0.95, (site, op, float(peaks[site].max()), worst)
    peaks = Emulated(R.net_at(site, R.OUT_OF_RANGE), None).site_maxima(x)
    over = [n for n in names if float(peaks[n].max()) >= F16_INF_FROM]
    assert over and over[0] == site, (site, over[:3])
    assert all(float(peaks[n].max()) < 10 for n in names[:names.index(site)]), site
    assert float(peaks[site].min()) >= F16_INF_FROM, (site, peaks[site])          # every one of the four boards overflows there


def test_range_boundary_nets_straddle_the_rounding_to_inf_point():
    """the stem-only nets of the boundary test: the largest stem value on f16-rounded weights is 65400 resp. 65650 to 1e-5, i.e. 1.8e-3 below / 2.0e-3 above 65520
    (the kernel's f32 accumulation of at most 1071 terms is off by at most 1071 x 2^-24 = 6.4e-5 relative); round_to agrees: finite below, inf above"""
    for target, finite in ((65400.0, True), (65650.0, False)):
        net, reached = R.stem_net_at(target)
        peaks = Emulated(net, "fp16", n_blocks=0).site_maxima(R.boards())
        assert abs(float(peaks["stem"].max()) / target - 1) <= 1e-5 and reached == float(peaks["stem"].max()), (target, reached)
        assert bool(torch.isfinite(round_to(peaks["stem"].max(), "fp16"))) == finite
        assert bool(torch.isfinite(Emulated(net, "fp16", n_blocks=0).tower(R.boards())).all()) == finite


def test_one_bad_board_net_has_a_gap_around_the_rounding_to_inf_point():
    """one board's peak at block9.t is above 65520 and every other board's below, each by more than 2e-3 relative (30 x the f32 accumulation error); every site
    in front of block9.t is O(1) and, for the three good boards, every site behind it is in range"""
    net, bad, peaks = R.one_bad_board()
    p = peaks["block9.t"]
    good = [b for b in range(R.N_BOARDS) if b != bad]
    assert float(p[bad]) > F16_INF_FROM * 1.002 and float(p[good].max()) < F16_INF_FROM * 0.998, (bad, p.tolist())
    clean = Emulated(net, "fp16").site_maxima(R.boards()[good])
    assert max(float(v.max()) for v in clean.values()) < F16_INF_FROM * 0.998
    # the bad board overflows to +inf (a peak of -65520 or below would pack to -inf and the ReLU would make the correct 0 of it): the emulation's probabilities
    # are non-finite on that board and on no other
    assert float(R.site_values(net, "block9.t", R.boards())[bad].max()) > F16_INF_FROM * 1.002
    pi, v = Emulated(net, "fp16")(R.boards(), inference=True)
    assert (~torch.isfinite(pi).all(1)).tolist() == [b == bad for b in range(R.N_BOARDS)] and bool(torch.isfinite(v[good]).all())


@pytest.mark.parametrize("site", R.SPLIT_SITES)
def test_split_range_nets_fit_the_split_packing_and_reach_their_target(site):
    """the two-layer nets for SplitPolicyNet(operands="fp16"): every folded weight below 65520 / 2^10 (what its constructor accepts); the 0.9 x net below 65520
    everywhere; the 2 x net first exceeds it at the site, and there every board's largest POSITIVE value does (the split kernels pack after the f32 ReLU)"""
    x = R.boards()
    names = site_names(19)
    for target in (R.IN_RANGE, R.OUT_OF_RANGE):
        net = R.split_net_at(site, target)
        assert R.largest_folded_weight(net) < R.SPLIT_W_LIMIT * 0.99, (site, target, R.largest_folded_weight(net))
        peaks = Emulated(net, None).site_maxima(x)
        assert abs(float(peaks[site].max()) / target - 1) <= 0.011
        if target == R.IN_RANGE:
            assert max(float(v.max()) for v in peaks.values()) < F16_INF_FROM * 0.95
        else:
            over = [n for n in names if float(peaks[n].max()) >= F16_INF_FROM]
            assert over[0] == site and all(float(peaks[n].max()) < 1000 for n in names[:names.index(site)])
            assert float(R.site_values(net, site, x, None).flatten(1).max(1).values.min()) > F16_INF_FROM * 1.5
