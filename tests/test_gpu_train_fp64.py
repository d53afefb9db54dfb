"""The train step's matrix-core pieces (sigma_zero_amd/trainconv.py: ConvBNAct, SplitConv3x3, the whole default step) against fp64 twins of the same computation,
each next to torch fp32's own distance from the same fp64 reference.  ReLU branch flips (an input within rounding of zero taking the other branch in one evaluation)
are taken out of the gradient comparisons by giving the fp64 and fp32 backward passes the device's mask y > 0."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sigma_zero_amd as sz
from sigma_zero_amd import train_rl
from sigma_zero_amd import trainconv as TC

pytestmark = pytest.mark.gpu

rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _conv_bn_act_ref(x, w, bn, res, mask):
    """relu(bn_train(conv3x3(x, w)) [+ res]) in the dtype of its inputs; mask given: the ReLU is multiplication by that mask (same value, fixed branches)"""
    pre = bn(F.conv2d(x, w, padding=1))
    if res is not None:
        pre = pre + res
    return pre * mask if mask is not None else torch.relu(pre)


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
def test_conv_bn_act_against_fp64(with_res):
    """trainconv.ConvBNAct (weight pack + split-precision convolution + fused train-mode BatchNorm / skip / ReLU, and its backward) against the same node in fp64:
    output, running_mean / running_var, and the gradients of x, w, gamma, beta and the skip input — each within max(3 x torch fp32's distance from fp64, 3e-7),
    the per-op bound of test_gpu_round3.py's BNAct test; batches 1, 8, 37, n/2, n/2+1, n (CUs: the two-workgroups-per-board form ends at n/2), 256 (the
    BatchNorm kernels' register cache, sz_train.hip BN_MAXV), 257, 300 (eight distinct sizes on 256 CUs).  Measured on MI355X, worst ratio to torch fp32's error
    (floor 1e-7) over the batches: y 2.7, running_mean 1.2, running_var 0.5, dx 2.2, dw 1.3, dgamma 2.9, dbeta 1.2, dres 0."""
    n = _n_cu()
    g = torch.Generator(device="cuda").manual_seed(17)
    C = 256
    names = ["y", "running_mean", "running_var", "dx", "dw", "dgamma", "dbeta"] + (["dres"] if with_res else [])
    worst = {k: 0.0 for k in names}
    for B in sorted({1, 8, 37, n // 2, n // 2 + 1, n, 256, 257, 300}):
        x = torch.randn(B, C, 8, 8, device="cuda", generator=g) * (torch.rand(B, C, 8, 8, device="cuda", generator=g) < 0.6)
        w = torch.randn(C, C, 3, 3, device="cuda", generator=g) * 0.03
        res = torch.randn(B, C, 8, 8, device="cuda", generator=g) if with_res else None
        gy = torch.randn(B, C, 8, 8, device="cuda", generator=g)
        out, mask = {}, None
        for kind in ("fused", "fp64", "torch"):
            dt = torch.float64 if kind == "fp64" else torch.float32
            bn = torch.nn.BatchNorm2d(C).cuda().to(dt).train()
            with torch.no_grad():
                bn.weight.copy_(torch.linspace(-0.5, 1.5, C)); bn.bias.copy_(torch.linspace(-0.3, 0.3, C)); bn.running_mean.fill_(0.1); bn.running_var.fill_(0.8)
            xx, ww = x.detach().to(dt).clone().requires_grad_(True), w.detach().to(dt).clone().requires_grad_(True)
            rr = res.detach().to(dt).clone().requires_grad_(True) if with_res else None
            if kind == "fused":
                y = TC.ConvBNAct.apply(xx, ww, bn.weight, bn.bias, rr, bn.running_mean, bn.running_var, bn.momentum, bn.eps)
                mask = (y.detach() > 0).to(torch.float64)
            else:
                y = _conv_bn_act_ref(xx, ww, bn, rr, mask.to(dt))
            y.backward(gy.to(dt))
            out[kind] = [y.detach(), bn.running_mean.clone(), bn.running_var.clone(), xx.grad, ww.grad, bn.weight.grad, bn.bias.grad] + ([rr.grad] if with_res else [])
        for i, name in enumerate(names):
            ef, et = rel(out["fused"][i], out["fp64"][i]), rel(out["torch"][i], out["fp64"][i])
            worst[name] = max(worst[name], ef / max(et, 1e-7))
            assert ef < max(3 * et, 3e-7), (B, with_res, name, ef, et)
    print("ConvBNAct vs fp64, worst ratio to torch fp32's error (floor 1e-7) per quantity:", {k: round(v, 2) for k, v in worst.items()})


def test_split_convolution_weight_magnitude_sweep():
    """SplitConv3x3 packs the weights times 2^10 as hi + lo f16: from max|w| = 3e-3 (lo parts near f16's subnormals) to 3 (the init scale x0.1 .. x100), forward,
    input gradient and weight gradient stay within 2e-6 relative L2 of fp64 (the bound of test_gpu_round3.py) and finite.  Measured on MI355X at every magnitude:
    5.1e-7 / 5.1e-7 / 1.9e-7.  Weights of 64 and more are refused when the convolutions are switched on (test_network_and_train.py)."""
    from sigma_zero_amd.trainconv import SplitConv3x3
    g = torch.Generator(device="cuda").manual_seed(9)
    base = torch.randn(256, 256, 3, 3, device="cuda", generator=g)
    base = base / base.abs().max()
    B = 37
    x = (torch.randn(B, 256, 8, 8, device="cuda", generator=g) * (torch.rand(B, 256, 8, 8, device="cuda", generator=g) < 0.5))
    gy = torch.randn(B, 256, 8, 8, device="cuda", generator=g)
    rows = []
    for wmax in (3e-3, 1e-2, 3e-2, 0.3, 3.0):
        w = (base * wmax).requires_grad_()
        xx = x.clone().requires_grad_()
        y64 = F.conv2d(xx.double(), w.double(), padding=1)
        y64.backward(gy.double())
        gx64, gw64 = xx.grad.clone(), w.grad.clone()
        xx.grad = None; w.grad = None
        y = SplitConv3x3.apply(xx, w)
        y.backward(gy)
        r = (rel(y, y64), rel(xx.grad, gx64), rel(w.grad, gw64))
        rows.append((wmax,) + r)
        assert all(bool(torch.isfinite(t).all()) for t in (y, xx.grad, w.grad))
        assert max(r) < 2e-6, (wmax, r)
    print("\n".join("max|w| %7.0e: forward %.2e, input gradient %.2e, weight gradient %.2e" % row for row in rows))


def _twin_step(net, batch, dtype, dev="cuda"):
    """gradients of one train step (train_rl.loss_fn, train mode) of `net` in `dtype`, flat double; per-parameter slices in the order of named_parameters()"""
    b = {k: v.to(dev).to(dtype) for k, v in batch.items()}
    net.zero_grad()
    loss, _, _ = train_rl.loss_fn(net, b, dev)
    loss.backward()
    return torch.cat([p.grad.flatten().double() for p in net.parameters()])


def _groups(net):
    """parameter groups for the report: stem, tower convolutions, tower BatchNorms, heads — as index slices of the flat gradient"""
    out, off = {}, 0
    for name, p in net.named_parameters():
        grp = "tower conv" if name.startswith("resnet_blocks") and ".conv" in name else "tower bn" if name.startswith("resnet_blocks") else \
              "stem" if name.startswith(("conv1", "norm_layer")) else "heads"
        out.setdefault(grp, []).append(slice(off, off + p.numel()))
        off += p.numel()
    return out


def _step_with_masks(net, batch, dtype, masks, record):
    """one step of `net` through split_convs(net) with trainconv._conv_bn_act wrapped (it is looked up when called): record=True runs the fused nodes and appends
    each of the 38 tower sites' mask y > 0 to `masks`; record=False computes every site as torch's conv + BatchNorm (+ skip) in `dtype` times the recorded mask —
    the same function, with the device's ReLU branches"""
    from sigma_zero_amd.trainconv import split_convs
    orig, it = TC._conv_bn_act, iter(masks)

    def wrapped(conv, bn, x, residual=None):
        if record:
            y = orig(conv, bn, x, residual)
            masks.append(y.detach() > 0)
            return y
        pre = bn(getattr(conv, "_sz_orig_forward", conv)(x))
        if residual is not None:
            pre = pre + residual
        return pre * next(it).to(pre.dtype)
    TC._conv_bn_act = wrapped
    try:
        with split_convs(net):
            return _twin_step(net, batch, dtype)
    finally:
        TC._conv_bn_act = orig


def test_whole_train_step_against_an_fp64_step(golden_dir):
    """the default train step (split_convs: ConvBNAct at the 38 tower sites) and MIOpen's fp32 step, each against an fp64 twin of the same step (same weights,
    same batch, train-mode BatchNorm), on the golden 8-sample batch and on a 128-sample batch (train_rl's batch size).
    Without masks the comparison measures ReLU branch flips, not arithmetic: a tower input within rounding of zero takes the other branch in one of the two
    evaluations, and 39 train-mode BatchNorms carry that through the whole gradient.  Measured on MI355X, unmasked, golden batch: split 5.2e-3, MIOpen 4.0e-4 in
    one process and 1.3e-6 in another (its algorithm choice decides which inputs flip) — uniform over the parameter groups, the signature of flips.
    So the asserted comparison gives all three steps the split step's own masks at the 38 tower sites (trainconv._conv_bn_act wrapped; the stem's and the heads'
    ReLUs stay unmasked).  Measured on MI355X, masked: golden 8 — MIOpen 1.2e-6, split + fused 2.75e-6 (ratio 2.2; stem / tower conv / tower bn / heads 2.3e-6 /
    2.8e-6 / 3.1e-6 / 5.7e-6 against MIOpen's 1.0e-6 / 1.3e-6 / 1.3e-6 / 2.5e-6); random 128 — MIOpen 3.6e-4, split 5.7e-4 (ratio 1.6, uniform over the groups:
    flips at the unmasked ReLUs remain).  The split step is not within 1.25x of MIOpen: it is within MASKED_RATIO x and MASKED_BOUND."""
    z = np.load(os.path.join(golden_dir, "train_loss_golden.npz"))
    g = torch.Generator().manual_seed(3)
    batches = {"golden8": {"states": torch.from_numpy(z["x"].astype(np.float32)), "actions": torch.from_numpy(z["p_target"]), "rewards": torch.from_numpy(z["v_target"])},
               "random128": {"states": (torch.rand(128, 119, 8, 8, generator=g) < 0.15).float(), "actions": torch.softmax(torch.randn(128, 4672, generator=g) * 3, 1),
                             "rewards": torch.randint(-1, 2, (128,), generator=g).float()}}
    from sigma_zero_amd.trainconv import split_convs
    for name, batch in batches.items():
        torch.manual_seed(0)
        net = sz.policyNN({}).cuda().train()
        state = copy.deepcopy(net.state_dict())
        net64 = copy.deepcopy(net).double()
        masks = []
        g_sp = _step_with_masks(net, batch, torch.float32, masks, record=True)
        assert len(masks) == 38
        net.load_state_dict(state)
        g_mi = _step_with_masks(net, batch, torch.float32, masks, record=False)
        g64 = _step_with_masks(net64, batch, torch.float64, masks, record=False)
        net.load_state_dict(state)
        u_mi = _twin_step(net, batch, torch.float32)
        net64.load_state_dict({k: v.double() for k, v in state.items()})
        u64 = _twin_step(net64, batch, torch.float64)
        r_mi, r_sp = rel(g_mi, g64), rel(g_sp, g64)
        lines = ["%s, masked: gradient rel L2 vs fp64 — MIOpen fp32 %.2e, split + fused %.2e (ratio %.2f); unmasked: MIOpen %.2e, split %.2e"
                 % (name, r_mi, r_sp, r_sp / r_mi, rel(u_mi, u64), rel(g_sp, u64))]
        for grp, sl in _groups(net).items():
            a, b, c = (torch.cat([t[s] for s in sl]) for t in (g_mi, g_sp, g64))
            lines.append("  %-10s MIOpen %.2e  split %.2e" % (grp, rel(a, c), rel(b, c)))
        print("\n".join(lines))
        assert r_sp <= MASKED_RATIO * r_mi and r_sp < MASKED_BOUND[name], (name, r_sp, r_mi)


MASKED_RATIO = 3.0
MASKED_BOUND = {"golden8": 1e-5, "random128": 2e-3}
