"""fp64 emulation of the train step's split-precision convolution kernels (sigma_zero_amd/trainconv.py SplitConv3x3; csrc/sz_nn_split.hip k_conv3x3_split_f32,
k_wgrad3x3_split + k_wgrad_reduce, f16 operands) for the tests: the kernels' stated arithmetic, rounded where they round and exact everywhere else, so that a
kernel differs from it by its f32 accumulation alone.  Plain torch; runs on the CPU and, in fp64, on the device.

What the kernels do, restated:
  scale     a scaling UNIT (one board for forward and backward-data, the whole tensor — each of gy and x — for the weight gradient) is multiplied by 2^k,
            k = 11 - (unbiased f32 exponent of the unit's max |t|) clamped to +-100, so that the maximum lands in [2^11, 2^12); k = 0 for an all-zero, subnormal or
            non-finite maximum (pow2_from_amax_bits and the copy inside k_conv3x3_split_f32).  The weights are multiplied by 2^10 (SP_WSCALE_LOG2).  Both exact.
  split     s -> hi = f16(s) (round to nearest even), lo = f16(f32(s) - f32(hi)); f16 subnormals are kept.
  product   w * x ~= w_hi * x_hi + w_lo * x_hi + w_hi * x_lo (three MFMAs, the lo * lo term dropped); every product of two f16 is exact in f32; the kernels add
            them in f32, this module in fp64 — the only difference between the two.
  unscale   convolution: times 2^-(k + 10) per board; weight gradient: times 2^-k_gy * 2^-k_x.  Exact.
Backward-data is the forward convolution of gy with W'[ci][co][tap] = w[co][ci][8 - tap] (packed times 2^10 like the forward stream).

The range contract this implies (RANGE below, tests/test_trainref.py holds it): with its unit's maximum at 2^11.., an element within 2^14 of that maximum has a
normal lo part and keeps 22 bits; below that lo is a multiple of f16's subnormal quantum 2^-24, the element's ABSOLUTE error stays at 2^-25 scaled (2^-36 .. 2^-37 of
the unit's maximum) and its relative error doubles per octave — 11 bits left 2^25 below the maximum, nothing 2^36 below.

`bug=` injects one plausible kernel bug on this side (the tests' teeth): see BUGS.
BatchNorm + skip + ReLU need no emulation: bn_act_ref is the plain formula in the dtype of its inputs, with torch's conventions.
"""
import torch
import torch.nn.functional as F

WSCALE_LOG2 = 10                                           # SP_WSCALE_LOG2
TARGET_LOG2 = 11                                           # a unit's maximum is scaled into [2^11, 2^12)
K_CLAMP = 100
# octaves below its unit's maximum at which an element: still keeps hi + lo's 22 bits / is down to hi's 11 / is flushed to zero (see the module docstring)
RANGE = {"full": 14, "hi_only": 25, "zero": 36}
BUGS = ("drop_x_lo_tile",          # the w_hi * x_lo (weight gradient: gy_hi * x_lo) product missing for input channels 16 * tile .. + 15
        "board_scale_octave",      # one board unscaled with k + 1 (convolution)
        "tap_shift",               # one tap reads its input one column to the right of where it should
        "wrong_tensor_scale")      # weight gradient: gy scaled with x's k and x with gy's


def scale_exp(amax):
    """k of the scale rule for a tensor of unit maxima (any float dtype holding f32 values): int64, same shape"""
    a = amax.float()
    _, e = torch.frexp(a)                                      # a = m * 2^e with 0.5 <= m < 1: the unbiased exponent is e - 1
    normal = torch.isfinite(a) & (a >= 2.0 ** -126)
    k = torch.where(normal, TARGET_LOG2 + 1 - e.long(), torch.zeros_like(e, dtype=torch.long))
    return k.clamp(-K_CLAMP, K_CLAMP)


def amax_bits(t):
    """the word sz_nn_conv3x3_split_f32 leaves in amax_bits: the f32 bit pattern of max |t| over the whole tensor"""
    return int(t.detach().float().abs().max().reshape(1).view(torch.int32).item())


def _pow2(k, like):
    return torch.ldexp(torch.ones((), dtype=like.dtype, device=like.device), k.to(like.device))


def split(s):
    """f32 tensor -> (hi, lo) as doubles: hi = f16(s), lo = f16(s - hi), both round to nearest even with subnormals (torch's conversion; tests/test_nnref.py holds
    it to the format's definition bit for bit)"""
    s = s.float()
    hi = s.to(torch.float16)
    lo = (s - hi.float()).to(torch.float16)
    return hi.double(), lo.double()


def conv64(x, w):
    """3x3 convolution, padding 1, in the dtype of its inputs (double in every reference) as unfold + one matrix product (several times faster on the CPU than
    torch's direct fp64 convolution; tests/test_trainref.py holds it and wgrad64 to autograd's F.conv2d)"""
    B, co = x.shape[0], w.shape[0]
    return (w.reshape(co, -1) @ F.unfold(x, 3, padding=1)).view(B, co, x.shape[2], x.shape[3])


def wgrad64(gy, x):
    """dw[co][ci][tap] = sum over boards and positions of gy[b][co][pos] * x[b][ci][pos + off(tap)] in double"""
    B, co, ci = gy.shape[0], gy.shape[1], x.shape[1]
    cols = F.unfold(x, 3, padding=1)                           # [B, ci * 9, 64]
    return torch.einsum("bop,bkp->ok", gy.reshape(B, co, -1), cols).view(co, ci, 3, 3)


def _shift_tap(w, tap):
    """the weights of `tap` = (ky, kx < 2) applied one column to the right: they land on tap (ky, kx + 1)"""
    ky, kx = tap
    w = w.clone()
    w[:, :, ky, kx + 1] += w[:, :, ky, kx]
    w[:, :, ky, kx] = 0
    return w


def conv3x3_split(x, w, transposed=False, bug=None, tile=1, board=0, tap=(0, 0)):
    """k_conv3x3_split_f32<ElemF16> on x [B, ci, 8, 8] and the torch weight w [co, ci, 3, 3] (f32 values): double [B, co, 8, 8].  transposed: the backward-data
    convolution (x is then the output gradient)."""
    wd = w.detach().float() * float(1 << WSCALE_LOG2)
    if transposed:
        wd = wd.transpose(0, 1).flip(2, 3)
    wh, wl = split(wd.contiguous())
    xf = x.detach().float()
    k = scale_exp(xf.abs().amax(dim=(1, 2, 3)))
    xh, xl = split(xf * _pow2(k, xf).view(-1, 1, 1, 1))
    if bug == "drop_x_lo_tile":
        xl = xl.clone(); xl[:, 16 * tile:16 * tile + 16] = 0
    if bug == "tap_shift":
        wh, wl = _shift_tap(wh, tap), _shift_tap(wl, tap)
    acc = conv64(xh, wh + wl) + conv64(xl, wh)                 # wh + wl is exact in double: (w_hi + w_lo) * x_hi + w_hi * x_lo
    ku = k + WSCALE_LOG2
    if bug == "board_scale_octave":
        ku = ku.clone(); ku[board] += 1
    return acc * _pow2(-ku, acc).view(-1, 1, 1, 1)


def wgrad_split(gy, x, bug=None, tile=1, tap=(0, 0)):
    """k_wgrad3x3_split + k_wgrad_reduce on gy, x [B, 256, 8, 8] (f32 values): double [co, ci, 3, 3]; one scale per TENSOR"""
    gf, xf = gy.detach().float(), x.detach().float()
    kg, kx = scale_exp(gf.abs().amax()), scale_exp(xf.abs().amax())
    sg, sx = (kx, kg) if bug == "wrong_tensor_scale" else (kg, kx)
    gh, gl = split(gf * _pow2(sg, gf))
    xh, xl = split(xf * _pow2(sx, xf))
    if bug == "drop_x_lo_tile":
        xl = xl.clone(); xl[:, 16 * tile:16 * tile + 16] = 0
    acc = wgrad64(gh + gl, xh) + wgrad64(gh, xl)               # gy_hi * x_hi + gy_lo * x_hi + gy_hi * x_lo
    if bug == "tap_shift":                                     # tap (ky, kx) computed from x one column to the right: it holds what belongs to tap (ky, kx + 1)
        acc = acc.clone(); acc[:, :, tap[0], tap[1]] = acc[:, :, tap[0], tap[1] + 1]
    return acc * _pow2(-(sg + sx), acc)


def bn_act_ref(x, gamma, beta, residual, running_mean, running_var, momentum, eps, mask=None):
    """relu(batch_norm_train(x) [+ residual]) in the dtype of its inputs with torch.nn.BatchNorm2d's conventions: biased variance in the output, unbiased into
    running_var, eps inside the root.  Returns (y, new running_mean, new running_var); `mask` given: the ReLU is multiplication by it (fixed branches)."""
    n = x.numel() // x.shape[1]
    mean = x.mean(dim=(0, 2, 3))
    d = x - mean.view(1, -1, 1, 1)
    ssd = (d * d).sum(dim=(0, 2, 3))
    pre = d * torch.rsqrt(ssd / n + eps).view(1, -1, 1, 1) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    if residual is not None:
        pre = pre + residual
    y = pre * mask if mask is not None else torch.relu(pre)
    return y, (1 - momentum) * running_mean + momentum * mean.detach(), (1 - momentum) * running_var + momentum * (ssd.detach() / max(n - 1, 1))


# ---- inputs shared by the CPU and the device tests ---------------------------------------------------------------------------------------------------------------
def integer_case(B, seed, device="cpu", zero_board=None):
    """(x, gy, w): x and gy integer-valued in [-4, 4] with whole rows, columns and channels zero (border tiles, the zero-tile skipping), w integer-valued in [-2, 2]"""
    g = torch.Generator().manual_seed(seed)
    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()
    out = []
    for _ in range(2):
        t = ints(-4, 4, B, 256, 8, 8)
        t = t * (torch.rand(B, 256, 1, 1, generator=g) < 0.8) * (torch.rand(B, 1, 8, 1, generator=g) < 0.8) * (torch.rand(B, 1, 1, 8, generator=g) < 0.8)
        t[:, :, 0, :] = 0; t[:, 32:48] = 0                     # the top row and one whole channel tile: zero in every board
        if zero_board is not None:
            t[zero_board] = 0
        out.append(t)
    w = ints(-2, 2, 256, 256, 3, 3)
    return out[0].to(device), out[1].to(device), w.to(device)


def gauss_case(B, seed, device="cpu"):
    """(x, gy, w) of one scale each: x half zeros (a ReLU's output), gy dense, w at the initialisation's scale"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 256, 8, 8, generator=g) * (torch.rand(B, 256, 8, 8, generator=g) < 0.5)
    gy = torch.randn(B, 256, 8, 8, generator=g)
    w = torch.randn(256, 256, 3, 3, generator=g) * 0.03
    return x.to(device), gy.to(device), w.to(device)


def line_rel(a, ref, dims):
    """relative L2 distance of `a` from the double `ref`, reduced over `dims` only (per board, per row, per column ...); a line whose reference is all zero has
    distance 0 if `a` is all zero there too, else inf"""
    num = (a.double() - ref).pow(2).sum(dims).sqrt()
    den = ref.pow(2).sum(dims).sqrt()
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


def octave_scales(n, first, last, device="cpu", dtype=torch.float32):
    """n powers of two whose exponents run evenly (rounded to integers) from `first` down to `last`"""
    e = torch.round(torch.linspace(float(first), float(last), n)).to(torch.int32)
    return torch.ldexp(torch.ones(n, dtype=dtype), e).to(device)
