"""The f16 networks at and beyond f16's range, on the device: FastPolicyNet(operands="fp16") stores its activations as f16 (a value of 65520 or more rounds
to inf), SplitPolicyNet(operands="fp16") keeps an unscaled f16 hi image (the same limit, for positive values).  Inputs are the nets of tests/f16range.py, which
reach 0.9 x 65504 or 2 x 65504 at ONE site (stem, block9.t, block15.out, block18.out, p1) on four fixed boards, checked on the CPU by test_nnref.py; the reference
is tests/nnref.py (fp64 with the kernels' rounding points; round_to overflows to inf as the conversion does).
  (a) in range, at the limit: finite, and per board within the fp16 bounds of test_gpu_exact_rounding.py (split: of test_gpu_network.py);
  (b) the boundary: 65400 stays finite and equals the emulation's bits, 65650 is +inf exactly where the emulation's rounding gives inf;
  (c) out of range: the kernels are never inf / NaN on a board that is good in the emulation, the good boards of the batch keep the bounds of (a), and the
      record of what the bad boards come out as (SILENT: three of six nets return finite garbage) is held; the range flag is set for every one of them;
  (d) teeth: (c) against an emulation that saturates at +-65504 fails;
  then the range flag: overflowed() of both networks and SelfPlayEngine.check_errors() raising on it.
Every case runs in the automatic workgroup form and in both forced ones, on the bf16 NHWC image and on the bit-packed planes."""
import copy
import functools

import pytest
import torch

from sigma_zero_amd import _native as N
from sigma_zero_amd.fastnet import FastPolicyNet, SplitPolicyNet, planes_nchw_to_nhwc128
from sigma_zero_amd.selfplay import SelfPlayEngine

import f16range as R
from nnref import Emulated, round_to
# the metrics and bounds of the O(1) tests, unchanged: FULL["fp16"] = tower 2e-3 / centred logits 3e-4 (relative L2), value 4e-4 (absolute);
# HEADS_SOFTMAX["fp16"] = 1e-4 (largest relative error of a probability, heads on the kernel's own tower output); MIN_IDENTICAL / MAX_EXCESS["fp16"] = 0.8 / 1e-3
from test_gpu_exact_rounding import FULL, HEADS_SOFTMAX, MAX_EXCESS, MIN_IDENTICAL, _ref_bits, _tower_bits, _tower_vals, _ulps
from test_gpu_network import _pack_bits128

pytestmark = pytest.mark.gpu

FORMS = (("auto", 0, 0), ("wgb1", N.SZ_NN_TOWER_WGB1, N.SZ_NN_SPLIT_WGB1), ("wgb2", N.SZ_NN_TOWER_WGB2, N.SZ_NN_SPLIT_WGB2))
OUT_CASES = R.SITES + ("one_bad_board",)
F16_INF_BITS = 0x7C00
# bounds of test_gpu_network.py::test_split_precision_network_with_f16_operands_is_as_close_to_fp64_as_fp32_is, per board: tower and centred logits in
# relative L2, value absolute
SPLIT_BOUNDS = {"tower": 3e-6, "logits": 3e-6, "value": 1e-6}
P_FLOOR = 1e-30            # probabilities below it are left out of the relative softmax error (f32 has no normal numbers below 1.2e-38; at O(1) none is that small)


def _net(case, target=None):
    if case == "one_bad_board":
        return R.one_bad_board()[0]
    if case == "base":
        return R.base_net()
    return R.net_at(case, target)


@functools.lru_cache(maxsize=None)
def _planes():
    """the four boards: (nchw [4, 119, 8, 8] double on the device, ((format, planes), ...))"""
    x = R.boards().cuda()
    img = planes_nchw_to_nhwc128(x.float())
    return x, (("nhwc128", img), ("bits128", _pack_bits128(img.float())))


_FAST = {}


def _fast(case, target=None, cls=FastPolicyNet, net=None):
    key = (case, target, cls)
    if key not in _FAST:
        _FAST[key] = cls(_net(case, target) if net is None else net, device="cuda", operands="fp16")
    return _FAST[key]


def _flat(v):
    return v.double().reshape(v.shape[0], -1)


def _per_board(y, l, v, y64, l64, v64):
    """the metrics of FULL, per board: {"tower", "logits": relative L2 (logits centred), "value": absolute} as [B] tensors"""
    cen = lambda t: t - t.mean(1, keepdim=True)
    r = lambda a, b: (_flat(a) - _flat(b)).norm(dim=1) / _flat(b).norm(dim=1)
    return {"tower": r(y, y64), "logits": r(cen(_flat(l)), cen(_flat(l64))), "value": (_flat(v) - _flat(v64)).abs().max(1).values}


def _softmax_rel(pi, pi64):
    """the metric of HEADS_SOFTMAX per board: largest |pi - pi64| / pi64 over the probabilities of at least P_FLOOR"""
    pi, pi64 = _flat(pi), _flat(pi64)
    return torch.where(pi64 >= P_FLOOR, (pi - pi64).abs() / pi64.clamp_min(P_FLOOR), torch.zeros_like(pi64)).max(1).values


class _Reference:
    """per net, computed once: the fp16 emulation and fp64 on the four boards, the emulation's own distance from fp64 in the metrics of FULL (its
    sensitivity: what one f16 rounding is worth in this net), and the emulation's bad boards (a non-finite probability or value)"""

    def __init__(self, net, emulation=Emulated):
        x = _planes()[0]
        self.em, self.em64 = emulation(net, "fp16", device="cuda"), Emulated(net, None, device="cuda")
        with torch.no_grad():
            self.y = self.em.tower(x)
            self.l, self.v = self.em.heads(self.y)
            self.pi = self.em.heads(self.y, inference=True)[0]
            y64 = self.em64.tower(x)
            l64, v64 = self.em64.heads(y64)
        self.bad = ~(torch.isfinite(self.pi).all(1) & torch.isfinite(self.v).all(1))
        self.sens = _per_board(self.y, self.l, self.v, y64, l64, v64)
        self.y64, self.l64, self.v64 = y64, l64, v64

    def softmax_sens(self, y):
        """the emulated heads' own distance from the fp64 heads on one tower output, in the metric of HEADS_SOFTMAX"""
        with torch.no_grad():
            return _softmax_rel(self.em.heads(y, inference=True)[0], self.em64.heads(y, inference=True)[0])


_REF = {}


def _ref(case, target=None):
    if (case, target) not in _REF:
        _REF[(case, target)] = _Reference(_net(case, target))
    return _REF[(case, target)]


def _bounds(ref, softmax_sens):
    """per-board bounds of the kernel's distance from the emulation: the bounds that hold at O(1) (FULL / HEADS_SOFTMAX, fp16) times the factor by which THIS
    net's sensitivity exceeds the healthy net's (never below the O(1) bound's own value).  Both sensitivities come from the reference alone: the distance of the
    f16 emulation from fp64, which grows with the net exactly as the effect of a one-ulp disagreement between the kernel's f32 sums and the emulation's does."""
    base = _ref("base")
    if not hasattr(base, "softmax_base"):
        base.softmax_base = base.softmax_sens(base.y).max()
    # a metric in which the healthy net's emulation does not differ from fp64 at all (its value: the value head's ReLU is at 0 on these boards) has no ratio
    # to scale by: its O(1) bound stays as it is
    factor = lambda s, s0: torch.clamp(s / s0, min=1.0) if float(s0) > 0 else torch.ones_like(s)
    out = {k: FULL["fp16"][k] * factor(ref.sens[k], base.sens[k].max()) for k in FULL["fp16"]}
    out["softmax"] = HEADS_SOFTMAX["fp16"] * factor(softmax_sens, base.softmax_base)
    return out


def _run(fast, planes):
    """one forward pair of the kernels: (tower [B, 256, 8, 8] double, logits, probabilities, value)"""
    with torch.no_grad():
        l, v = (t.clone() for t in fast(planes, inference=False))
        pi, vi = (t.clone() for t in fast(planes, inference=True))
        y = _tower_vals(fast, planes, "fp16").clone()
    assert torch.equal(v.isnan(), vi.isnan()) and torch.equal(v.nan_to_num(7.0), vi.nan_to_num(7.0))
    return y, l, pi, v


def _check_boards(what, ref, y, l, pi, v, boards):
    """the boards in `boards` are finite and within the per-board bounds of the emulation; returns the figures"""
    with torch.no_grad():
        m = _per_board(y, l, v, ref.y, ref.l, ref.v)
        m["softmax"] = _softmax_rel(pi, ref.em.heads(torch.where(torch.isfinite(y), y, torch.zeros_like(y)), inference=True)[0])
        bound = _bounds(ref, ref.softmax_sens(torch.where(torch.isfinite(y), y, torch.zeros_like(y))))
    for b in boards:
        assert all(bool(torch.isfinite(t[b]).all()) for t in (y, l, pi, v)), (what, "board %d is not finite" % b)
        assert abs(float(pi[b].double().sum()) - 1) < 1e-5, (what, b, float(pi[b].double().sum()))
        for k in m:
            assert float(m[k][b]) <= float(bound[k][b]), (what, "board %d" % b, k, float(m[k][b]), float(bound[k][b]))
    return {k: (max(float(m[k][b]) for b in boards), min(float(bound[k][b]) for b in boards)) for k in m} if boards else {}


def _figures(fig):
    return "  ".join("%s %.2e (bound %.2e)" % (k, a, b) for k, (a, b) in fig.items())


# ---- (a) in range, at the limit ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site", R.SITES)
def test_in_range_at_the_limit(site):
    """net_at(site, 0.9 x 65504) through FastPolicyNet(operands="fp16"): tower, logits, probabilities and value finite, and every board within the fp16 bounds of
    test_gpu_exact_rounding.py of the emulation: FULL (tower 2e-3, centred logits 3e-4, value 4e-4) and HEADS_SOFTMAX (1e-4).  The logits and softmax bounds were
    measured on O(1) activations and do not hold here as they are, so a bound is its O(1) value times (this net's sensitivity / the healthy net's), the
    sensitivity being the f16 emulation's own distance from unrounded fp64 on the same net and boards (_bounds) — nothing of it comes from the kernel.
    Sensitivities, worst of the four boards (tower / logits / value / softmax): healthy net 7.4e-4 / 2.0e-4 / 0 / 1.5e-4; stem 9.5e-4 / 1.1e-3 / 0 / 8.3e-2;
    block9.t 1.0e-3 / 1.1e-3 / 1.1e-4 / 4.0e-3; block15.out 6.6e-4 / 9.3e-4 / 1e-13 / 1.4e-1; block18.out 7.3e-4 / 9.3e-4 / 0 / 1.1e-1; p1 7.5e-4 / 8.8e-4 / 0 / 2.0 (one
    board; 0 on the three whose policy is one move).  Kernel against emulation, measured on MI355X, the same in all forms and formats (bound in brackets):
    stem 2.0e-5 (2.5e-3) / 7.9e-5 (1.6e-3) / 0 / 1.5e-2 (3.7e-2); block9.t 8.6e-4 (2.6e-3) / 9.1e-4 (1.5e-3) / 4.6e-5 (4e-4) / 4.8e-4 (2.2e-3); block15.out 5.5e-4 (2e-3)
    / 7.5e-4 (1.4e-3) / 2e-13 / 5.5e-3 (4.7e-2); block18.out 7.2e-4 (2e-3) / 8.9e-4 (1.3e-3) / 0 / 9.3e-4 (4.3e-2); p1 7.3e-4 (2e-3) / 8.4e-4 (1.3e-3) / 2e-9 / 2.2e-3 on
    the board whose sensitivity is 2.0 (bound 1.4), 0 on the others.  The figures of every run are printed next to their bounds (run with -s)."""
    ref, fast = _ref(site, R.IN_RANGE), _fast(site, R.IN_RANGE)
    assert not bool(ref.bad.any())
    for fmt, planes in _planes()[1]:
        for form, flag, _ in FORMS:
            fast.force_wgb = flag
            fig = _check_boards((site, fmt, form), ref, *_run(fast, planes), boards=range(R.N_BOARDS))
            fast.force_wgb = 0
            print("%-11s %-7s %-4s %s" % (site, fmt, form, _figures(fig)))
    print("%-11s sensitivity (emulation against fp64): %s" % (site, {k: "%.2e" % float(v.max()) for k, v in ref.sens.items()}))


def _split_metrics(split, planes, em64, y64, l64, v64):
    B = planes.shape[0]
    with torch.no_grad():
        l, v = (t.clone() for t in split(planes, inference=False))
        pi = split(planes, inference=True)[0].clone()
        y = split.tower(planes).clone().view(B, 8, 8, 256).permute(0, 3, 1, 2)
    return y, l, pi, v, _per_board(y, l, v, y64, l64, v64)


@pytest.mark.parametrize("site", R.SITES)
def test_split_in_range_at_the_limit(site):
    """SplitPolicyNet(operands="fp16") against fp64, per board, at the bounds of test_gpu_network.py (tower and centred logits 3e-6 relative L2, value 1e-6).
    Its constructor refuses every one of the five nets of net_at(): they reach the target from O(1) activations with one layer, whose folded weights are 2e3 .. 1e4,
    and the x 2^10 weight packing holds less than 64.  That is asserted.  Turning layers BEHIND the site down does not change the site's own weights, so the
    magnitude is built in two layers instead (f16range.split_net_at: the site in front lifted to 512, then the site itself; folded weights 11 .. 37).  The stem
    has no layer in front — 59000 from at most 1071 planes of 0 / 1 needs weights of 55 on average — and is the one site skipped."""
    with pytest.raises(ValueError, match="f16"):
        SplitPolicyNet(copy.deepcopy(R.net_at(site, R.IN_RANGE)), device="cuda", operands="fp16")       # a copy: the constructor moves its module to the device
    if site == "stem":
        return
    net = R.split_net_at(site, R.IN_RANGE)
    split = _fast(("split", site), R.IN_RANGE, SplitPolicyNet, copy.deepcopy(net))
    x = _planes()[0]
    em64 = Emulated(net, None, device="cuda")
    with torch.no_grad():
        y64 = em64.tower(x)
        l64, v64 = em64.heads(y64)
    for fmt, planes in _planes()[1]:
        for form, _, flag in FORMS:
            split.force_wgb = flag
            y, l, pi, v, m = _split_metrics(split, planes, em64, y64, l64, v64)
            split.force_wgb = 0
            print("split %-11s %-7s %-4s %s" % (site, fmt, form, "  ".join("%s %.2e" % (k, float(t.max())) for k, t in m.items())))
            assert all(bool(torch.isfinite(t).all()) for t in (y, l, pi, v)), (site, fmt, form)
            for k, bound in SPLIT_BOUNDS.items():
                assert float(m[k].max()) < bound, (site, fmt, form, k, m[k].tolist(), bound)
    assert not split.overflowed()


# ---- (b) the boundary -------------------------------------------------------------------------------------------------------------------------------------------
def _stem_bits(target):
    net, _ = R.stem_net_at(target)
    fast = _fast(("stem_at", target), None, FastPolicyNet, net)
    x = _planes()[0]
    with torch.no_grad():
        y64 = Emulated(net, "fp16", n_blocks=0, device="cuda").tower(x)
    out = []
    for fmt, planes in _planes()[1]:
        for form, flag, _ in FORMS:
            fast.force_wgb = flag
            out.append(((fmt, form), _tower_bits(fast, planes, "fp16")))
            fast.force_wgb = 0
    return y64, out


def test_boundary_just_below_stays_finite():
    """stem_net_at(65400): the largest stem value is 1.8e-3 below 65520, 30 x the f32 accumulation error (test_nnref.py): the kernel's stem output is finite and
    is the emulation's f16 bits within MIN_IDENTICAL / MAX_EXCESS of the k = 0 truncated tower"""
    y64, runs = _stem_bits(65400.0)
    assert bool(torch.isfinite(y64).all()) and float(y64.max()) > 65300
    ref = _ref_bits(y64, "fp16")
    for key, got in runs:
        assert int(got.max()) < F16_INF_BITS, key
        mu, ident, ex = _ulps(got, ref, "fp16")
        print("65400", key, "max ulp %d identical %.6f excess %.2e" % (mu, ident, ex))
        assert ident >= MIN_IDENTICAL["fp16"] and ex <= MAX_EXCESS["fp16"], (key, mu, ident, ex)


def test_boundary_just_above_is_inf_where_the_rounding_says_so():
    """stem_net_at(65650): 2.0e-3 above 65520: +inf in the kernel's stem output at exactly the elements where round_to gives inf, no NaN, and the finite
    elements are the emulation's bits as far as MIN_IDENTICAL asks"""
    y64, runs = _stem_bits(65650.0)
    inf = torch.isinf(y64)
    assert bool(inf.any()) and not bool(torch.isnan(y64).any())
    ref = _ref_bits(torch.where(inf, torch.zeros_like(y64), y64), "fp16")
    for key, got in runs:
        assert torch.equal(got == F16_INF_BITS, inf), (key, int((got == F16_INF_BITS).sum()), int(inf.sum()))
        assert int(got.max()) == F16_INF_BITS, key                                 # nothing above inf's pattern: no NaN
        same = (got == ref)[~inf].double().mean()
        assert float(same) >= MIN_IDENTICAL["fp16"], (key, float(same))
    print("65650: %d of %d stem outputs are +inf in the kernel and in the emulation" % (int(inf.sum()), inf.numel()))


# ---- (c) out of range: record, then hold ----------------------------------------------------------------------------------------------------------------------
def _count(t):
    t = _flat(t)
    return "+inf %d -inf %d nan %d" % (int((t == float("inf")).sum()), int((t == float("-inf")).sum()), int(t.isnan().sum()))


# What the kernels do out of range, recorded on MI355X (identical in the automatic and both forced workgroup forms, on both input formats; elements of the four
# boards together; DESIGN.md has the table).  SILENT: the nets whose bad boards come out FINITE — the case this file exists for.  The convolution behind a
# +inf gives NaN (inf - inf) with the sign bit set, and the kernels' ReLU is an integer maximum with 0 on the bit pattern, which makes 0 of such a NaN:
#   stem           every board: the stem stores +inf, block 0 erases it: tower output, logits, probabilities finite (value 1 / 0.0978 / 0.0978 / 0.0978)
#   block9.t       every board: 256 +inf left in the tower output, conv_p1 makes NaN of them and its ReLU 0: logits and probabilities finite, value finite
#   one_bad_board  board 0 (block9.t): 1149 +inf in its tower output, logits, probabilities and value (0.252) finite
#   block15.out    7904 +inf in the tower output -> logits 612 +inf, 623 -inf, 8474 NaN -> every probability NaN, value NaN
#   block18.out    1914 +inf in the tower output -> logits 1039 +inf, 955 -inf, 8810 NaN -> every probability NaN, value NaN / 1 / 1 / 1
#   p1             tower output finite -> logits 412 +inf, 481 -inf, 17795 NaN -> every probability NaN, value finite (the value head does not read p1)
# The range flag (overflowed()) is what catches all nine; the softmax spreads a +inf / NaN logit over its whole row, but nothing spreads what the ReLU erased.
SILENT = ("stem", "block9.t", "one_bad_board")


def _hold(case, fast, ref, record=None):
    """(c) for one net, in every form and input format: the kernel is never non-finite on a board that is good in the emulation; on the emulation's bad boards it
    is non-finite too, except for the SILENT nets, where it is finite on every board (the record above); the good boards keep the bounds of (a); and the
    network's range flag is set by every one of these forwards that had a bad board in it."""
    bad = ref.bad.tolist()
    for fmt, planes in _planes()[1]:
        for form, flag, _ in FORMS:
            fast.overflowed()
            fast.force_wgb = flag
            y, l, pi, v = _run(fast, planes)
            fast.force_wgb = 0
            kbad = (~(torch.isfinite(pi).all(1) & torch.isfinite(v).all(1))).tolist()
            if record is not None:
                record.append("%-13s %-7s %-4s tower[%s] logits[%s] probs[%s] value %s  bad boards: kernel %s emulation %s" % (
                    case, fmt, form, _count(y), _count(l), _count(pi), ["%.3g" % t for t in v.view(-1).tolist()], [b for b in range(R.N_BOARDS) if kbad[b]],
                    [b for b in range(R.N_BOARDS) if bad[b]]))
            assert not any(k and not b for k, b in zip(kbad, bad)), "%s %s %s: bad boards of the kernel %s, of the emulation %s" % (case, fmt, form, kbad, bad)
            assert kbad == ([False] * R.N_BOARDS if case in SILENT else bad), "%s %s %s: bad boards of the kernel %s, of the emulation %s" % (case, fmt, form, kbad, bad)
            _check_boards((case, fmt, form), ref, y, l, pi, v, boards=[b for b in range(R.N_BOARDS) if not bad[b]])
            assert fast.overflowed() is any(bad), "%s %s %s: range flag against bad boards %s" % (case, fmt, form, bad)


@pytest.mark.parametrize("case", OUT_CASES)
def test_out_of_range_record_then_hold(case):
    """net_at(site, 2 x 65504) and one_bad_board(): the emulation's bad boards (a non-finite probability or value; round_to overflows to inf, torch carries inf
    and NaN through every ReLU and the heads) against what the kernel returns, in every form and input format: see SILENT for the record — three of the six nets
    come out finite on their bad boards — and _hold for what is asserted.  The good boards of the same batch stay within the per-board bounds of (a): in
    one_bad_board's two-board form the bad board shares a workgroup and the softmax exchange buffer with a good one.  Every net sets the range flag."""
    ref = _ref(case, R.OUT_OF_RANGE)
    assert bool(ref.bad.any()) and (case != "one_bad_board" or ref.bad.tolist() == [b == R.one_bad_board()[1] for b in range(R.N_BOARDS)])
    record = []
    try:
        _hold(case, _fast(case, R.OUT_OF_RANGE), ref, record)
    finally:
        print("\n".join(record))


# ---- (d) teeth --------------------------------------------------------------------------------------------------------------------------------------------------
class _Saturating(Emulated):
    """the mutant: an emulation that clamps to +-65504 where the conversion overflows — what a kernel that quietly saturated would compute"""

    def r(self, x):
        return torch.clamp(round_to(x, self.op), -R.F16_MAX, R.F16_MAX)


def test_out_of_range_check_has_teeth():
    """(c) with the saturating emulation in the reference's place fails on every out-of-range net: that emulation has no bad board, so the kernel's NaN boards
    are one too many, its finite boards (SILENT) are nowhere near the saturated values, and the range flag is set although no board is bad — a kernel that
    clamped instead of overflowing would not pass (c) as "in range" either"""
    for case in OUT_CASES:
        mutant = _Reference(_net(case, R.OUT_OF_RANGE), _Saturating)
        assert not bool(mutant.bad.any()), case
        with pytest.raises(AssertionError):
            _hold(case, _fast(case, R.OUT_OF_RANGE), mutant)


# ---- the range flag ---------------------------------------------------------------------------------------------------------------------------------------------
def _search_and_check(fast, planes):
    """a SelfPlayEngine search of 2 simulations on four boards whose every network call evaluates the four fixture boards, then check_errors()"""
    eng = SelfPlayEngine(fast, {"C": 2, "num_searches": 2}, R.N_BOARDS, chess960=False, planes_dtype="bits128")
    try:
        eng.new_games([-1] * R.N_BOARDS)
        eng.search(evaluator=lambda _: eng.evaluate(planes))
        return eng.check_errors()
    finally:
        eng.close()


@pytest.mark.parametrize("case", OUT_CASES)
def test_search_on_an_overflowing_network_raises(case):
    """every out-of-range net and one_bad_board, in every form: check_errors() after the search raises and names the way out; the flag is cleared by that"""
    fast = _fast(case, R.OUT_OF_RANGE)
    fast.overflowed()
    for _, planes in _planes()[1]:
        for form, flag, _ in FORMS:
            fast.force_wgb = flag
            try:
                with pytest.raises(ValueError, match='use operands="bf16" or SplitPolicyNet'):
                    _search_and_check(fast, planes)
            finally:
                fast.force_wgb = 0
            assert fast.overflowed() is False, (case, form)


@pytest.mark.parametrize("case", R.SITES + ("base",))
def test_search_in_range_does_not_raise(case):
    fast = _fast(case, R.IN_RANGE if case != "base" else None)
    for _, planes in _planes()[1]:
        for form, flag, _ in FORMS:
            fast.force_wgb = flag
            try:
                st = _search_and_check(fast, planes)
            finally:
                fast.force_wgb = 0
            assert st["boards_error"] == 0 and fast.overflowed() is False, (case, form)


def test_flag_is_sticky_until_read_and_bf16_has_none():
    """one overflowing forward, then healthy ones: overflowed() is True once, then False; logits (no softmax to spread an inf over the row) are flagged too;
    the same net on bf16 operands (f32's range) is finite and never flagged"""
    net, bad, _ = R.one_bad_board()
    fast = _fast("one_bad_board", R.OUT_OF_RANGE)
    bits = _planes()[1][1][1]
    good = bits[[b for b in range(R.N_BOARDS) if b != bad]].contiguous()
    fast.overflowed()
    with torch.no_grad():
        fast(good); fast(good, inference=False)
        assert fast.overflowed() is False
        fast(bits); fast(good); fast(good)
        assert fast.overflowed() is True and fast.overflowed() is False
        fast(good)
        assert fast.overflowed() is False
        fast(bits[bad:bad + 1].contiguous(), inference=False)
        assert fast.overflowed() is True
        p1 = _fast("p1", R.OUT_OF_RANGE)
        p1.overflowed()
        l, v = p1(bits, inference=False)
        assert bool(torch.isfinite(v).all()) and not bool(torch.isfinite(l).all())           # the value head does not read p1: the logits alone carry it
        assert p1.overflowed() is True
        for case in ("stem", "p1"):
            b16 = FastPolicyNet(R.net_at(case, R.OUT_OF_RANGE), device="cuda")
            pi, v = b16(bits)
            assert bool(torch.isfinite(pi).all()) and bool(torch.isfinite(v).all()) and b16.overflowed() is False
            assert _search_and_check(b16, bits)["boards_error"] == 0


@pytest.mark.parametrize("site", R.SPLIT_SITES)
def test_split_out_of_range_is_flagged(site):
    """SplitPolicyNet(operands="fp16") on split_net_at(site, 2 x 65504): the split kernels take the ReLU in f32 and pack the hi image then, so a board is bad
    when its largest POSITIVE value at the site reaches 65520 (all four boards, by more than 1.5 x: test_nnref.py).  Recorded on MI355X, every form and
    format: p1 gives NaN probabilities on all four boards; block9.t, block15.out and block18.out come out FINITE on all four (hi = inf, lo = NaN, the
    products NaN, and the f32 ReLU — an integer maximum with 0 — erases them): silent.  The range flag is set in every case, the search raises, and the bf16
    split network (f32's range) on the same net does neither."""
    net = R.split_net_at(site, R.OUT_OF_RANGE)
    split = _fast(("split", site), R.OUT_OF_RANGE, SplitPolicyNet, copy.deepcopy(net))
    split.overflowed()
    for fmt, planes in _planes()[1]:
        for form, _, flag in FORMS:
            split.force_wgb = flag
            try:
                with torch.no_grad():
                    pi, v = (t.clone() for t in split(planes, inference=True))
                kbad = (~(torch.isfinite(pi).all(1) & torch.isfinite(v).all(1))).tolist()
                print("split %-11s %-7s %-4s probs[%s] value %s" % (site, fmt, form, _count(pi), ["%.3g" % t for t in v.view(-1).tolist()]))
                assert kbad == [site == "p1"] * R.N_BOARDS, (site, fmt, form, kbad)
                assert split.overflowed() is True and split.overflowed() is False
                if fmt == "bits128":
                    with pytest.raises(ValueError, match='use operands="bf16" or SplitPolicyNet'):
                        _search_and_check(split, planes)
            finally:
                split.force_wgb = 0
    sb = SplitPolicyNet(copy.deepcopy(net), device="cuda")
    bits = _planes()[1][1][1]
    with torch.no_grad():
        pi, v = sb(bits)
        assert bool(torch.isfinite(pi).all()) and bool(torch.isfinite(v).all()) and sb.overflowed() is False
    assert _search_and_check(sb, bits)["boards_error"] == 0
