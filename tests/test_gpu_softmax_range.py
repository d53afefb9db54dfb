"""The `inference=True` probability row — the one thing the search reads from a network — on peaked logits, against fp64.

Networks of tests/softmaxref.py (probe_net: identity tower, conv_p2 = a designed matrix on grids every operand format holds) give every kernel path the SAME logits,
exactly, so what is compared is the softmax epilogue alone: k_heads16_bf16 (FastPolicyNet bf16 and fp16), k_policy_head (FastPolicyNet bf16, fused_heads=False) and
the fused heads of k_tower_split (SplitPolicyNet bf16 and fp16, one- and two-board workgroups).  Per family and case:
  harness   inference=False returns the designed logits bit for bit (else the probe is wrong, not the softmax);
  accuracy  every entry: |p - p64| <= (|d| + 64) * 2^-23 * p64 + 1.5 * 2^-149 (softmaxref.py derives it);
  zero set  p64 >= 2^-148 => p != 0;  p64 < 2^-152 => p == 0 (no entry of any case lies between);
  rows      |sum p - 1| <= 64 * 2^-23, all finite, equal logits give bit-equal probabilities within a row, and a board type's row is the same bits in every batch
            size (1, 2, 3, 8; #CUs + 1 for the split forms), workgroup form and input format;
then what the tree makes of such rows (one k_search_step per position of softmaxref.POSITIONS): children = the legal actions with p64 >= 2^-148, priors inside the
interval the bound allows.
Before softmax_exp (sz_nn_common.h) the three epilogues took __expf, one v_exp_f32, which delivers nothing below 2^-126: every kept entry more than 87.34 below the
row maximum came out 0 (profiles/softmax_range.txt has the table of both libraries) and a position whose legal moves all sat there had no legal mass left (0 / 0 in k_search_step)."""
import copy
import functools

import numpy as np
import pytest
import torch

from sigma_zero_amd import _native as N
from sigma_zero_amd.fastnet import FastPolicyNet, SplitPolicyNet, planes_nchw_to_nhwc128
from sigma_zero_amd.selfplay import SelfPlayEngine

import softmaxref as R
from test_gpu_network import _pack_bits128

pytestmark = pytest.mark.gpu

FAMILIES = ("fast_bf16", "fast_fp16", "fast_bf16_unfused", "split_bf16", "split_fp16")
ZONES = ("normal", "subnormal", "below")


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _forms(family):
    return (("wgb1", N.SZ_NN_SPLIT_WGB1), ("wgb2", N.SZ_NN_SPLIT_WGB2)) if family.startswith("split") else (("auto", 0),)


def _batches(family):
    return (1, 2, 3, 8) + ((_n_cu() + 1,) if family.startswith("split") else ())


@functools.lru_cache(maxsize=None)
def _probe(case):
    return R.probe_net(R.case(case))


@functools.lru_cache(maxsize=None)
def _network(family, case):
    net = copy.deepcopy(_probe(case))                     # SplitPolicyNet moves its module to the device
    if family.startswith("split"):
        return SplitPolicyNet(net, device="cuda", operands=family[6:])
    fast = FastPolicyNet(net, device="cuda", operands="fp16" if family == "fast_fp16" else "bf16")
    fast.fused_heads = family != "fast_bf16_unfused"
    return fast


@functools.lru_cache(maxsize=None)
def _inputs(case, B):
    """((format, planes), ...) of a batch of B boards of the case, board types in turn"""
    img = planes_nchw_to_nhwc128(R.probe_planes(R.types_of(case, B)).cuda())
    return (("nhwc128", img), ("bits128", _pack_bits128(img.float())))


def _forward(net, planes, form=0):
    net.force_wgb = form
    try:
        with torch.no_grad():
            logits = net(planes, inference=False)[0].clone()
            probs = net(planes, inference=True)[0].clone()
    finally:
        net.force_wgb = 0
    return logits, probs


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _canonical(family, case):
    """(logits, probabilities) [K, 4672] on the device of one board of every type: first form, bit-packed input"""
    K = R.case(case).off.shape[0]
    return _forward(_network(family, case), _inputs(case, K)[1][1], _forms(family)[0][1])


@pytest.mark.parametrize("case", R.CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_probability_rows_against_fp64(family, case):
    ref = R.reference(case)
    K = ref.d.shape[0]
    logits, probs = _canonical(family, case)
    assert torch.equal(logits.cpu().double(), ref.logits), "harness: the logits are not the designed ones"
    m = R.measure(probs, ref, list(range(K)))
    print("%-18s %-12s %s" % (family, case, m))                        # the figures first, then the assertions
    R.check(probs, ref, list(range(K)), (family, case))
    R.equal_logits_equal_bits(probs, ref.logits)
    net = _network(family, case)
    for form, flag in _forms(family):
        for B in _batches(family):
            types = torch.tensor(R.types_of(case, B), device="cuda")
            for fmt, planes in _inputs(case, B):
                l, p = _forward(net, planes, flag)
                assert torch.equal(_bits(l), _bits(logits[types])), (family, case, form, B, fmt, "logits")
                assert torch.equal(_bits(p), _bits(probs[types])), (family, case, form, B, fmt, "a board's row depends on its batch, form or input format")
    if hasattr(net, "overflowed"):
        assert net.overflowed() is False


def test_equal_rows_of_different_networks_and_boards_are_equal_bits():
    """the all-equal row (flat, type 0) is 1 / 4672 in every entry, in every family: exp(0) = 1 exactly, the sum 4672 exactly, one rounding in 1 / 4672"""
    want = torch.full((R.N_ACTIONS,), 1.0 / 4672, dtype=torch.float64).float()
    for family in FAMILIES:
        p = _canonical(family, "flat")[1][0].cpu()
        assert torch.equal(_bits(p), _bits(want)), family


# ---- record: torch on the device on the same logits / boards, and every family, per zone (printed, not asserted) --------------------------------------------------
def record_table(cases=R.CASES):
    """lines "site zone worst-error/bound wrongly-zero" over all cases: the kernels' families, torch.softmax on the device on the designed logits, and the fp32
    module on the device on the same boards"""
    sites = {f: (lambda c, f=f: _canonical(f, c)[1]) for f in FAMILIES}
    sites["torch.softmax (device)"] = lambda c: torch.softmax(R.reference(c).logits.float().cuda(), 1)

    def module(c):
        K = R.case(c).off.shape[0]
        with torch.no_grad():
            return copy.deepcopy(_probe(c)).cuda()(R.probe_planes(R.types_of(c, 8)).cuda(), inference=True)[0][:K]
    sites["policyNN.cuda()"] = module
    lines = ["%-24s %10s %10s %10s %14s %14s %10s" % ("site", "normal", "subnormal", "below", "wrongly zero", "wrongly kept", "non-finite")]
    for site, fn in sites.items():
        worst, wz, wk, nf = dict.fromkeys(ZONES, 0.0), 0, 0, 0
        for c in cases:
            p = fn(c)
            m = R.measure(p, R.reference(c), list(range(p.shape[0])))
            worst = {z: max(worst[z], m[z]) for z in ZONES}
            wz, wk, nf = wz + m["wrongly_zero"], wk + m["zero"], nf + int((~torch.isfinite(p)).sum())
        lines.append("%-24s %10.3g %10.3g %10.3g %14d %14d %10d" % ((site,) + tuple(worst[z] for z in ZONES) + (wz, wk, nf)))
    return lines


def test_record_of_torch_on_the_device():
    """printed only (run with -s): worst error / bound per zone, entries that are 0 although p64 >= 2^-148, entries that are not 0 although p64 < 2^-152"""
    print("\n" + "\n".join(record_table()))


# ---- what the tree makes of it ------------------------------------------------------------------------------------------------------------------------------------
BOARDS = tuple((pos, kind) for pos in R.POSITIONS for kind in "ab")


def _root_children(policy):
    """one search step on the eight boards (position x case a / b) with `policy` [8, 4672] as the network's answer for the roots"""
    eng = SelfPlayEngine(None, {"C": 2, "num_searches": 2}, len(BOARDS), learning=False)
    try:
        for b, (pos, _) in enumerate(BOARDS):
            eng.upload_game(b, R.position_game(pos))
        eng.begin()
        eng.step(policy.float().contiguous(), torch.zeros(len(BOARDS), device="cuda"))
        action, _, n_child, prior, _ = eng.root_children()
        st = eng.check_errors()
        assert st["boards_error"] == 0
        return action, n_child, prior
    finally:
        eng.close()


@pytest.mark.parametrize("source", FAMILIES + ("reference",))
def test_children_and_priors_of_the_tree(source):
    """k_search_step keeps a legal move iff p / total != 0: the children are the legal actions with p64 >= 2^-148 in action order, every prior lies in
    [lo_a / sum hi, hi_a / sum lo] (the bound pushed through p[a] / sum of the legal p, widened by 2^-22 for the engine's own f32 sum and division), and in case (b)
    — the maximum on an illegal action, every legal move 89 to 100 below it — the child count is the full legal count and every prior is finite.  `reference`:
    p64 rounded to f32 as the policy, the engine alone."""
    rows = []
    for pos, kind in BOARDS:
        name = "%s_%s" % (pos, kind)
        rows.append(R.reference(name).p64[0].float().cuda() if source == "reference" else _canonical(source, name)[1][0])
    action, n_child, prior = _root_children(torch.stack(rows))
    for b, (pos, kind) in enumerate(BOARDS):
        legal = list(R.legal_actions(pos))
        kept, lo, hi = R.expected_children(R.reference("%s_%s" % (pos, kind)), 0, legal)
        k = int(n_child[b])
        pr = torch.from_numpy(prior[b, :k].astype(np.float64))
        print("%-10s %-9s %s: %3d children of %3d legal (expected %3d), priors %.3g .. %.3g" % (source, pos, kind, k, len(legal), len(kept), float(pr.min()) if k else 0, float(pr.max()) if k else 0))
        assert k == len(kept) and action[b, :k].tolist() == kept, (source, pos, kind, k, len(kept))
        assert bool(torch.isfinite(pr).all()), (source, pos, kind, "non-finite priors")
        assert bool((pr >= lo).all() and (pr <= hi).all()), (source, pos, kind, "a prior outside its interval")
        if kind == "b":
            assert k == len(legal)
