"""tests/softmaxref.py on the CPU: the cases hold what they are designed to hold, the fp32 module reproduces the designed logits bit for bit and passes the softmax
bound with room, and mutants of the reference fail it."""
import numpy as np
import pytest
import torch

import softmaxref as R


@pytest.fixture(scope="module")
def module_rows():
    """{case: (logits, probabilities) of the fp32 CPU module on one board of every type}"""
    out = {}
    with torch.no_grad():
        for name in R.CASES:
            c = R.case(name)
            net, x = R.probe_net(c), R.probe_planes(range(c.off.shape[0]))
            out[name] = (net(x, inference=False)[0], net(x, inference=True)[0])
    return out


def test_designs_are_on_the_grids_and_out_of_the_band():
    for name in R.CASES:
        c, ref = R.case(name), R.reference(name)
        W = np.concatenate([c.wsq, c.off.T], 1)
        assert np.abs(W).max() <= R.W_LIMIT and np.all(W * 4 == np.round(W * 4)), name
        assert np.all(c.b / R.B_GRID == np.round(c.b / R.B_GRID)) and float(ref.logits.abs().max()) < 2 ** 14, name
        assert torch.equal(ref.logits.float().double(), ref.logits), name                 # every designed logit is an f32 number
        assert int(R.zones(ref)["band"].sum()) == 0, name
    assert R.case("deep").blocks == 19 and all(R.case(n).blocks == 0 for n in R.CASES if n != "deep")


def test_zones_maxima_and_special_rows():
    """what the issue's table asks the cases to hold between them"""
    for name in ("zones", "minus1e4", "argmax0", "argmax1", "deep", "halves0", "halves1") + tuple(n for n in R.POSITION_CASES if n.endswith("_a")):
        ref, z = R.reference(name), R.zones(R.reference(name))
        for k in range(ref.d.shape[0]):                                                 # all three zones in the same row
            assert all(bool(z[zone][k].any()) for zone in ("normal", "subnormal", "zero")), (name, k)
    for name in ("zones", "minus1e4", "argmax0", "argmax1", "deep", "halves0", "halves1", "flat"):
        ref, z = R.reference(name), R.zones(R.reference(name))
        n = int((z["subnormal"] & (ref.d < R.D_FLUSH)).sum())
        print("%-9s kept entries below d = %.2f: %d of %d" % (name, R.D_FLUSH, n, ref.d.numel()))
        assert n >= 300, (name, n)
    for name, squares in (("argmax0", R.ARGMAX_SQUARES), ("argmax1", R.ARGMAX_SQUARES[::-1]), ("deep", (32, 0, 63, 31))):
        ref = R.reference(name)
        assert ref.logits.argmax(1).tolist() == [pl * 64 + sq for pl, sq in zip(R.ARGMAX_PLANES, squares)], name
        assert bool(((ref.d == 0).sum(1) == 1).all())
    for name, sq in (("halves0", 3), ("halves1", 35)):                                   # the maximum in one wave's half, nearly all of the sum in the other's
        ref = R.reference(name)
        assert ref.logits.argmax(1).tolist() == [5 * 64 + sq] * 2
        other = (torch.arange(R.N_ACTIONS) % 64 // 32 != sq // 32)
        assert float(ref.p64[:, other].sum(1).min()) > 0.995 and float(ref.S.min()) > 100
    flat = R.reference("flat")
    assert bool((flat.logits[0] == flat.logits[0, 0]).all())                             # a row of all-equal logits
    assert ((flat.d == 0).sum(1)).tolist() == [4672, 2560, 2560, 2560] and float(flat.S.min()) >= 2560          # thousands tied at the maximum
    e2 = flat.p64[2] * flat.S[2]                                                         # type 2: exp(d) is a subnormal number, p64 = exp(d) / 2560 is 0 in f32
    assert bool(((e2 >= R.P_KEPT) | (e2 == 1))[40 * 64:].all()) and bool((flat.p64[2, 40 * 64:] < R.P_ZERO).all())
    m = R.reference("minus1e4")
    assert float(m.logits.max()) < -9.8e3 and float(m.logits.min()) > -1.02e4            # a row whose logits are all about -1e4


def test_position_rows():
    seen_black = False
    for pos in R.POSITIONS:
        g = R.position_game(pos)
        legal = list(R.legal_actions(pos))
        assert len(legal) == len(set(legal)) > 0
        seen_black |= not g.board.turn
        a, b = R.reference(pos + "_a"), R.reference(pos + "_b")
        za = R.zones(a)
        assert int(a.logits[0].argmax()) in legal                                        # (a) the maximum on a legal move, the others over all three zones
        assert all(bool(za[zone][0, legal].any()) for zone in ("normal", "subnormal", "zero")), pos
        kept, lo, hi = R.expected_children(a, 0, legal)
        assert 0 < len(kept) < len(legal) and bool((lo <= hi).all())
        assert int(b.logits[0].argmax()) not in legal                                    # (b) the maximum on an illegal action, every legal move at d in [-100, -89]
        assert float(b.d[0, legal].max()) <= -89 and float(b.d[0, legal].min()) >= -100
        assert bool((b.p64[0, legal] >= R.P_KEPT).all()) and bool((b.p64[0, legal] < R.P_NORMAL).all())
        kept, lo, hi = R.expected_children(b, 0, legal)
        assert kept == legal and bool(torch.isfinite(hi).all()) and bool((lo > 0).all())
    assert seen_black and len(R.legal_actions("moves218")) == 218


def test_fp32_module_reproduces_the_designed_logits(module_rows):
    for name, (logits, _) in module_rows.items():
        assert logits.dtype == torch.float32 and torch.equal(logits.double(), R.reference(name).logits), name


def test_fp32_module_softmax_passes_with_room(module_rows):
    """torch's fp32 softmax on the CPU keeps f32's subnormals.  Where the relative term of the bound is what counts (p64 >= 2^-126) its worst error / bound is 0.08
    on these cases and stays under 0.25.  Below 2^-126 no evaluation can: a correctly rounded f32 value is up to half a quantum off, a third of the 1.5 quanta the
    bound allows there (test_reference_passes_its_own_check...), and torch rounds twice (the exponential, then the product with 1 / S): 0.58 measured, held to the
    bound itself."""
    worst = {"normal": 0.0, "subnormal": 0.0, "below": 0.0}
    for name, (_, p) in module_rows.items():
        ref = R.reference(name)
        m = R.check(p, ref, list(range(p.shape[0])), name)
        R.equal_logits_equal_bits(p, ref.logits)
        worst = {k: max(v, m[k]) for k, v in worst.items()}
        print("%-12s %s" % (name, m))
    assert worst["normal"] < 0.25 and max(worst.values()) <= 1.0, worst


def test_reference_passes_its_own_check_and_the_engine_interval_holds_it():
    """p64 rounded to f32 once: far inside the relative bound, and at most half a quantum off below 2^-126 (1 / 3 of the absolute term)"""
    for name in R.CASES:
        ref = R.reference(name)
        m = R.check(ref.p64.float(), ref, list(range(ref.d.shape[0])), name)
        assert m["normal"] < 0.01 and max(m["subnormal"], m["below"]) <= 1.0 / 3, (name, m)
    for pos in R.POSITIONS:
        for kind in "ab":
            ref, legal = R.reference("%s_%s" % (pos, kind)), list(R.legal_actions(pos))
            kept, lo, hi = R.expected_children(ref, 0, legal)
            p = ref.p64[0, kept]
            prior = p / p.sum()
            assert bool((lo <= prior).all() and (prior <= hi).all())


# the cases on which each mutant must fail: where its error shows
MUTANT_FAILS = {"flush": R.CASES, "half_max": ("halves0", "halves1", "zones"), "padded_planes": ("flat", "minus1e4"), "bf16": R.CASES}


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutants_of_the_reference_fail(mutant):
    for name in MUTANT_FAILS[mutant]:
        ref = R.reference(name)
        p = R.MUTANTS[mutant](ref.logits)
        with pytest.raises(AssertionError):
            R.check(p, ref, list(range(p.shape[0])), (mutant, name))
    if mutant == "flush":                                                                # and what it does to the tree: case (b) loses every child
        for pos in R.POSITIONS:
            ref, legal = R.reference(pos + "_b"), list(R.legal_actions(pos))
            assert float(R.MUTANTS[mutant](ref.logits)[0, legal].max()) == 0.0
