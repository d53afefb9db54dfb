"""The policy softmax on peaked logits: a probe network whose logits are known exactly, the cases, and the fp64 reference with its bound (no GPU).

The probe (probe_net): every BatchNorm is the identity (mean 0, var 1, gamma 1, beta 0, eps 1e-30: the fold of fastnet._fold_bn is exactly 1 in double), the stem copies
input plane c to channel c through its centre tap, the tower passes x through (no block, or 19 blocks of zero weights: relu(0 + x) = x), conv_p1 is the 256 x 256
identity, conv_p2 is W [73, 256] with bias b [73].  A board (planes) has plane `pos` set at square `pos` for the 64 squares and, for board type k < 55, plane 64 + k
set on every square, so
    logit[co, pos] = W[co, pos] + W[co, 64 + k] + b[co]
W is kept on multiples of 0.25 with |W| <= 60 (bf16 holds them, and split-f16 packs w * 2^10 into f16: below 63.97) and b on multiples of 2^-10 with
|logit| < 2^14: every sum is exact in f32 in any order, so the fp32 module and every kernel return the designed logits bit for bit and what is left to compare is
the softmax alone.

A Case is (W's square part [73, 64], the per-type plane offsets [K, 73], b [73]); CASES is the table.  reference(case) gives, per board type, the designed logits,
d = logit - row maximum, p64 = the fp64 softmax, and S = sum exp(d).  Zones of an entry: normal (p64 >= 2^-126), subnormal (2^-148 <= p64 < 2^-126), zero
(p64 < 2^-152).  The band between, p64 or exp(d) = p64 * S in [2^-152, 2^-148), is where correctly rounded fp32 evaluations legitimately disagree on 0 against one
quantum: the designs are redrawn until no entry of any case is in it (test_softmaxref.py asserts that).

The bound (measure / check):  |p - p64| <= bound(d) * p64 + 1.5 * 2^-149,  bound(d) = (|d| + 64) * 2^-23.  Derived, not tuned: the exponential's argument carries
two roundings of |d| * 2^-24 each (l - max, and the product with log2 e), which the exponential turns into relative errors of the same size: |d| * 2^-23 together;
the constant 64 * 2^-23 covers an exponential of 2 ulp, the f32 sum of at most about 90 positive terms per partial (20 per lane, the shuffles, 64 partials in the split
kernel), the reciprocal and the final product; the absolute term is the two roundings at subnormal granularity (the exponential's and the product's, half a quantum
each, and half a quantum of slack for the first one carried through 1 / S <= 1).
"""
import collections
import functools

import numpy as np
import torch

import nnref

Q = 2.0 ** -149                       # f32's quantum below 2^-126
P_NORMAL = 2.0 ** -126
P_KEPT = 2.0 ** -148                  # from here on a probability is not 0 in any correctly rounded evaluation
P_ZERO = 2.0 ** -152                  # below this it is 0 in every one
D_FLUSH = -87.34                      # exp(d) < 2^-126 below this: what one v_exp_f32 does not deliver
ROW_SUM = 64 * 2.0 ** -23
N_ACTIONS, N_PLANES, N_TYPES = 4672, 73, 55
W_LIMIT, W_GRID, B_GRID = 60.0, 0.25, 2.0 ** -10

Case = collections.namedtuple("Case", "name wsq off b blocks")          # wsq [73, 64], off [K, 73], b [73] as float64 numpy arrays; blocks: 0 or 19
Reference = collections.namedtuple("Reference", "logits d p64 S")       # [K, 4672] double tensors, S [K, 1]


def bound(d):
    return (d.abs() + 64.0) * 2.0 ** -23


def interval(p64, d):
    """the fp64 interval the bound allows a probability: (lo, hi), lo clamped at 0"""
    tol = bound(d) * p64 + 1.5 * Q
    return (p64 - tol).clamp_min(0.0), p64 + tol


def design_logits(case):
    """[K, 4672] double: the logits the case is designed to give, board type by board type (flatten order plane * 64 + square)"""
    l = case.wsq[None, :, :] + (case.off + case.b[None, :])[:, :, None]
    return torch.from_numpy(l.reshape(case.off.shape[0], N_ACTIONS).copy())


def reference_of_logits(logits):
    logits = logits.double()
    d = logits - logits.max(1, keepdim=True).values
    e = torch.exp(d)
    S = e.sum(1, keepdim=True)
    return Reference(logits, d, e / S, S)


def zones(ref):
    """{"normal", "subnormal", "zero", "band"}: boolean masks [K, 4672]"""
    p, e = ref.p64, ref.p64 * ref.S
    band = ((p >= P_ZERO) & (p < P_KEPT)) | ((e >= P_ZERO) & (e < P_KEPT))
    return {"normal": p >= P_NORMAL, "subnormal": (p >= P_KEPT) & (p < P_NORMAL), "zero": p < P_ZERO, "band": band}


# ---- the designs --------------------------------------------------------------------------------------------------------------------------------------------------
def _grid(rs, lo, hi, shape):
    """uniform on the multiples of 0.25 in [lo, hi]"""
    return rs.randint(int(lo * 4), int(hi * 4) + 1, size=shape) / 4.0


def _clear_band(name, wsq, off, b, rs, fixed, lo, hi, blocks=0):
    """redraw the free entries of wsq (uniform on the grid in [lo, hi]) that put an entry of any board type into the band, until there is none"""
    for _ in range(200):
        case = Case(name, wsq, off, b, blocks)
        bad = zones(reference_of_logits(design_logits(case)))["band"].any(0).view(N_PLANES, 64).numpy()
        if not bad.any():
            return case
        assert not (bad & fixed).any(), (name, "a designed entry is in the band")
        wsq[bad] = _grid(rs, lo, hi, int(bad.sum()))
    raise AssertionError("%s: the band did not empty" % name)


def _case_zones(name="zones", seed=1, shift=0.0, k=8, span=60.0, blocks=0):
    """random W over the whole grid range: every row has entries in all three zones, the maximum wherever it falls; b on the 2^-10 grid (shift: all about -1e4)"""
    rs = np.random.RandomState(seed)
    wsq, off = _grid(rs, -span, span, (N_PLANES, 64)), _grid(rs, -span, span, (k, N_PLANES))
    b = shift + rs.randint(-2048, 2049, size=N_PLANES) * B_GRID
    return _clear_band(name, wsq, off, b, rs, np.zeros((N_PLANES, 64), bool), -span, span, blocks)


ARGMAX_PLANES, ARGMAX_SQUARES = (0, 63, 64, 72), (0, 31, 32, 63)


def _case_argmax(name, seed, squares, blocks=0):
    """board type k has its maximum at plane ARGMAX_PLANES[k], square squares[k]: the first and last real planes, both sides of the fifth 16-channel tile; both waves of a
    board in k_heads16_bf16 and their first and last lanes.  The plane's offset of 40 lifts it over the others; the background in [-60, 0] spreads over the zones."""
    rs = np.random.RandomState(seed)
    wsq, off, fixed = _grid(rs, -60, 0, (N_PLANES, 64)), np.zeros((4, N_PLANES)), np.zeros((N_PLANES, 64), bool)
    for k, (pl, sq) in enumerate(zip(ARGMAX_PLANES, squares)):
        wsq[pl, sq], fixed[pl, sq], off[k, pl] = 20.0, True, 40.0
    return _clear_band(name, wsq, off, np.full(N_PLANES, 0.5 + B_GRID), rs, fixed, -60, 0, blocks)


def _case_halves(name, seed, square):
    """the maximum (one entry, plane 5) in one 32-square half, nearly all of the sum in the other: 2336 entries within 2 of the maximum there (S about 900), the
    maximum's own half 25 to 110 below.  Type 1 lowers the planes by up to 2 (not plane 5)."""
    rs = np.random.RandomState(seed)
    own = np.arange(64) // 32 == square // 32
    wsq, fixed = np.empty((N_PLANES, 64)), np.zeros((N_PLANES, 64), bool)
    wsq[:, own] = _grid(rs, -60, 25, (N_PLANES, 32))
    wsq[:, ~own] = _grid(rs, 48, 49.75, (N_PLANES, 32))
    wsq[5, square], fixed[5, square] = 50.0, True
    fixed[:, ~own] = True
    off = np.stack([np.zeros(N_PLANES), -_grid(rs, 0, 2, N_PLANES)])
    off[1, 5] = 0.0
    case = _clear_band(name, wsq, off, np.full(N_PLANES, -3 * B_GRID), rs, fixed, -60, 25)
    return case


def _case_flat():
    """type 0: all 4672 logits equal.  Types 1-3: 2560 entries tied at the maximum (S = 2560), the other 2112 at 90 (subnormal), 100 (exp(d) is a subnormal number,
    p64 = exp(d) / 2560 is below the band: exactly 0) and 120 (zero) below."""
    wsq, off = np.zeros((N_PLANES, 64)), np.zeros((4, N_PLANES))
    wsq[40:] = -60.0                                         # planes 40..72 sit 60 lower on every square; type 0 lifts them back
    off[0, 40:], off[1, 40:], off[2, 40:], off[3, 40:] = 60.0, -30.0, -40.0, -60.0
    return Case("flat", wsq, off, np.full(N_PLANES, 3.0 + B_GRID), 0)


# positions for the search (4): legal actions from the rules on the host
POSITIONS = collections.OrderedDict([
    ("start", None),
    ("moves218", "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"),
    ("promotion", "8/P7/8/8/8/8/7k/K7 w - - 0 1"),
    ("black", "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R b KQkq - 0 1"),
])
ILLEGAL_CANDIDATES = (72 * 64 + 63, 0, 64 * 64 + 32, 63 * 64 + 31, 5 * 64 + 3, 30 * 64 + 40)


def position_game(name):
    import sigma_zero_amd as sz
    return sz.ChessTensor(fen=POSITIONS[name]) if POSITIONS[name] else sz.ChessTensor()


@functools.lru_cache(maxsize=None)
def legal_actions(name):
    """legal actions of the position in ascending order (the mover's view), from the host rules"""
    return tuple(sorted(position_game(name).legal_action_indices()))


def _case_position(pos, kind, seed):
    """(a) the maximum on a legal move (the middle one of the list), the other legal moves in turn normal (d in [-85, -0.25]), subnormal ([-102, -88]) and zero
    ([-110, -106]); (b) the maximum on an illegal action, every legal move at d in [-100, -89].  The illegal actions are 70 to 110 below the maximum."""
    rs = np.random.RandomState(seed)
    legal = np.array(legal_actions(pos))
    w = _grid(rs, -60, -20, N_ACTIONS)
    fixed = np.zeros(N_ACTIONS, bool)
    fixed[legal] = True
    if kind == "a":
        top = legal[len(legal) // 2]
        rest = [a for a in legal if a != top]
        ranges = ((-85, -0.25), (-102, -88), (-110, -106))
        for i, a in enumerate(rest):
            w[a] = 50.0 + _grid(rs, *ranges[(i + 1) % 3], None)
    else:
        k = list(POSITIONS).index(pos)
        top = next(a for a in ILLEGAL_CANDIDATES[k:] + ILLEGAL_CANDIDATES[:k] if a not in set(legal.tolist()))
        fixed[top] = True
        w[legal] = 50.0 + _grid(rs, -100, -89, len(legal))
    w[top] = 50.0
    return _clear_band("%s_%s" % (pos, kind), w.reshape(N_PLANES, 64), np.zeros((1, N_PLANES)), np.full(N_PLANES, 5 * B_GRID), rs, fixed.reshape(N_PLANES, 64), -60, -20)


POSITION_CASES = tuple("%s_%s" % (p, k) for p in POSITIONS for k in "ab")
_BUILDERS = collections.OrderedDict([
    ("zones", lambda: _case_zones()),
    ("minus1e4", lambda: _case_zones("minus1e4", seed=2, shift=-1.0e4, k=2, span=50.0)),
    ("argmax0", lambda: _case_argmax("argmax0", 3, ARGMAX_SQUARES)),
    ("argmax1", lambda: _case_argmax("argmax1", 4, ARGMAX_SQUARES[::-1])),
    ("deep", lambda: _case_argmax("deep", 5, (32, 0, 63, 31), blocks=19)),
    ("halves0", lambda: _case_halves("halves0", 6, 3)),
    ("halves1", lambda: _case_halves("halves1", 7, 35)),
    ("flat", _case_flat),
])
for _i, _n in enumerate(POSITION_CASES):
    _BUILDERS[_n] = functools.partial(_case_position, _n.rsplit("_", 1)[0], _n[-1], 10 + _i)
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of_logits(design_logits(case(name)))


# ---- the probe ----------------------------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def probe_net(c):
    """policyNN (fp32, eval, on the CPU) that returns design_logits(c) for probe_planes(c, types)"""
    import sigma_zero_amd as sz
    torch.manual_seed(0)                                                 # the value head keeps its initial weights: it is not under test
    net = sz.policyNN({}).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.zero_(); m.running_var.fill_(1.0); m.weight.fill_(1.0); m.bias.zero_()
            m.eps = 1e-30
    net.conv1.weight.zero_()
    for ch in range(119):
        net.conv1.weight[ch, ch, 1, 1] = 1.0
    if c.blocks == 0:
        net = nnref.truncated(net, 0)
    else:
        assert c.blocks == len(net.resnet_blocks)
        for blk in net.resnet_blocks:
            blk.conv1.weight.zero_(); blk.conv2.weight.zero_()
    net.conv_p1.weight.copy_(torch.eye(256).view(256, 256, 1, 1))
    W = np.zeros((N_PLANES, 256))
    W[:, :64] = c.wsq
    W[:, 64:64 + c.off.shape[0]] = c.off.T
    assert c.off.shape[0] <= N_TYPES and np.abs(W).max() <= W_LIMIT and np.all(W / W_GRID == np.round(W / W_GRID)) and np.all(c.b / B_GRID == np.round(c.b / B_GRID))
    net.conv_p2.weight.copy_(torch.from_numpy(W).float().view(N_PLANES, 256, 1, 1))
    net.conv_p2.bias.copy_(torch.from_numpy(c.b).float())
    return net


def probe_planes(types):
    """[B, 119, 8, 8] float 0 / 1: board i is of type types[i]"""
    x = torch.zeros(len(types), 119, 64)
    x[:, torch.arange(64), torch.arange(64)] = 1.0
    for i, k in enumerate(types):
        x[i, 64 + int(k), :] = 1.0
    return x.view(len(types), 119, 8, 8)


def types_of(name, B):
    """board types of a batch of B boards of the case: 0 .. K-1 in turn"""
    return [i % case(name).off.shape[0] for i in range(B)]


# ---- the checks of a probability row against the reference --------------------------------------------------------------------------------------------------------
def measure(p, ref, rows):
    """p [B, 4672] f32 against ref's rows `rows` [B]: figures, nothing asserted.  {"normal" / "subnormal": worst error / tolerance in the zone, "zero": entries of the
    zero zone that are not 0, "wrongly_zero": entries with p64 >= 2^-148 that are 0, "row_sum": worst |sum - 1|, "finite": all finite}"""
    p = p.detach().cpu()
    p64, d = ref.p64[rows], ref.d[rows]
    z = {k: v[rows] for k, v in zones(ref).items()}
    pd = p.double()
    ratio = (pd - p64).abs() / (bound(d) * p64 + 1.5 * Q)
    ratio = torch.where(torch.isfinite(pd), ratio, torch.full_like(ratio, float("inf")))
    worst = lambda m: float(ratio[m].max()) if bool(m.any()) else 0.0
    return {"normal": worst(z["normal"]), "subnormal": worst(z["subnormal"]), "below": worst(~z["normal"] & ~z["subnormal"]),
            "zero": int((z["zero"] & (p != 0)).sum()), "wrongly_zero": int(((p64 >= P_KEPT) & (p == 0)).sum()),
            "row_sum": float((pd.sum(1) - 1).abs().max()), "finite": bool(torch.isfinite(p).all())}


def check(p, ref, rows, what=""):
    """the assertions on a network's probability rows; returns measure()'s figures"""
    m = measure(p, ref, rows)
    assert m["finite"], (what, "not finite", m)
    assert m["wrongly_zero"] == 0, (what, "%d entries with p64 >= 2^-148 are 0" % m["wrongly_zero"], m)
    assert m["zero"] == 0, (what, "%d entries with p64 < 2^-152 are not 0" % m["zero"], m)
    assert max(m["normal"], m["subnormal"], m["below"]) <= 1.0, (what, "error / bound", m)
    assert m["row_sum"] <= ROW_SUM, (what, "row sum", m)
    return m


def equal_logits_equal_bits(p, logits):
    """within every row, entries of equal logit have bit-equal probabilities; returns the number of pairs looked at"""
    p, logits = p.detach().cpu(), logits.cpu()
    order = logits.argsort(dim=1, stable=True)
    ls, ps = logits.gather(1, order), p.contiguous().view(torch.int32).gather(1, order)
    same = ls[:, 1:] == ls[:, :-1]
    assert bool((ps[:, 1:] == ps[:, :-1])[same].all()), "equal logits, different probabilities"
    return int(same.sum())


# ---- what the tree makes of a row ---------------------------------------------------------------------------------------------------------------------------------
def expected_children(ref, row, legal):
    """(actions kept, prior lo, prior hi) for a position whose network row is ref's row `row`: the legal actions with p64 >= 2^-148 in action order, and for each the
    fp64 interval of p[a] / sum over the legal p with every p anywhere in its interval(), widened by 2^-22 for the engine's own f32 sum and division"""
    legal = torch.tensor(sorted(legal))
    p64, d = ref.p64[row, legal], ref.d[row, legal]
    assert not bool(((p64 >= P_ZERO) & (p64 < P_KEPT)).any())
    keep = p64 >= P_KEPT
    lo, hi = interval(p64[keep], d[keep])
    sum_lo, sum_hi = float(lo.sum()), float(hi.sum())
    w = 2.0 ** -22
    prior_lo = lo / sum_hi * (1 - w)
    prior_hi = hi / sum_lo * (1 + w) if sum_lo > 0 else torch.full_like(hi, float("inf"))
    return legal[keep].tolist(), prior_lo, prior_hi


# ---- mutants of the reference: each is a softmax that is wrong in one way a kernel could be ----------------------------------------------------------------------------
def _f32(t):
    return t.float()


def mutant_flush(logits):
    """exp(d) below 2^-126 comes out as 0 (one v_exp_f32), everything else exact"""
    d = logits - logits.max(1, keepdim=True).values
    e = torch.exp(d)
    e = torch.where(e < P_NORMAL, torch.zeros_like(e), e)
    return _f32(e / e.sum(1, keepdim=True))


def mutant_half_max(logits):
    """each 32-square half subtracts its own maximum"""
    l = logits.view(-1, N_PLANES, 2, 32)
    e = torch.exp(l - l.amax(dim=(1, 3), keepdim=True)).view(-1, N_ACTIONS)
    return _f32(e / e.sum(1, keepdim=True))


def mutant_padded_planes(logits):
    """the padding planes 73..79 (logit 0 + no bias) counted in the sum"""
    mx = logits.max(1, keepdim=True).values
    e = torch.exp(logits - mx)
    return _f32(e / (e.sum(1, keepdim=True) + 7 * 64 * torch.exp(-mx)))


def mutant_bf16(logits):
    return _f32(torch.softmax(logits, 1)).to(torch.bfloat16).float()


MUTANTS = collections.OrderedDict([("flush", mutant_flush), ("half_max", mutant_half_max), ("padded_planes", mutant_padded_planes), ("bf16", mutant_bf16)])
