"""Plain-Python restatement of the search summary (sz_set_search_summary / sz_fetch_search_summary / sz_search_summary_stats /
sz_debug_search_summary, args["search_targets"], a NON-REFERENCE option; include/sigmazero.h is the specification).  It is what
wave_summary_values and wave_summary_surprise (k_summary_pre / k_summary_post, csrc/sz_engine.hip) and csrc/sz_summary.h are held to, bit for
bit (tests/test_gpu_search_summary.py).  Built on kldref, the top of fullref's chain, which stays as it is: the option observes a finished search
and changes nothing, so nothing of the search is restated here.

  * value_term / root_q_of / best_q_of / prior_ok / term repeat csrc/sz_summary.h operator for operator on Python floats (IEEE f64, one rounding
    per operator), with slog from gumbelref and the fixed-order sum wsum of gumbeltreeref;
  * values(N, W) is k_summary_pre's part on plain arrays, surprise(n, P) k_summary_post's, plays() the early-return conditions of sz_play;
  * play_ply(g, u) is sz_play on one board with the option on: the root's children are read while the tree is intact, Game.play(u) writes the
    record (and prunes, compacts or ends the game), the surprise is formed on that record -> (record, Summary);
  * the surprise is formed on the priors as the tree stores them.  Where those sum to 1 (no noise, or Dirichlet root noise) it is
    KL(target || prior) >= 0; under the reference's learning noise (0.75 p + 0.25 * a constant near 1 on every child) they sum to more than 1
    and the figure can be negative: the rule reports it as it is, train_rl.surprise_weights counts a negative one as 0;
  * exact_values / exact_surprise are the same quantities by math.fsum and math.log, what tests/test_summary_ref.py measures the restatement
    against.

Deviation of the restatement from the fsum / log formulas, measured by tests/test_summary_ref.py on hook_cases(): root_q within
MEASURED_ROOT_Q_DEV = 1.2e-16 of max(1, |exact|) (best_q is one division: exact to the bit), surprise within MEASURED_SURPRISE_DEV = 4.3e-16 of
max(1, sum |term|); the test bounds are four times those.

configs() and hook_cases() are the inputs both test modules use."""
import collections
import math

import numpy as np

import kldref as KR
from kldref import KldStop, bits, engine_args, gammas, new_game, begin_ply, worst_case, position_record   # noqa: F401 (re-exported)
from gumbelref import slog
from gumbeltreeref import wsum

MAX_MOVES = 218
NAN = float("nan")
F32_MIN_NORMAL = float(np.float32(1.17549435e-38))
F32_MAX = float(np.float32(3.40282347e+38))
MEASURED_ROOT_Q_DEV = 1.2e-16
MEASURED_SURPRISE_DEV = 4.3e-16
ROOT_Q_BOUND = 4 * MEASURED_ROOT_Q_DEV
SURPRISE_BOUND = 4 * MEASURED_SURPRISE_DEV

Summary = collections.namedtuple("Summary", "valid root_q best_q surprise dropped")
NO_SUMMARY = Summary(0, NAN, NAN, NAN, 0)                  # a board that did not play in this sz_play


# ---------------------------------------------------------------------------------------------------------------- the rule
def value_term(n_c, w_c):
    """sz_summary_value_term"""
    return float(w_c) if int(n_c) >= 1 else 0.0


def root_q_of(ws, total):
    """sz_summary_root_q"""
    return -(float(ws) / float(int(total)))


def best_q_of(w, n):
    """sz_summary_best_q: wave_ending's m"""
    return -(float(w) / float(int(n)))


def prior_ok(p):
    """sz_summary_prior_ok: a normal positive finite f32"""
    p = float(np.float32(p))
    return p >= F32_MIN_NORMAL and p <= F32_MAX


def term(n_c, rtotal, p):
    """sz_summary_term -> (term, dropped)"""
    if int(n_c) <= 0:
        return 0.0, 0
    if not prior_ok(p):
        return 0.0, 1
    t = float(int(n_c)) / float(int(rtotal))
    return t * slog(t / float(np.float32(p))), 0       # sz_kld_term(t, (double)p)


def values(N, W):
    """wave_summary_values: the K = len(N) root children's counted visits and value sums in the tree's order -> (root_q, best_q), or None
    without a child or a visit (k_play's SZ_ERR_ZERO_VISITS)"""
    N = [int(x) for x in N]
    total = sum(N)
    if len(N) == 0 or total == 0:
        return None
    rq = root_q_of(wsum([value_term(n, w) for n, w in zip(N, W)]), total)
    cs = max(range(len(N)), key=lambda c: (N[c], -c))      # the first maximum
    with np.errstate(all="ignore"):
        return rq, best_q_of(W[cs], N[cs])


def surprise(n, P):
    """wave_summary_surprise: the record's counts and the stored priors -> (surprise, dropped); NaN when the record holds no visit"""
    n = [int(x) for x in n]
    rtotal = sum(n)
    if rtotal == 0:
        return NAN, 0
    ts = [term(c, rtotal, p) for c, p in zip(n, P)]
    return wsum([t for t, _ in ts]), sum(d for _, d in ts)


def plays(searching, done, error, game_over):
    """k_play's early return, restated: the board plays in this sz_play"""
    return bool(searching) and bool(done) and not error and not game_over


def summary(N, W, P, record_visits):
    """both kernels on one board that passed plays(): record_visits is a function of no argument that returns the record's counts, called only
    when k_summary_pre found the board valid (k_play writes no record otherwise)"""
    v = values(N, W)
    if v is None:
        return NO_SUMMARY
    s, dropped = surprise(record_visits(), P)
    return Summary(1, v[0], v[1], s, dropped)


def exact_values(N, W):
    """root_q by math.fsum -> (root_q, best_q)"""
    N = [int(x) for x in N]
    total = sum(N)
    cs = max(range(len(N)), key=lambda c: (N[c], -c))
    return -(math.fsum(float(w) for n, w in zip(N, W) if n >= 1) / total), -(float(W[cs]) / N[cs])


def exact_surprise(n, P):
    """KL(target || prior) by math.log and math.fsum over the terms the rule forms -> (surprise, sum of |term|)"""
    n = [int(x) for x in n]
    rtotal = sum(n)
    ts = [(c / rtotal) * math.log((c / rtotal) / float(np.float32(p))) for c, p in zip(n, P) if c > 0 and prior_ok(p)]
    return math.fsum(ts), math.fsum(abs(t) for t in ts)


# ---------------------------------------------------------------------------------------------------------------- one board, ply after ply
def root_arrays(s):
    """the root's children of a finished search while the tree is intact -> (N, W, P) in the tree's order"""
    acts, vis = s.root_children()
    f, k = int(s.first[0]), len(acts)
    return np.asarray(vis, np.int64).copy(), s.W[f:f + k].copy(), s.P[f:f + k].copy()


def play_ply(g, u):
    """sz_play with the option on, on a board that plays (its search is done, no error, its game not over) -> (record, Summary, tree counts,
    stored priors)"""
    assert plays(True, True, g.error is not None, g.over)
    N, W, P = root_arrays(g.search)
    rec = g.play(u)
    k = int(rec["n_child"])
    assert k == len(N), "the record's children are the root's"
    return rec, summary(N, W, P, lambda: rec["visits"][:k]), N, P


# ---------------------------------------------------------------------------------------------------------------- the engine configurations
Config = KR.Config
# chosen on the m these boards see (|m| from 0.001 to 0.7) so that one game resigns at its fourth ply and one at its sixth: an ending that fires
# writes the record all the same, and the summary is made (tests/test_summary_ref.py asserts it)
FORCED_ENDINGS = dict(resign_value=-0.05, resign_patience=2, resign_min_ply=2, draw_value=0.0, draw_patience=0, draw_min_ply=0, proven=0)


def configs():
    """8 boards, 24-48 simulations, 6 plies, the shapes of kldref.configs(): plain; reuse_subtree with L = 4 and the solver; forced playouts with
    FPU, endings and root noise; playout-cap budgets with kld_stop"""
    import fpuref as FP
    B8 = ["wide", "sp518", "sp77", "sp333", "sp0", "sp959", "sp400", "mate1"]
    full, fast = 48, 12
    budgets = [[full if (b + ply) % 3 else fast for b in range(8)] for ply in range(6)]
    out = [
        Config("plain", 32, 6, KR._boards(B8), 1, False, False, 0.0, None, None, False, None, None, None, True, None),
        Config("L4_solver_reuse", 32, 6, KR._boards(B8), 4, True, True, 0.0, None, None, False, None, None, None, False, None),
        Config("forced_fpu_endings_noise", 48, 6, KR._boards(B8), 1, False, False, 2.0, FORCED_ENDINGS, FP.CONFIGS["red_tree_abs1_root"], True,
               None, None, None, True, None),
        Config("playout_cap_budgets_kld", 48, 6, KR._boards(B8), 1, False, False, 0.0, None, None, False, None, budgets, None, True, KldStop(6e-3, 8, 8)),
    ]
    assert all(len(c.boards) == 8 and 24 <= c.S <= 48 and c.plies >= 6 for c in out)
    return out


def play(cfg):
    """the restatement alone: every board of the configuration through its plies -> ([Game], per ply per board the record or None, per ply per
    board the Summary (NO_SUMMARY for a board that does not play), per ply per board the tree counts or None, likewise the stored priors)"""
    games, gam = [new_game(cfg, b) for b in range(len(cfg.boards))], gammas(cfg) if cfg.noise else None
    recs, sums, trees, priors = [], [], [], []
    for ply in range(cfg.plies):
        row, srow, trow, prow = [], [], [], []
        for b, (g, bd) in enumerate(zip(games, cfg.boards)):
            if not g.live:
                row.append(None), srow.append(NO_SUMMARY), trow.append(None), prow.append(None)
                continue
            begin_ply(cfg, g, b, ply, gam)
            g.run()
            assert g.error is None, g.error
            rec, sm, N, P = play_ply(g, bd.u(ply))
            row.append(rec), srow.append(sm), trow.append(N), prow.append(P)
        recs.append(row), sums.append(srow), trees.append(trow), priors.append(prow)
    return games, recs, sums, trees, priors


def pruned_plies(recs, trees):
    """(ply, board) where the record's counts are not the tree's: policy-target pruning cut visits.  Counted on the restatement alone."""
    return [(ply, b) for ply, (row, trow) in enumerate(zip(recs, trees)) for b, (rec, N) in enumerate(zip(row, trow))
            if rec is not None and not np.array_equal(rec["visits"][:len(N)], N)]


# ---------------------------------------------------------------------------------------------------------------- sz_debug_search_summary cases
HookCases = collections.namedtuple("HookCases", "n_child tree_vc value_sum prior record_vc")
# [n] int32, [n, MAX_MOVES] int32, [n, MAX_MOVES] f64, [n, MAX_MOVES] f32, [n, MAX_MOVES] int32; zeros beyond n_child
WIDTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 218)      # the lane-stride and butterfly boundaries


def hook_cases(n_random=1500, seed=61):
    """Cases for sz_debug_search_summary, the stand-alone host program and the accuracy test.  At every width of WIDTHS and at seeded ones: a
    search's worth of visits with zero-visit children, all visits on one child, record counts below the tree's (pruning), a record without a
    visit (rtotal == 0), a tree without a visit, the record equal to the tree; priors from a Dirichlet draw as f32, some far below 1 / K, a few
    that the precondition rule drops (0, negative, subnormal, infinite, NaN)."""
    rng = np.random.default_rng(seed)
    rows = []

    def add(N, W, P, n):
        rows.append((np.asarray(N, np.int64), np.asarray(W, np.float64), np.asarray(P, np.float32), np.asarray(n, np.int64)))

    def tree(K, total, alpha):
        N = rng.multinomial(total, rng.dirichlet(np.full(K, alpha))) if K else np.zeros(0, np.int64)
        q = rng.uniform(-1.0, 1.0, size=K)
        W = np.where(N > 0, N * q + rng.normal(0.0, 1e-3, size=K) * (N > 0), 0.0)
        P = rng.dirichlet(np.full(K, float(rng.choice([0.05, 0.3, 1.0])))).astype(np.float32) if K else np.zeros(0, np.float32)
        P = np.maximum(P, np.float32(2.0 ** -120))           # expansion drops a prior that is exactly 0
        return N, W, P

    def prune(N):
        n = N.copy()
        if len(n) and n.sum() > 0:
            top = int(np.argmax(n))
            cut = rng.integers(0, 4, size=len(n))
            cut[top] = 0
            n = np.maximum(n - cut, 0)
        return n

    for K in WIDTHS:
        for total in (1, 47, 800, 10 ** 5):
            N, W, P = tree(K, total, 0.3)
            add(N, W, P, N)                                           # the record is the tree
            add(N, W, P, prune(N))                                    # pruning
            add(N, W, P, np.zeros(K, np.int64))                       # rtotal == 0
            add(np.zeros(K, np.int64), np.zeros(K), P, N)             # a tree without a visit
            if K:
                one = np.zeros(K, np.int64)
                one[int(rng.integers(K))] = total
                add(one, np.where(one > 0, -0.25 * total, 0.0), P, one)       # all visits on one child
                bad = P.copy()
                bad[int(rng.integers(K))] = rng.choice(np.array([0.0, -0.5, 1e-40, np.inf, np.nan], np.float32))
                add(N, W, bad, N)                                     # the precondition rule
    add([5], [-2.5], [1.0], [5])                                      # K = 1, target == prior: the surprise is exactly 0
    widths = np.concatenate([rng.integers(1, 40, size=n_random * 3 // 4), rng.integers(40, MAX_MOVES + 1, size=n_random - n_random * 3 // 4)])
    for K in widths:
        N, W, P = tree(int(K), int(2.0 ** rng.uniform(0.0, 14.0)), float(rng.choice([0.05, 0.3, 1.0, 10.0])))
        add(N, W, P, prune(N) if rng.random() < 0.5 else N)
    n = len(rows)
    hc = HookCases(np.zeros(n, np.int32), np.zeros((n, MAX_MOVES), np.int32), np.zeros((n, MAX_MOVES), np.float64), np.zeros((n, MAX_MOVES), np.float32),
                   np.zeros((n, MAX_MOVES), np.int32))
    for i, (N, W, P, r) in enumerate(rows):
        k = len(N)
        hc.n_child[i] = k
        hc.tree_vc[i, :k], hc.value_sum[i, :k], hc.prior[i, :k], hc.record_vc[i, :k] = N, W, P, r
    return hc


def hook_case(hc, i):
    k = int(hc.n_child[i])
    return hc.tree_vc[i, :k], hc.value_sum[i, :k], hc.prior[i, :k], hc.record_vc[i, :k]


def hook_reference(hc):
    """the restatement's answers to the cases -> out3 f64 [n, 3]: root_q, best_q (NaN both without a child or a visit), surprise (NaN when the
    record holds no visit), the two parts independent of each other as in k_debug_search_summary"""
    out = np.full((len(hc.n_child), 3), NAN, np.float64)
    for i in range(len(hc.n_child)):
        N, W, P, r = hook_case(hc, i)
        v = values(N, W)
        if v is not None:
            out[i, 0], out[i, 1] = v
        out[i, 2] = surprise(r, P)[0]
    return out


def same_bits(a, b):
    """two f64 arrays bit for bit, every NaN one value (the device's memset NaN is all ones, Python's the quiet NaN)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))
