"""The per-edge value spread and lower-confidence-bound move selection on the GPU (sz_set_lcb / sz_fetch_lcb / sz_lcb_stats /
sz_root_value_spread / sz_debug_tree_spread / sz_debug_lcb, args["lcb"], a NON-REFERENCE option): the HIP engine against the plain-Python
restatement tests/lcbref.py, bit for bit.  1. the device functions on the CPU test's cases, every 64-lane stride boundary among them, and ssqrt
on a few thousand arguments; 2. the engine ply after ply in the three configurations of lcbref.configs(): trees with Q, records, positions,
sz_fetch_lcb and every counter; 3. select = 0 and the option off give the same trees, records, moves and counters, and under select = 0 Q is
the restatement's; 4. a terminal root and a proven root: the counted-out Q; 5. the setter rules; 6. sim.play_games takes the option from args
on fewer slots than games.  tests/test_lcb_ref.py proves on the CPU that the cases and configurations reach the conditions they are there
for."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine, lcb_options_of
from hashmodel import HashModel, evaluate_packed, pack_planes
import lcbref as LR

pytestmark = pytest.mark.gpu

ST_PENDING = 2
MATED_FEN = "R5k1/5ppp/8/8/8/8/8/4K3 b - - 0 1"
STARTS = [0, 17, 518, 77, 333, 959]


def _opts_dict(t):
    return dict(visit_offset=t.visit_offset, value_cutoff=t.value_cutoff if t.use_cutoff else None)


# ------------------------------------------------------------------------------------------------ 1. the device functions on the CPU test's cases
def test_device_lcb_and_ssqrt_equal_restatement_bit_for_bit():
    hc = LR.hook_cases()
    n, cells = len(hc.opts), len(hc.n)
    assert n >= 1400 and set(np.diff(hc.offsets).tolist()) == {1, 2, 63, 64, 65, 127, 128, 129, 218}
    assert hc.opts.dtype.itemsize == C.sizeof(N.sz_lcb_options) == 12
    move, cstar, ncand, bad, lcb, cov = LR.hook_reference(hc)
    LR.assert_coverage(cov, LR.HOOK_COVERAGE)
    x = LR.ssqrt_arguments()
    assert len(x) >= 4000
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ins = [dev(a) for a in (hc.offsets, hc.n, hc.N, hc.W, hc.Q, hc.opts)]
    x_d = dev(x)
    i32 = lambda k: torch.full((k,), -7, dtype=torch.int32, device="cuda")
    move_d, cstar_d, ncand_d, bad_d, xbad_d = i32(n), i32(n), i32(n), i32(n), i32(len(x))
    lcb_d = torch.full((cells,), 7.0, dtype=torch.float64, device="cuda")
    sx_d = torch.full((len(x),), 7.0, dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = [ptr(t) for t in (move_d, cstar_d, ncand_d, bad_d, lcb_d)]
    assert N.lib().sz_debug_lcb(ptr(x_d), ptr(sx_d), ptr(xbad_d), len(x), *[ptr(t) for t in ins], *outs, n, s) == N.SZ_OK
    torch.cuda.synchronize()
    got = np.stack([t.cpu().numpy() for t in (move_d, cstar_d, ncand_d, bad_d)], 1)
    want = np.stack([move, cstar, ncand, bad], 1)
    wrong = np.argwhere(got != want)
    assert not len(wrong), "case %d (K = %d, opts %s) field %d: device %d, restatement %d (%d differ)" % (
        wrong[0][0], np.diff(hc.offsets)[wrong[0][0]], hc.opts[wrong[0][0]], wrong[0][1], got[tuple(wrong[0])], want[tuple(wrong[0])], len(wrong))
    got_lcb = lcb_d.cpu().numpy()
    wrong = np.nonzero(~LR.same_bits(got_lcb, lcb))[0]
    assert not len(wrong), "child %d: device lcb %r, restatement %r (%d differ)" % (wrong[0], got_lcb[wrong[0]], lcb[wrong[0]], len(wrong))
    ref = [LR.ssqrt(v) for v in x.tolist()]
    got_sx = sx_d.cpu().numpy()
    wrong = np.nonzero(~LR.same_bits(got_sx, np.array([r for r, _ in ref])))[0]
    assert not len(wrong), "ssqrt(%r): device %r, restatement %r (%d differ)" % (x[wrong[0]], got_sx[wrong[0]], ref[wrong[0]][0], len(wrong))
    assert xbad_d.cpu().numpy().tolist() == [b for _, b in ref] and sum(b for _, b in ref) >= 6
    # each part alone, and the refusals
    assert N.lib().sz_debug_lcb(ptr(x_d), ptr(sx_d), None, len(x), *[None] * 6, *[None] * 5, 0, s) == N.SZ_OK
    assert N.lib().sz_debug_lcb(None, None, None, 0, *[ptr(t) for t in ins], *outs, n, s) == N.SZ_OK
    torch.cuda.synchronize()
    assert np.array_equal(move_d.cpu().numpy(), move) and LR.same_bits(sx_d.cpu().numpy(), got_sx).all()
    assert N.lib().sz_debug_lcb(None, None, None, 0, *[None] * 6, *outs, n, s) == N.SZ_ERR_INVALID
    assert N.lib().sz_debug_lcb(None, None, None, 0, *[ptr(t) for t in ins], *outs, 0, s) == N.SZ_ERR_INVALID
    assert N.lib().sz_debug_lcb(ptr(x_d), None, None, len(x), *[None] * 6, *[None] * 5, 0, s) == N.SZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 2. the engine against the restatement
def _tree_bytes(eng, b):
    return tuple(a.tobytes() for a in eng.debug_tree(b) + eng.debug_tree_proven(b))


def _assert_tree(tag, eng, b, s, with_q):
    for a, y in zip(eng.debug_tree(b), s.tree()):
        assert a.dtype == y.dtype and a.tobytes() == y.tobytes(), "%s: tree differs" % tag
    pr, co = eng.debug_tree_proven(b)
    proven = s.tree_proven()
    assert np.array_equal(pr, proven[0]) and np.array_equal(co, proven[1]), "%s: proven labels / complete bits differ" % tag
    if with_q:
        q, want = eng.debug_tree_spread(b), s.tree_spread()
        assert q.shape == want.shape and LR.same_bits(q, want).all(), "%s: Q differs at rows %s" % (tag, np.nonzero(~LR.same_bits(q, want))[0][:8].tolist())


def _steps(eng, searches, live, modes, tag, S, chunk):
    """the steps of one search on every live board b against searches[b], sz_search_check_stop after every chunk-th step: boards pending and
    every network input row -> steps"""
    B, L = eng.B, eng.L
    t = 0
    while True:
        torch.cuda.synchronize()
        pend = (eng.debug_pending()[4] & ST_PENDING) != 0
        want = [bool(live[b]) and t < len(s.steps) for b, s in enumerate(searches)]
        assert pend.tolist() == want, "%s step %d: boards waiting for the network %s, restatement %s" % (tag, t, pend.tolist(), want)
        if not pend.any():
            return t
        assert t < S
        planes = pack_planes(eng.planes.float().cpu().numpy())
        pol = np.zeros((B * L, N.SZ_ACTIONS), np.float32)
        val = np.zeros(B * L, np.float32)
        for b in np.nonzero(pend)[0]:
            rows = searches[b].steps[t]
            assert np.array_equal(planes[b * L:b * L + len(rows)], rows), "%s step %d board %d: network input rows differ" % (tag, t, b)
            for i in range(len(rows)):
                pol[b * L + i], val[b * L + i] = evaluate_packed(rows[i], *modes[b])
        eng.step(torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda())
        t += 1
        if t % chunk == 0:
            eng.check_stop()


def _drive(cfg, lcb):
    """one engine through the configuration's plies, lock step with the restatement.  lcb: "config" (the per-ply options of the configuration),
    an Lcb for every ply, or None = the option off.  -> (per ply what the engine left: trees, record, counters; the games)"""
    B = len(cfg.boards)
    eng = SelfPlayEngine(None, LR.engine_args(cfg), B, chess960=True, learning=cfg.learning)
    games = [LR.new_game(cfg, b, lcb) for b in range(B)]
    modes = [(bd.mode, bd.salt) for bd in cfg.boards]
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    if cfg.endings is not None:
        eng.set_endings(LR.KR.PR.FU.ER.options(**cfg.endings), [0] * B)
    if cfg.kld is not None:
        eng.set_kld_stop(tuple(cfg.kld))
    if cfg.summary:
        eng.set_search_summary(True)
    on = lcb is not None
    if on:
        with pytest.raises(N.NativeError):
            eng.fetch_lcb()                                              # never on yet
    left = []
    n_plies = n_steps = n_made = n_idle = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(cfg.plies):
            live = [g.live for g in games]
            assert any(live)
            n_plies += 1
            if on:
                eng.set_lcb(tuple(LR.lcb_of(cfg, ply, lcb)))             # new options at every ply, between searches
                if ply == 0:
                    first = eng.fetch_lcb()
                    assert (first["move"] == -1).all() and (first["cstar"] == -1).all() and np.isnan(first["lcb_move"]).all() and not first["decided"].any()
            if cfg.budgets is not None:
                eng.set_budgets([cfg.budgets[ply][b] if live[b] else 0 for b in range(B)])
            if cfg.forced_k:
                eng.set_forced_playouts(cfg.forced_k, [1] * B)
            if cfg.temperature is not None:
                topts, temps = cfg.temperature[ply % len(cfg.temperature)]
                eng.set_move_temperature(_opts_dict(topts), temps)
            for b, g in enumerate(games):
                if live[b]:
                    LR.begin_ply(cfg, g, b, ply)
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s board %d (%s) ply %d" % (cfg.name, b, cfg.boards[b].name, ply)
            eng.begin()
            chunk = -(-cfg.kld.interval // cfg.L) if cfg.kld is not None else cfg.S + 1
            n_steps += _steps(eng, [g.search for g in games], live, modes, "%s ply %d" % (cfg.name, ply), cfg.S, chunk)
            st = eng.check_errors()
            assert st["boards_pending"] == 0 and st["boards_done"] == sum(live)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search, on)
            if on:
                rq = eng.root_value_spread()
                for b, g in enumerate(games):
                    want = g.search.root_spread() if live[b] else np.zeros(0)
                    assert LR.same_bits(rq[b, :len(want)], want).all() and not rq[b, len(want):].any(), "%s: sz_root_value_spread" % tag(b)
            trees = [_tree_bytes(eng, b) for b in range(B)]
            u = np.array([LR.uniform_of(cfg, b, ply) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            rec = eng.fetch_ply()
            ends = eng.fetch_endings() if cfg.endings is not None else None
            got = eng.fetch_lcb() if on else None
            summ = eng.fetch_search_summary() if cfg.summary else None
            for b, g in enumerate(games):
                if not live[b]:                                          # its game is over: the board did not play
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tag(b)
                    if on:
                        n_idle += 1
                        assert (got["move"][b], got["cstar"][b], got["n_candidates"][b], got["decided"][b]) == (-1, -1, 0, 0) and math.isnan(got["lcb_move"][b]) and \
                            math.isnan(got["lcb_cstar"][b]), "%s: sz_fetch_lcb for a board that did not play" % tag(b)
                    continue
                if cfg.summary:
                    want, sm, _, _ = LR.SR.play_ply(g, u[b])
                    assert (int(summ["valid"][b]), LR.bits(summ["root_q"][b]), LR.bits(summ["best_q"][b]), LR.bits(summ["surprise"][b])) == \
                        (sm.valid, LR.bits(sm.root_q), LR.bits(sm.best_q), LR.bits(sm.surprise)), "%s: search summary" % tag(b)
                else:
                    want = g.play(u[b])
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                have = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert have == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r, restatement %r, lcb %r" % (
                    tag(b), have, {k: want[k] for k in ("n_child", "colour", "chosen", "game_over", "result")}, g.last_lcb)
                assert eng.debug_position(b)[0].tobytes() == LR.SR.position_record(g.game), "%s: position record after sz_play" % tag(b)
                if on:
                    l = g.last_lcb
                    n_made += l.move >= 0
                    have = (int(got["move"][b]), int(got["cstar"][b]), LR.bits(got["lcb_move"][b]), LR.bits(got["lcb_cstar"][b]), int(got["n_candidates"][b]), int(got["decided"][b]))
                    assert have == (l.move, l.cstar, LR.bits(l.lcb_move), LR.bits(l.lcb_cstar), l.n_candidates, l.decided), "%s: sz_fetch_lcb %r, restatement %r" % (tag(b), have, l)
                if ends is not None:
                    assert int(ends["kind"][b]) == g.last[0], "%s: sz_fetch_endings" % tag(b)
                    if g.last[0] and on:
                        assert want["chosen"] == -1 and g.last_lcb.move == -1, "%s: an ending that fires makes no choice" % tag(b)
                if cfg.temperature is not None:
                    tmp = eng.fetch_temperature()
                    assert int(tmp["n_eligible"][b]) == g.last_temp[0] and LR.same_bits(tmp["p_chosen"][b], g.last_temp[1]), "%s: sz_fetch_temperature" % tag(b)
            assert eng.lcb_stats() == tuple(sum(g.lcb_stats[i] for g in games) for i in range(3)), "%s ply %d: sz_lcb_stats" % (cfg.name, ply)
            assert eng.forced_stats() == (sum(g.forced_selections for g in games), sum(g.pruned_visits for g in games)), "%s ply %d: sz_forced_stats" % (cfg.name, ply)
            assert eng.solver_stats() == (sum(g.proven_stops for g in games), sum(g.proved for g in games)), "%s ply %d: solver counters" % (cfg.name, ply)
            assert eng.kld_stop_stats() == tuple(sum(g.kld_stats[i] for g in games) for i in range(3)), "%s ply %d: sz_kld_stop_stats" % (cfg.name, ply)
            if ends is not None:
                assert eng.ending_stats() == tuple(sum(g.ended[i] for g in games) for i in range(4)), "%s ply %d: sz_ending_stats" % (cfg.name, ply)
            if cfg.temperature is not None:
                assert eng.temperature_stats() == tuple(sum(g.temp_stats[i] for g in games) for i in range(3)), "%s ply %d: sz_temperature_stats" % (cfg.name, ply)
            st = eng.stats()
            assert tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth")) == \
                tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits", "sum_depth")), "%s ply %d: sz_stats" % (cfg.name, ply)
            left.append(dict(trees=trees, rec={k: v.tobytes() for k, v in rec.items()},
                             stats=tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth", "sum_children", "boards_done", "boards_error")),
                             solver=eng.solver_stats(), forced=eng.forced_stats(), kld=eng.kld_stop_stats(),
                             endings=eng.ending_stats() if cfg.endings is not None else None,
                             temperature=eng.temperature_stats() if cfg.temperature is not None else None))
    eng.close()
    print("%s (lcb %s): %d plies, %d network steps, %d choices under the option, %d boards sat a ply out, stats %s" % (
        cfg.name, lcb if not on or lcb == "config" else tuple(lcb), n_plies, n_steps, n_made, n_idle, [sum(g.lcb_stats[i] for g in games) for i in range(3)]))
    assert n_plies >= 6 and n_steps >= 6 * 8 // cfg.L and (not on or n_made >= 24)
    return left, games


@pytest.mark.parametrize("name", [c.name for c in LR.configs()])
def test_engine_matches_restatement_ply_after_ply(name):
    cfg = next(c for c in LR.configs() if c.name == name)
    assert len(cfg.boards) == 8 and cfg.S == 24 and 6 <= cfg.plies <= 8
    left, games = _drive(cfg, "config")
    cov = LR.coverage(games)
    LR.assert_coverage(cov, LR.CONFIG_COVERAGE)                          # counted on the restatement alone
    assert sum(g.lcb_stats[2] for g in games) == 0, "no ssqrt argument outside 0.0 and the positive normal numbers"


# ------------------------------------------------------------------------------------------------ 3. select = 0 and the option off
@pytest.mark.parametrize("name", [c.name for c in LR.configs()][:2])
def test_select_zero_and_option_off_leave_the_same_engine(name):
    cfg = next(c for c in LR.configs() if c.name == name)
    observe, games = _drive(cfg, LR.options(5.0, 0.15, False))           # Q is held to the restatement's inside
    off, games_off = _drive(cfg, None)
    assert len(observe) == len(off)
    for ply, (a, b) in enumerate(zip(observe, off)):
        for key in a:
            assert a[key] == b[key], "%s ply %d: %s differs between select = 0 and the option off" % (name, ply, key)
    assert [g.chosen for g in games] == [g.chosen for g in games_off]
    assert sum(g.lcb_stats[0] for g in games) == 0 and sum(g.lcb_stats[1] for g in games) > 0, "the rule's move differed somewhere and was not played"


# ------------------------------------------------------------------------------------------------ 4. a terminal root and a proven root
def test_terminal_root_and_proven_root_count_their_budget_into_q():
    S = 24
    mk = [lambda: sz.ChessTensor(fen=MATED_FEN), lambda: sz.ChessTensor(fen=LR.KR.MATE_IN_1_FEN), lambda: sz.ChessTensor(chess960=True, scharnagl=518)]
    eng = SelfPlayEngine(None, {"C": 2, "num_searches": S, "solver": True, "lcb": {}}, 3, chess960=True, learning=False)
    assert eng.lcb == (5.0, float(np.float32(0.15)), True)
    games = [LR.Game(m(), S, None, reuse=False, L=1, lam=1.0, solver=True, c=2.0, learning=False, mode="rational", salt=2, lcb=LR.options()) for m in mk]
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
        g.begin()
        g.run()
    eng.begin()
    _steps(eng, [g.search for g in games], [True] * 3, [("rational", 2)] * 3, "roots", S, S + 1)
    for b, g in enumerate(games):
        _assert_tree("board %d" % b, eng, b, g.search, True)
    mated, proven = games[0].search, games[1].search
    assert mated.tree_spread().tolist() == [float(S)] and int(mated.N[0]) == S + 1 and float(mated.W[0]) == -float(S), "the terminal root: Q = (tv * tv) * S"
    assert int(proven.R[0]) == LR.WIN and proven.proven_stops >= 1 and int(proven.N[0]) == S + 1, "the root was proven before its budget ran out and counted it out"
    assert float(proven.Q[0]) >= proven.proven_stops - 1e-9, "every proven stop backs up +-1: exactly 1.0 more in Q[0], one simulation at a time"
    assert eng.debug_tree_spread(1)[0] == float(proven.Q[0])
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. setter rules
def _search(eng):
    eng.begin()
    for _ in range(eng.S):
        eng.step(*eng.evaluate(eng.planes))


def test_setter_rules():
    lib = N.lib()
    O = N.sz_lcb_options
    eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 16}, 3, chess960=True, learning=False)
    s = eng._stream()
    z = C.c_void_p()
    nan, inf = float("nan"), float("inf")
    assert lib.sz_set_lcb(None, C.byref(O(5.0, 0.15, 1)), s) == N.SZ_ERR_INVALID and lib.sz_fetch_lcb(None, z, z, z, z, z, z, s) == N.SZ_ERR_INVALID
    for bad in (O(nan, 0.15, 1), O(inf, 0.15, 1), O(-1.0, 0.15, 1), O(5.0, nan, 1), O(5.0, -0.01, 1), O(5.0, 1.01, 1), O(5.0, inf, 1)):
        assert lib.sz_set_lcb(eng._e, C.byref(bad), s) == N.SZ_ERR_INVALID, (bad.stdevs, bad.min_visit_prop)
    assert lib.sz_fetch_lcb(eng._e, z, z, z, z, z, z, s) == N.SZ_ERR_STATE, "fetch before the option was ever on"
    assert eng.lcb_stats() == (0, 0, 0), "a refused call allocates and counts nothing"
    assert lib.sz_set_lcb(eng._e, None, s) == N.SZ_OK, "off is always accepted"
    q = torch.zeros(3, N.SZ_MAX_MOVES, dtype=torch.float64, device="cuda")
    assert lib.sz_root_value_spread(eng._e, C.c_void_p(q.data_ptr()), s) == N.SZ_ERR_STATE
    eng.new_games(STARTS[:3])
    eng.begin()
    for _ in range(5):
        eng.step(*eng.evaluate(eng.planes))
    assert lib.sz_set_lcb(eng._e, C.byref(O(5.0, 0.15, 1)), s) == N.SZ_ERR_STATE, "during a search"
    with pytest.raises(N.NativeError):
        eng.set_lcb((5.0, 0.15, True))
    assert eng.lcb is None and lib.sz_fetch_lcb(eng._e, z, z, z, z, z, z, s) == N.SZ_ERR_STATE, "nothing changed"
    for _ in range(5, 16):
        eng.step(*eng.evaluate(eng.planes))
    eng.check_errors()
    # the search is done, but it was begun without the option: the sz_play that follows plays as without it
    eng.set_lcb((0.0, 0.0, True))
    assert lib.sz_fetch_lcb(eng._e, z, z, z, z, z, z, s) == N.SZ_OK, "every pointer may be NULL"
    assert lib.sz_root_value_spread(eng._e, C.c_void_p(q.data_ptr()), s) == N.SZ_ERR_STATE, "the search begun last kept no second moment"
    with pytest.raises(N.NativeError):
        eng.debug_tree_spread(0)
    _, visits, n_child, _, _ = eng.root_children()
    action = eng.root_children()[0]
    eng.play([-1.0] * 3)
    rec, got = eng.fetch_ply(), eng.fetch_lcb()
    for b in range(3):
        assert rec["chosen"][b] == action[b, int(np.argmax(visits[b, :n_child[b]]))], "the most visited move, as without the option"
    assert (got["move"] == -1).all() and not got["decided"].any() and eng.lcb_stats() == (0, 0, 0)
    # the next search takes it up: stdevs = 0 and min_visit_prop = 0 play the best mean among the children with two visits
    _search(eng)
    eng.check_errors()
    action, visits, n_child, _, wsum = eng.root_children()
    rq = eng.root_value_spread()
    eng.play([-1.0] * 3)
    rec, got = eng.fetch_ply(), eng.fetch_lcb()
    for b in range(3):
        k = int(n_child[b])
        fd = LR.choose(visits[b, :k], visits[b, :k], wsum[b, :k], rq[b, :k], LR.options(0.0, 0.0))
        assert (int(got["move"][b]), int(got["cstar"][b]), int(got["n_candidates"][b]), int(got["decided"][b])) == (fd.move, fd.cstar, fd.n_candidates, 1)
        assert rec["chosen"][b] == action[b, fd.move] and LR.same_bits(got["lcb_move"][b], fd.lcb[fd.move])
        assert (rq[b, :k] >= 0).all() and (rq[b, :k] <= visits[b, :k]).all() and (rq[b, :k][visits[b, :k] > 0] > 0).any()
    assert eng.lcb_stats()[0] == 3
    eng.begin()
    eng.step(*eng.evaluate(eng.planes))
    assert lib.sz_set_lcb(eng._e, None, s) == N.SZ_ERR_STATE, "during a search, off too"
    assert eng.lcb == (0.0, 0.0, True)
    eng.close()

    # a reuse_subtree engine refuses; Gumbel and the option refuse each other, in both directions
    reuse = SelfPlayEngine(HashModel(salt=3), {"C": 2, "num_searches": 16, "reuse_subtree": True}, 2, chess960=True, learning=False)
    assert lib.sz_set_lcb(reuse._e, C.byref(O(5.0, 0.15, 1)), reuse._stream()) == N.SZ_ERR_STATE
    assert lib.sz_set_lcb(reuse._e, None, reuse._stream()) == N.SZ_OK
    reuse.close()
    g_on = SelfPlayEngine(HashModel(salt=3), {"C": 2, "num_searches": 24, "gumbel": {"m": 4}}, 8, chess960=True, learning=True)
    s = g_on._stream()
    assert lib.sz_set_lcb(g_on._e, C.byref(O(5.0, 0.15, 1)), s) == N.SZ_ERR_STATE
    assert lib.sz_set_lcb(g_on._e, None, s) == N.SZ_OK, "off is always accepted"
    g_on.set_gumbel(None)
    assert lib.sz_set_lcb(g_on._e, C.byref(O(5.0, 0.15, 1)), s) == N.SZ_OK
    gopt = N.sz_gumbel_options(4, 50.0, 1.0)
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_ERR_STATE
    assert lib.sz_set_lcb(g_on._e, None, s) == N.SZ_OK
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_OK
    g_on.close()
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 8, "lcb": {"stdevs": -1}}, 1)
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 24, "lcb": {}, "gumbel": {"m": 4}}, 2)
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 24, "lcb": {}, "reuse_subtree": True}, 2)


# ------------------------------------------------------------------------------------------------ 6. play_games
def test_play_games_takes_the_option_from_args():
    from sigma_zero_amd.sim import play_games
    salt, starts, caps = 4, [0, 959, 518, 400, 77, 5], [4, 3, 4, 3, 3, 4]
    u = lambda g, ply: -1.0 if (g + ply) % 2 else ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0      # greedy and sampled plies in every game
    base = {"C": 2, "num_searches": 24}
    lcb = {"stdevs": 0.0, "min_visit_prop": 0.0}
    args = dict(base, lcb=lcb)
    opts = LR.options(*lcb_options_of(args))
    stats = {}
    got = play_games(HashModel(salt=salt), args, 6, c960=True, scharnagl=starts, uniforms=u, max_plies=caps, learning=True, n_boards=4, stats=stats)
    off = play_games(HashModel(salt=salt), base, 6, c960=True, scharnagl=starts, uniforms=u, max_plies=caps, learning=True, n_boards=4)
    decided = differs = n = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for g, (start, cap) in enumerate(zip(starts, caps)):               # a refilled slot starts with clean state: every game is its own restatement
            ref = LR.Game(sz.ChessTensor(chess960=True, scharnagl=start), 24, None, reuse=False, c=2.0, learning=True, mode="dyadic", salt=salt, lcb=opts)
            ply = 0
            while ref.live and ply < cap:
                ref.begin()
                ref.run()
                assert ref.error is None
                ref.play(u(g, ply))
                ply += 1
            assert got[g]["chosen_actions"] == ref.chosen, "game %d: moves played" % g
            decided, differs, n = decided + ref.lcb_stats[0], differs + ref.lcb_stats[1], n + ply
    assert n >= 18 and (stats["lcb_decided"], stats["lcb_differs"]) == (decided, differs) and decided >= 6
    assert any(a["chosen_actions"] != b["chosen_actions"] for a, b in zip(got, off)), "the rule changed a move"
    assert all(set(a) == set(b) for a, b in zip(got, off)), "nothing new is kept per sample"
