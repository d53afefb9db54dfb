"""The search summary on the GPU (sz_set_search_summary / sz_fetch_search_summary / sz_search_summary_stats / sz_debug_search_summary,
args["search_targets"], a NON-REFERENCE option): the HIP engine against the plain-Python restatement tests/summaryref.py, bit for bit.
1. the device functions on the CPU test's cases, every lane-stride and butterfly boundary among them; 2. the engine ply after ply in the
configurations of summaryref.configs() (plain; reuse_subtree with L = 4 and the solver; forced playouts + FPU + endings + root noise; playout-cap
budgets + kld_stop): root_q, best_q, surprise and valid of every board after every sz_play, and the same run with the option off for trees,
records and counters (the option observes and changes nothing); 3. boards that do not play; sz_play_moves; 4. the setter rules;
5. sim.play_games takes the option from args on fewer slots than games.  tests/test_summary_ref.py proves on the CPU that the configurations
reach the conditions they are there for."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine, search_targets_of
from hashmodel import HashModel, evaluate_packed, pack_planes
import summaryref as SR

pytestmark = pytest.mark.gpu

ST_PENDING, ST_ERROR = 2, 16
STARTS = [0, 17, 518, 77, 333, 959]
UNIFORMS = [-1.0, 0.3, 0.7, -1.0, 0.55, 0.1]


def _bits(x):
    return [SR.bits(v) for v in np.asarray(x, np.float64).tolist()]


# ------------------------------------------------------------------------------------------------ 1. the device functions on the CPU test's cases
def test_device_summary_equals_restatement_bit_for_bit():
    hc = SR.hook_cases()
    n = len(hc.n_child)
    assert n >= 1700 and hc.tree_vc.shape == (n, N.SZ_MAX_MOVES) and set(SR.WIDTHS) <= set(hc.n_child.tolist())
    assert SR.WIDTHS == (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 218)
    want = SR.hook_reference(hc)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ins = [dev(x) for x in (hc.n_child, hc.tree_vc, hc.value_sum, hc.prior, hc.record_vc)]
    out = torch.full((n, 3), 12345.0, dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert N.lib().sz_debug_search_summary(*[ptr(t) for t in ins], ptr(out), n, s) == N.SZ_OK
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.argwhere(~SR.same_bits(got, want))
    assert not len(bad), "case %d (K %d) value %d: device %r, restatement %r (%d differ)" % (
        bad[0][0], hc.n_child[bad[0][0]], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
    assert len(set(want[~np.isnan(want)].tolist())) > 3000, "the cases are not a handful of values"
    # what the cases are there for, counted on the restatement's inputs
    k = hc.n_child
    rows = lambda m: int(np.count_nonzero(m))
    tree_total, rec_total = hc.tree_vc.sum(1), hc.record_vc.sum(1)
    assert rows((hc.tree_vc == 0).any(1) & (tree_total > 0) & (k > 1)) >= 300, "zero-visit children"
    assert rows((hc.tree_vc.max(1) == tree_total) & (tree_total > 1) & (k > 1)) >= 10, "all visits on one child"
    assert rows((hc.record_vc <= hc.tree_vc).all(1) & (rec_total < tree_total) & (rec_total > 0)) >= 300, "record counts below tree counts"
    assert rows((rec_total == 0) & (k > 0)) >= 10 and np.isnan(want[(rec_total == 0), 2]).all(), "rtotal == 0"
    assert N.lib().sz_debug_search_summary(None, *[ptr(t) for t in ins[1:]], ptr(out), n, s) == N.SZ_ERR_INVALID
    assert N.lib().sz_debug_search_summary(*[ptr(t) for t in ins], ptr(out), 0, s) == N.SZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 2. the engine against the restatement
def _tree_bytes(eng, b):
    return tuple(x.tobytes() for x in eng.debug_tree(b) + eng.debug_tree_proven(b))


def _assert_tree(tag, eng, b, tree, proven):
    for x, y in zip(eng.debug_tree(b), tree):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: tree differs" % tag
    pr, co = eng.debug_tree_proven(b)
    assert np.array_equal(pr, proven[0]) and np.array_equal(co, proven[1]), "%s: proven labels / complete bits differ" % tag


def _steps(eng, searches, live, modes, tag, S, chunk):
    """the steps of one search on every live board b against searches[b], sz_search_check_stop after every chunk-th step (a no-op while
    kld_stop is off): boards pending and every network input row -> steps"""
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


def _drive(cfg, on):
    """one engine through the configuration's plies, lock step with the restatement.  on: the summary is switched on and held to the
    restatement after every sz_play.  -> (per ply what the engine left: trees, record, counters; restatement's per-ply (records, tree counts))"""
    B = len(cfg.boards)
    eng = SelfPlayEngine(None, SR.engine_args(cfg), B, chess960=True, learning=cfg.learning, edges_per_board=SR.worst_case(cfg.S) if cfg.reuse else 0)
    games = [SR.new_game(cfg, b) for b in range(B)]
    modes = [(bd.mode, bd.salt) for bd in cfg.boards]
    gam = SR.gammas(cfg) if cfg.noise else None
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    if cfg.endings is not None:
        eng.set_endings(SR.KR.PR.FU.ER.options(**cfg.endings), [0] * B)
    if cfg.kld is not None:
        eng.set_kld_stop(tuple(cfg.kld))
    if on:
        with pytest.raises(N.NativeError):
            eng.fetch_search_summary()                                   # never on yet
        eng.set_search_summary(True)
        first = eng.fetch_search_summary()
        assert not first["valid"].any() and all(np.isnan(first[k]).all() for k in ("root_q", "best_q", "surprise")), "before the first sz_play"
    assert eng.search_summary == bool(on)
    left, rrecs, rtrees = [], [], []
    n_plies = n_steps = n_made = n_idle = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(cfg.plies):
            live = [g.live for g in games]
            assert any(live)
            n_plies += 1
            if cfg.budgets is not None:
                eng.set_budgets([cfg.budgets[ply][b] if live[b] else 0 for b in range(B)])
            if cfg.noise:
                eng.set_search_root_noise(torch.from_numpy(gam[ply]), [0] * B)
            if cfg.forced_k:
                eng.set_forced_playouts(cfg.forced_k, [1] * B)
            for b, g in enumerate(games):
                if live[b]:
                    SR.begin_ply(cfg, g, b, ply, gam)
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s board %d (%s) ply %d start=%s" % (cfg.name, b, cfg.boards[b].name, ply, games[b].starts[-1])
            eng.begin()
            chunk = -(-cfg.kld.interval // cfg.L) if cfg.kld is not None else cfg.S + 1
            n_steps += _steps(eng, [g.search for g in games], live, modes, "%s ply %d" % (cfg.name, ply), cfg.S, chunk)
            st = eng.check_errors()
            assert st["boards_pending"] == 0 and st["boards_done"] == sum(live)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search.tree(), g.search.tree_proven())
            trees = [_tree_bytes(eng, b) for b in range(B)]
            u = np.array([cfg.boards[b].u(ply) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            rec = eng.fetch_ply()
            ends = eng.fetch_endings() if cfg.endings is not None else None
            got = eng.fetch_search_summary() if on else None
            rrow, trow = [], []
            for b, g in enumerate(games):
                if not live[b]:                                          # its game is over: the board did not play
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tag(b)
                    rrow.append(None), trow.append(None)
                    if on:
                        n_idle += 1
                        assert got["valid"][b] == 0 and all(np.isnan(got[k][b]) for k in ("root_q", "best_q", "surprise")), "%s: a summary for a board that did not play" % tag(b)
                    continue
                want, sm, Ntree, _ = SR.play_ply(g, u[b])
                rrow.append(want), trow.append(Ntree)
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]), "%s: the record's child order is the root's" % tag(b)
                assert np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                have = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert have == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r, restatement %r" % (tag(b), have, want)
                if on:
                    n_made += 1
                    have = (int(got["valid"][b]), SR.bits(got["root_q"][b]), SR.bits(got["best_q"][b]), SR.bits(got["surprise"][b]))
                    assert have == (sm.valid, SR.bits(sm.root_q), SR.bits(sm.best_q), SR.bits(sm.surprise)), \
                        "%s: summary valid / root_q / best_q / surprise %r, restatement %r" % (tag(b), (got["valid"][b], got["root_q"][b], got["best_q"][b], got["surprise"][b]), sm)
                    if ends is not None:
                        assert SR.bits(got["best_q"][b]) == SR.bits(ends["mover_value"][b]), "%s: best_q is sz_fetch_endings' mover_value" % tag(b)
                if ends is not None:
                    assert int(ends["kind"][b]) == g.last[0], "%s: sz_fetch_endings" % tag(b)
            rrecs.append(rrow), rtrees.append(trow)
            if on:
                assert eng.search_summary_stats() == (n_made, 0), "%s ply %d: sz_search_summary_stats" % (cfg.name, ply)
            else:
                assert eng.search_summary_stats() == (0, 0)
            st = eng.stats()
            left.append(dict(trees=trees, after=[_tree_bytes(eng, b) for b in range(B)], rec={k: v.tobytes() for k, v in rec.items()},
                             stats=tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth", "sum_children", "boards_done", "boards_error")),
                             solver=eng.solver_stats(), forced=eng.forced_stats(), kld=eng.kld_stop_stats(),
                             endings=eng.ending_stats() if cfg.endings is not None else None))
    eng.close()
    print("%s (summary %s): %d plies, %d network steps, %d summaries made, %d boards sat a ply out" % (cfg.name, "on" if on else "off", n_plies, n_steps, n_made, n_idle))
    assert n_plies >= 6 and n_steps >= 6 * 12 // cfg.L and (not on or (n_made >= 30 and n_idle >= 1))
    return left, rrecs, rtrees, games


@pytest.mark.parametrize("name", [c.name for c in SR.configs()])
def test_engine_summary_matches_restatement_and_changes_nothing(name):
    cfg = next(c for c in SR.configs() if c.name == name)
    assert len(cfg.boards) == 8 and 24 <= cfg.S <= 48 and cfg.plies >= 6
    on, rrecs, rtrees, games = _drive(cfg, True)
    off = _drive(cfg, False)[0]
    assert len(on) == len(off)
    for ply, (a, b) in enumerate(zip(on, off)):
        for key in a:
            assert a[key] == b[key], "%s ply %d: %s differs between the option on and off" % (name, ply, key)
    if cfg.reuse:
        assert any(s == "reused" for g in games for s in g.starts), "kept subtrees: k_summary_pre ran before the compaction"
    if cfg.forced_k:                                                     # counted on the restatement alone
        pruned = SR.pruned_plies(rrecs, rtrees)
        assert len(pruned) >= 1 and sum(g.pruned_visits for g in games) > 0, "a board and ply where the pruned counts are not the tree's"
        assert any(g.termination is not None for g in games), "an ending fired: the record was written and the summary made"
    if cfg.kld is not None:
        assert sum(g.kld_stats[0] for g in games) > 0 and on[-1]["kld"][0] > 0, "boards stopped early"


# ------------------------------------------------------------------------------------------------ 3. boards that do not play; sz_play_moves
def _search(eng):
    eng.begin()
    for _ in range(eng.S):
        eng.step(*eng.evaluate(eng.planes))


def test_boards_that_do_not_play_and_play_moves():
    S, Bn = 24, 4
    eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": S, "search_targets": {}}, Bn, chess960=True, learning=False)
    assert eng.search_targets == (0.0, "root", 0.0) and eng.search_summary
    eng.new_games(STARTS[:Bn], [1, 1, 1, 0])                             # board 3 is inactive
    eng.set_budgets([S, 0, S, S])                                        # board 1 searches nothing: SZ_ERR_ZERO_VISITS at sz_play, sticky
    nan3 = lambda got, b: got["valid"][b] == 0 and all(np.isnan(got[k][b]) for k in ("root_q", "best_q", "surprise"))
    for ply in range(2):
        _search(eng)
        _, visits, n_child, prior, wsum = eng.root_children()           # the finished search's root, while the tree is intact
        eng.play(UNIFORMS[:Bn])
        got, rec, status = eng.fetch_search_summary(), eng.fetch_ply(), eng.debug_pending()[4]
        assert status[1] & ST_ERROR and eng.stats()["first_error"] == N.SZ_ERR_ZERO_VISITS and eng.stats()["boards_error"] == 1
        assert nan3(got, 1) and nan3(got, 3), "ply %d: an error board and an inactive board have no summary" % ply
        for b in (0, 2):
            k = int(rec["n_child"][b])
            assert got["valid"][b] == 1 and rec["active"][b] == 1
            assert k == int(n_child[b]) and np.array_equal(rec["visits"][b, :k], visits[b, :k])
            sm = SR.summary(visits[b, :k], wsum[b, :k], prior[b, :k], lambda: rec["visits"][b, :k])
            assert (1, SR.bits(sm.root_q), SR.bits(sm.best_q), SR.bits(sm.surprise)) == (1, SR.bits(got["root_q"][b]), SR.bits(got["best_q"][b]), SR.bits(got["surprise"][b]))
            assert -1.0 <= got["root_q"][b] <= 1.0 and -1.0 <= got["best_q"][b] <= 1.0 and got["surprise"][b] >= -1e-12, "learning off: the priors sum to 1"
        assert eng.search_summary_stats() == (2 * (ply + 1), 0)
    # sz_play_moves makes no summary and leaves the last one alone
    before = eng.fetch_search_summary()
    _search(eng)
    action = eng.root_children()[0]
    moves = np.array([action[0, 0], -1, action[2, 0], -1], np.int32)
    eng.play_moves(moves)
    rec = eng.fetch_ply()
    assert rec["chosen"][0] == moves[0] and rec["chosen"][2] == moves[2] and eng.stats()["boards_error"] == 1
    after = eng.fetch_search_summary()
    assert all(_bits(before[k]) == _bits(after[k]) for k in ("root_q", "best_q", "surprise")) and before["valid"].tolist() == after["valid"].tolist()
    assert eng.search_summary_stats() == (4, 0)
    # off again: sz_play makes none, the last one stays readable
    eng.set_search_summary(False)
    _search(eng)
    eng.play(UNIFORMS[:Bn])
    after = eng.fetch_search_summary()
    assert all(_bits(before[k]) == _bits(after[k]) for k in ("root_q", "best_q", "surprise")) and eng.search_summary_stats() == (4, 0)
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. setter rules
def test_setter_rules():
    lib = N.lib()
    eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 16}, 3, chess960=True, learning=False)
    s = eng._stream()
    z = C.c_void_p()
    assert lib.sz_set_search_summary(None, 1, s) == N.SZ_ERR_INVALID and lib.sz_fetch_search_summary(None, z, z, z, z, s) == N.SZ_ERR_INVALID
    assert lib.sz_fetch_search_summary(eng._e, z, z, z, z, s) == N.SZ_ERR_STATE, "fetch before the option was ever on"
    assert eng.search_summary_stats() == (0, 0)
    assert lib.sz_set_search_summary(eng._e, 0, s) == N.SZ_OK, "off is always accepted"
    assert lib.sz_fetch_search_summary(eng._e, z, z, z, z, s) == N.SZ_ERR_STATE
    eng.new_games(STARTS[:3])
    eng.begin()
    for _ in range(5):
        eng.step(*eng.evaluate(eng.planes))
    assert lib.sz_set_search_summary(eng._e, 1, s) == N.SZ_ERR_STATE, "during a search"
    with pytest.raises(N.NativeError):
        eng.set_search_summary(True)
    assert not eng.search_summary and lib.sz_fetch_search_summary(eng._e, z, z, z, z, s) == N.SZ_ERR_STATE, "nothing changed"
    for _ in range(5, 16):
        eng.step(*eng.evaluate(eng.planes))
    eng.check_errors()
    eng.set_search_summary(True)                                         # the search is done: takes effect at the sz_play that follows
    assert lib.sz_fetch_search_summary(eng._e, z, z, z, z, s) == N.SZ_OK, "every pointer may be NULL"
    eng.play(UNIFORMS[:3])
    got = eng.fetch_search_summary()
    assert got["valid"].tolist() == [1, 1, 1] and eng.search_summary_stats() == (3, 0)
    eng.begin()
    eng.step(*eng.evaluate(eng.planes))
    assert lib.sz_set_search_summary(eng._e, 0, s) == N.SZ_ERR_STATE, "during a search, off too"
    assert eng.search_summary
    eng.close()

    # Gumbel's record is the improved policy and it exports v_mix itself: each refuses the other with SZ_ERR_STATE, in both directions
    g_on = SelfPlayEngine(HashModel(salt=3), {"C": 2, "num_searches": 24, "gumbel": {"m": 4}}, 8, chess960=True, learning=True)
    s = g_on._stream()
    assert lib.sz_set_search_summary(g_on._e, 1, s) == N.SZ_ERR_STATE
    assert lib.sz_set_search_summary(g_on._e, 0, s) == N.SZ_OK, "off is always accepted"
    g_on.set_gumbel(None)
    assert lib.sz_set_search_summary(g_on._e, 1, s) == N.SZ_OK
    gopt = N.sz_gumbel_options(4, 50.0, 1.0)
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_ERR_STATE
    assert lib.sz_set_gumbel(g_on._e, None, None, s) == N.SZ_OK
    assert lib.sz_set_search_summary(g_on._e, 0, s) == N.SZ_OK
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_OK
    g_on.close()
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 8, "search_targets": {"q_ratio": 1.5}}, 1)
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 24, "search_targets": {}, "gumbel": {"m": 4}}, 2)


# ------------------------------------------------------------------------------------------------ 5. play_games
@pytest.mark.parametrize("source", ["root", "best"])
def test_play_games_takes_the_option_from_args(source):
    from sigma_zero_amd.sim import play_games
    salt, starts, caps, r = 4, [0, 959, 518, 400, 77, 5], [4, 3, 4, 3, 3, 4], 0.5
    u = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    base = {"C": 2, "num_searches": 32}
    args = dict(base, search_targets={"q_ratio": r, "q_source": source})
    assert search_targets_of(args) == (r, source, 0.0)
    got = play_games(HashModel(salt=salt), args, 6, c960=True, scharnagl=starts, uniforms=u, max_plies=caps, learning=True, n_boards=4)
    off = play_games(HashModel(salt=salt), base, 6, c960=True, scharnagl=starts, uniforms=u, max_plies=caps, learning=True, n_boards=4)
    n = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for g, (start, cap) in enumerate(zip(starts, caps)):
            ref = SR.KR.Game(sz.ChessTensor(chess960=True, scharnagl=start), 32, None, reuse=False, c=2.0, learning=True, mode="dyadic", salt=salt)
            values, surprises = [], []
            while ref.live and len(values) < cap:
                ref.begin()
                ref.run()
                assert ref.error is None
                _, sm, _, _ = SR.play_ply(ref, u(g, len(values)))
                values.append(sm.best_q if source == "best" else sm.root_q)
                surprises.append(sm.surprise)
            assert got[g]["chosen_actions"] == ref.chosen, "game %d: moves played" % g
            assert _bits(got[g]["search_values"]) == _bits(values), "game %d: search values" % g
            assert _bits(got[g]["surprises"]) == _bits(surprises), "game %d: surprises" % g
            want = [(1.0 - r) * z + r * q for z, q in zip(got[g]["rewards"], values)]
            assert _bits(got[g]["value_targets"]) == _bits(want), "game %d: value_targets" % g
            assert len(got[g]["value_targets"]) == len(got[g]["states"]) == len(got[g]["rewards"])
            n += len(values)
    assert n >= 18
    for a, b in zip(got, off):
        assert a["rewards"] == b["rewards"] and a["chosen_actions"] == b["chosen_actions"] and a["sample_plies"] == b["sample_plies"]
        assert [list(x.items()) for x in a["actions"]] == [list(x.items()) for x in b["actions"]], "the policy targets are what they are without the key"
        assert all(np.array_equal(x, y) for x, y in zip(a["packed_states"], b["packed_states"]))
        assert not any(k in b for k in ("search_values", "surprises", "value_targets")), "with the key absent nothing new is stored"
    assert any(x != float(y) for a in got for x, y in zip(a["value_targets"], a["rewards"])), "the blend changes the value targets"
