"""The move-selection temperature on the GPU (sz_set_move_temperature / sz_fetch_temperature / sz_temperature_stats / sz_debug_temperature,
args["temperature"], a NON-REFERENCE option): the HIP engine against the plain-Python restatement tests/tempref.py, bit for bit.  1. the
device's move choice on seeded cases; 2. the engine ply after ply in three configurations (plain; solver + forced playouts + endings + FPU
with leaves_per_step 2; reuse_subtree), with temperatures that differ per board and per ply: trees at search begin (the kept subtree) and
end, records, the position after sz_play, sz_fetch_temperature and every counter; 3. T = 1 without offset and cutoff is the engine without
the option and T = 0 is the negative uniform; 4. the setter rules; 5. sim.play_games end to end on fewer slots than games.
tests/test_temp_ref.py proves on the CPU that the cases and configurations reach the branches they are there for.
p_chosen and the weights are compared by their bits, except that any NaN equals any NaN."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine, temperature_at, temperature_options_of
from hashmodel import HashModel
import tempref as TR
from forcedref import position_record, worst_case

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))


def _opts_dict(o):
    return {"visit_offset": o.visit_offset, "value_cutoff": o.value_cutoff if o.use_cutoff else None}


# ------------------------------------------------------------------------------------------------ 1. the device's move choice on seeded cases
def test_device_move_choice_on_seeded_cases():
    hc = TR.hook_cases()
    n = len(hc.T)
    widths = np.diff(hc.offsets)
    assert n >= 3000 and set(widths.tolist()) == set(TR.HOOK_K)
    assert hc.opts.dtype.itemsize == C.sizeof(N.sz_temperature_options) == 12
    move, kind, ne, p, ex, w, cov = TR.hook_reference(hc)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ins = [dev(x) for x in (hc.offsets, hc.n, hc.N, hc.W, hc.T, hc.u, hc.pmove, hc.opts)]
    i32 = lambda: torch.full((n,), -7, dtype=torch.int32, device="cuda")
    move_d, kind_d, ne_d, ex_d = i32(), i32(), i32(), i32()
    p_d = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    w_d = torch.full((len(hc.n),), math.nan, dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = N.lib().sz_debug_temperature(*[ptr(t) for t in ins], ptr(move_d), ptr(kind_d), ptr(ne_d), ptr(p_d), ptr(ex_d), ptr(w_d), n, s)
    assert rc == N.SZ_OK
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (move_d, kind_d, ne_d, ex_d)]
    got_p, got_w = p_d.cpu().numpy(), w_d.cpu().numpy()
    print("hook cases: %d cases, %d children; %s" % (n, len(hc.n), {k: int(v) for k, v in cov.items()}))
    bad_w = np.add.reduceat((~_same_bits(got_w, w)).astype(np.int64), hc.offsets[:-1]) > 0
    bad = np.nonzero((got[0] != move) | (got[1] != kind) | (got[2] != ne) | (got[3] != ex) | ~_same_bits(got_p, p) | bad_w)[0]
    assert not len(bad), "case %d (K = %d, T = %r, u = %r, opts %s): move %d kind %d n_eligible %d excluded %d p %r, restatement %d %d %d %d %r" % (
        bad[0], widths[bad[0]], hc.T[bad[0]], hc.u[bad[0]], hc.opts[bad[0]], got[0][bad[0]], got[1][bad[0]], got[2][bad[0]], got[3][bad[0]], got_p[bad[0]],
        move[bad[0]], kind[bad[0]], ne[bad[0]], ex[bad[0]], p[bad[0]])
    assert all(cov[k] > 0 for k in TR.HOOK_COVERAGE), dict(cov)
    # the same cases without a proving move and with the tree's counts taken from the sampled ones (both optional arrays NULL)
    hc2 = hc._replace(N=hc.n, pmove=np.full(n, -1, np.int32))
    move2, kind2, ne2, p2, ex2, _, _ = TR.hook_reference(hc2)
    rc = N.lib().sz_debug_temperature(ptr(ins[0]), ptr(ins[1]), None, ptr(ins[3]), ptr(ins[4]), ptr(ins[5]), None, ptr(ins[7]),
                                      ptr(move_d), ptr(kind_d), ptr(ne_d), ptr(p_d), ptr(ex_d), ptr(w_d), n, s)
    assert rc == N.SZ_OK
    torch.cuda.synchronize()
    assert np.array_equal(move_d.cpu().numpy(), move2) and np.array_equal(kind_d.cpu().numpy(), kind2) and np.array_equal(ne_d.cpu().numpy(), ne2)
    assert np.array_equal(ex_d.cpu().numpy(), ex2) and _same_bits(p_d.cpu().numpy(), p2).all() and not (kind2 == TR.PROVEN_WIN).any()
    assert N.lib().sz_debug_temperature(None, *[ptr(t) for t in ins[1:]], ptr(move_d), ptr(kind_d), ptr(ne_d), ptr(p_d), ptr(ex_d), ptr(w_d), n, s) == N.SZ_ERR_INVALID
    assert N.lib().sz_debug_temperature(*[ptr(t) for t in ins], ptr(move_d), ptr(kind_d), ptr(ne_d), ptr(p_d), ptr(ex_d), ptr(w_d), 0, s) == N.SZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 2. the engine against the restatement
def _assert_tree(tag, eng, b, tree, proven):
    for x, y in zip(eng.debug_tree(b), tree):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: tree differs" % tag
    pr, co = eng.debug_tree_proven(b)
    assert np.array_equal(pr, proven[0]) and np.array_equal(co, proven[1]), "%s: proven labels / complete bits differ" % tag


def _engine(cfg, args=None):
    return SelfPlayEngine(HashModel(salt=cfg.salt), TR.engine_args(cfg) if args is None else args, len(cfg.starts), chess960=True, learning=True,
                          edges_per_board=worst_case(cfg.S) if cfg.reuse else 0)


def _search(eng, S):
    """begin() was called: the steps of the search, the network on every row"""
    steps = 0
    while eng.pending_boards():
        assert steps < S
        eng.step(*eng.evaluate(eng.planes))
        steps += 1
    return steps


@pytest.mark.parametrize("name", [cfg.name for cfg in TR.CONFIGS])
def test_engine_matches_restatement_ply_after_ply(name):
    cfg = next(c for c in TR.CONFIGS if c.name == name)
    B = len(cfg.starts)
    assert B == 8 and cfg.S == 24 and cfg.plies == 8
    eng = _engine(cfg)
    games = [TR.new_game(cfg, b) for b in range(B)]
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    n_plies = n_moves = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(cfg.plies):
            live = [g.live for g in games]
            assert sum(live) >= 5
            n_plies += 1
            temps = TR.temps_of(ply, B)
            eng.set_move_temperature(_opts_dict(TR.OPTS[ply % len(TR.OPTS)]), temps)        # new options and new temperatures at every ply
            for b, g in enumerate(games):
                if live[b]:
                    TR.begin_ply(cfg, g, b, ply)
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s board %d ply %d T=%r start=%s" % (cfg.name, b, ply, temps[b], games[b].starts[-1])
            eng.begin()
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search begin", eng, b, g.search.begin_tree, g.search.begin_proven)
            _search(eng, cfg.S)
            st = eng.check_errors()
            assert tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth")) == \
                tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits", "sum_depth")), "%s ply %d: sz_stats" % (cfg.name, ply)
            assert st["boards_pending"] == 0 and st["boards_done"] == sum(live)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search.tree(), g.search.tree_proven())
            u = np.array([TR.uniform_of(b, ply) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            rec, tmp = eng.fetch_ply(), eng.fetch_temperature()
            ends = eng.fetch_endings() if cfg.endings is not None else None
            for b, g in enumerate(games):
                if not live[b]:
                    assert not rec["active"][b] and tmp["n_eligible"][b] == 0 and math.isnan(tmp["p_chosen"][b]), "%s: a board that did not play" % tag(b)
                    continue
                want = g.play(u[b])
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r, restatement %r" % (tag(b), got, want)
                assert int(tmp["n_eligible"][b]) == g.last_temp[0] and _same_bits(tmp["p_chosen"][b], g.last_temp[1]), \
                    "%s: sz_fetch_temperature %d %r, restatement %r" % (tag(b), tmp["n_eligible"][b], tmp["p_chosen"][b], g.last_temp)
                if ends is not None:
                    assert int(ends["kind"][b]) == g.last[0], "%s: sz_fetch_endings" % tag(b)
                    if g.last[0]:
                        assert want["chosen"] == -1 and g.last_temp[0] == 0 and math.isnan(g.last_temp[1]), "%s: an ending reads no temperature" % tag(b)
                assert eng.debug_position(b)[0].tobytes() == position_record(g.game), "%s: position record after sz_play" % tag(b)
                n_moves += want["chosen"] >= 0
            assert eng.temperature_stats() == tuple(sum(g.temp_stats[i] for g in games) for i in range(3)), "%s ply %d: sz_temperature_stats" % (cfg.name, ply)
            assert eng.forced_stats() == (sum(g.forced_selections for g in games), sum(g.pruned_visits for g in games)), "%s ply %d: sz_forced_stats" % (cfg.name, ply)
            assert eng.solver_stats() == (sum(g.proven_stops for g in games), sum(g.proved for g in games)), "%s ply %d: solver counters" % (cfg.name, ply)
            if ends is not None:
                assert eng.ending_stats() == tuple(sum(g.ended[i] for g in games) for i in range(4)), "%s ply %d: sz_ending_stats" % (cfg.name, ply)
    if cfg.reuse:                                                   # the subtree kept by the last sz_play, at one more sz_search_begin
        for b, g in enumerate(games):
            if g.live:
                TR.begin_ply(cfg, g, b, cfg.plies)
                g.run()
        eng.begin()
        for b, g in enumerate(games):
            if g.live:
                _assert_tree("%s board %d after the last ply" % (cfg.name, b), eng, b, g.search.begin_tree, g.search.begin_proven)
        _search(eng, cfg.S)
        assert all(s == "reused" for g in games for s in g.starts[1:])
    ts = eng.temperature_stats()
    eng.close()
    cov = TR.coverage(games)
    print("%s: %d plies, %d moves; sampled, greedy, excluded = %s; %s" % (cfg.name, n_plies, n_moves, ts, {k: cov[k] for k in TR.COVERAGE}))
    assert n_plies == 8 and n_moves >= 50 and ts[0] >= 30 and ts[1] >= 10 and ts[2] > 0
    if cfg.solver:
        assert cov["temp_proven_win"] > 0 and cov["temp_on_pruned_counts"] > 0 and cov["ended_resign"] > 0
    if cfg.reuse:
        assert cov["temp_on_continued_ply"] > 0


# ------------------------------------------------------------------------------------------------ 3. equivalence to the path without the option
def _plies(eng, cfg, u_of, plies=4, before=None):
    """plies with HashModel evaluations -> per ply (trees at the end of the search, record, positions)"""
    B = eng.B
    eng.new_games(list(TR.STARTS))
    out = []
    for ply in range(plies):
        if before is not None:
            before(ply)
        eng.search()
        eng.check_errors()
        trees = [eng.debug_tree(b) for b in range(B)]
        eng.play([u_of(b, ply) for b in range(B)])
        out.append((trees, eng.fetch_ply(), [eng.debug_position(b)[0].tobytes() for b in range(B)]))
    return out


def _same_run(a, b):
    for ply, ((ta, ra, pa), (tb, rb, pb)) in enumerate(zip(a, b)):
        assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for ua, ub in zip(ta, tb) for x, y in zip(ua, ub)), "ply %d: trees" % ply
        assert all(ra[k].tobytes() == rb[k].tobytes() for k in ra), "ply %d: records" % ply
        assert pa == pb, "ply %d: positions" % ply


@pytest.mark.parametrize("name", ["plain", "reuse_subtree"])
def test_temperature_1_is_the_engine_without_the_option(name):
    cfg = next(c for c in TR.CONFIGS if c.name == name)._replace(starts=TR.STARTS)
    u_of = lambda b, ply: ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    runs, stats = {}, {}
    for how in ("off", "T1", "T0", "greedy", "on_then_null"):
        eng = _engine(cfg)
        if how == "T1":
            eng.set_move_temperature(_opts_dict(TR.options()), np.ones(8))
        if how == "T0":
            eng.set_move_temperature(_opts_dict(TR.options(-0.8, 0.1)), np.zeros(8))
        if how == "on_then_null":
            eng.set_move_temperature(_opts_dict(TR.options(-0.8, 0.1)), np.full(8, 0.25))
            eng.set_move_temperature(None)
        runs[how] = _plies(eng, cfg, (lambda b, ply: -1.0) if how == "greedy" else u_of)
        stats[how] = eng.temperature_stats()
        tmp = eng.fetch_temperature()
        if how in ("off", "greedy", "on_then_null"):
            assert not tmp["n_eligible"].any() and np.isnan(tmp["p_chosen"]).all(), "off: nothing is reported"
        if how == "T0":
            assert (tmp["n_eligible"] == 1).all() and (tmp["p_chosen"] == 1.0).all()
        eng.close()
    _same_run(runs["off"], runs["T1"])
    _same_run(runs["off"], runs["on_then_null"])
    _same_run(runs["greedy"], runs["T0"])
    assert stats["off"] == stats["greedy"] == stats["on_then_null"] == (0, 0, 0)
    assert stats["T1"] == (32, 0, 0) and stats["T0"] == (0, 32, 0)
    chosen = lambda run: [r[1]["chosen"].tolist() for r in run]
    assert chosen(runs["off"]) != chosen(runs["greedy"]), "the sampled games are not the greedy ones: the comparison says something"


# ------------------------------------------------------------------------------------------------ 4. setter rules
def test_setter_rules():
    lib = N.lib()
    cfg = TR.CONFIGS[0]
    eng = _engine(cfg)
    s = eng._stream()
    temps = torch.ones(8, dtype=torch.float64, device="cuda")
    tp = C.c_void_p(temps.data_ptr())
    O = lambda off=0.0, cut=0.0, use=0: N.sz_temperature_options(off, cut, use)
    nan, inf = float("nan"), float("inf")
    assert lib.sz_set_move_temperature(None, C.byref(O()), tp, s) == N.SZ_ERR_INVALID
    assert lib.sz_set_move_temperature(eng._e, C.byref(O()), None, s) == N.SZ_ERR_INVALID, "options without temperatures"
    for bad in (O(nan), O(inf), O(-inf), O(0.0, -0.1, 1), O(0.0, nan, 1), O(0.0, inf, 1)):
        assert lib.sz_set_move_temperature(eng._e, C.byref(bad), tp, s) == N.SZ_ERR_INVALID, (bad.visit_offset, bad.value_cutoff, bad.use_cutoff)
    assert lib.sz_temperature_stats(eng._e, None, s) == N.SZ_ERR_INVALID and lib.sz_fetch_temperature(None, None, None, s) == N.SZ_ERR_INVALID
    assert eng.temperature_stats() == (0, 0, 0), "a refused call allocates and counts nothing"
    assert lib.sz_set_move_temperature(eng._e, None, None, s) == N.SZ_OK, "off while off"
    assert lib.sz_set_move_temperature(eng._e, C.byref(O(0.0, nan, 0)), tp, s) == N.SZ_OK, "use_cutoff 0: the cutoff is ignored"
    assert lib.sz_set_move_temperature(eng._e, C.byref(O(-1e30, 2.0, 1)), tp, s) == N.SZ_OK, "finite, any sign"
    assert lib.sz_set_move_temperature(eng._e, None, None, s) == N.SZ_OK
    for bad in ([1.0] * 7, [1.0] * 7 + [-0.5], [1.0] * 7 + [nan]):
        with pytest.raises(ValueError):
            eng.set_temperatures(bad)
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 24, "temperature": {"t0": -1.0}}, 2)
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 24, "temperature": {}, "gumbel": {"m": 4}}, 2)

    # during a search: refused, and nothing changes (on, new options and off alike); changing the option never drops a kept subtree
    eng.close()
    reuse = next(c for c in TR.CONFIGS if c.name == "reuse_subtree")
    u_of = lambda b, ply: ((b * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    first = TR.options(-0.8, 0.1)
    runs = []
    for meddle in (False, True):
        eng = _engine(reuse)
        eng.set_move_temperature(_opts_dict(first), np.full(8, 0.5))
        s = eng._stream()

        extra = []

        def before(ply, eng=eng, s=s, meddle=meddle, extra=extra):
            if meddle:
                eng.set_move_temperature(_opts_dict(first), np.full(8, 0.5))  # the same options again, between searches, before every ply
            if ply == 2:                                                      # one ply stepped by hand, in both runs
                eng.begin()
                assert eng.pending_boards() > 0
                if meddle:
                    assert lib.sz_set_move_temperature(eng._e, C.byref(O(2.0, 0.0, 1)), tp, s) == N.SZ_ERR_STATE
                    assert lib.sz_set_move_temperature(eng._e, None, None, s) == N.SZ_ERR_STATE
                _search(eng, reuse.S)
                eng.play([u_of(b, 99) for b in range(8)])
                extra.append((eng.fetch_ply(), eng.fetch_temperature()))
        runs.append((_plies(eng, reuse, u_of, plies=3, before=before), eng.temperature_stats(), extra[0]))
        eng.close()
    (a, sa, xa), (b, sb, xb) = runs
    _same_run(a, b)                                                           # trees included: no kept subtree was dropped, no refused call changed anything
    assert sa == sb and sa[0] + sa[1] == 32 and sa[2] > 0
    assert all(xa[0][k].tobytes() == xb[0][k].tobytes() for k in xa[0]) and np.array_equal(xa[1]["n_eligible"], xb[1]["n_eligible"])
    assert _same_bits(xa[1]["p_chosen"], xb[1]["p_chosen"]).all() and xa[0]["active"].all() and (xa[1]["n_eligible"] >= 1).all()

    # Gumbel chooses its own move: each refuses the other with SZ_ERR_STATE, in both directions
    g_on = SelfPlayEngine(HashModel(salt=3), {"C": 2, "num_searches": 24, "gumbel": {"m": 4}}, 8, chess960=True, learning=True)
    s = g_on._stream()
    assert lib.sz_set_move_temperature(g_on._e, C.byref(O()), tp, s) == N.SZ_ERR_STATE
    assert lib.sz_set_move_temperature(g_on._e, None, None, s) == N.SZ_OK, "off is always accepted"
    g_on.set_gumbel(None)
    assert lib.sz_set_move_temperature(g_on._e, C.byref(O()), tp, s) == N.SZ_OK
    gopt = N.sz_gumbel_options(4, 50.0, 1.0)
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_ERR_STATE
    assert lib.sz_set_gumbel(g_on._e, None, None, s) == N.SZ_OK
    assert lib.sz_set_move_temperature(g_on._e, None, None, s) == N.SZ_OK
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_OK
    g_on.close()


# ------------------------------------------------------------------------------------------------ 5. play_games end to end
def _restate_games(args, starts, caps, salt, uniforms, full_search=None):
    """the games of play_games on the restatement, one after another: a game's temperature follows its own ply"""
    topts = temperature_options_of(args)
    o = TR.options(topts["visit_offset"], topts["value_cutoff"])
    S, fast = args["num_searches"], (args["playout_cap"]["fast"] if "playout_cap" in args else None)
    out, stats = [], [0, 0, 0]
    for g, (n, cap) in enumerate(zip(starts, caps)):
        ref = TR.Game(sz.ChessTensor(chess960=True, scharnagl=n), S, None, reuse=False, c=2.0, learning=True, mode="dyadic", salt=salt)
        recs, fulls, temps = [], [], []
        while ref.live and len(recs) < cap:
            ply = len(recs)
            full = True if full_search is None else bool(full_search(g, ply))
            T = temperature_at(topts, ply, full=full)
            ref.set_move_temperature(o, T)
            ref.begin(None if fast is None else (S if full else fast))
            ref.run()
            assert ref.error is None
            recs.append(ref.play(uniforms(g, ply)))
            fulls.append(full)
            temps.append(T)
        stats = [a + b for a, b in zip(stats, ref.temp_stats)]
        out.append((ref, recs, fulls, temps))
    return out, tuple(stats)


def _check_games(got, want):
    for g, (ref, recs, fulls, _) in enumerate(want):
        tag = "game %d" % g
        assert got[g]["chosen_actions"] == ref.chosen and len(ref.chosen) == len(recs), tag
        assert got[g]["sample_plies"] == [p for p, f in enumerate(fulls) if f], tag
        for i, p in enumerate(got[g]["sample_plies"]):
            vis = recs[p]["visits"][:recs[p]["n_child"]].astype(np.int64)
            assert list(got[g]["actions"][i].values()) == (vis / int(vis.sum())).tolist(), "%s ply %d: the record is not tempered" % (tag, p)
            assert np.array_equal(got[g]["packed_states"][i], recs[p]["packed"]), "%s ply %d" % (tag, p)
        assert got[g]["termination"] == ("rules" if ref.over else "max_plies"), tag


def test_play_games_end_to_end():
    from sigma_zero_amd.sim import play_games
    salt, starts, caps = 4, [0, 959, 518, 400, 77, 5], [6, 3, 5, 6, 3, 4]
    uniforms = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    temp = {"t0": 2.0, "t_final": 0.25, "plies": 2, "visit_offset": -0.8, "value_cutoff": 0.5}
    args = {"C": 2, "num_searches": 24, "temperature": temp}
    stats = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = play_games(HashModel(salt=salt), args, 6, c960=True, scharnagl=starts, uniforms=uniforms, max_plies=caps, learning=True, n_boards=4, stats=stats)
        want, want_stats = _restate_games(args, starts, caps, salt, uniforms)
    _check_games(got, want)
    assert (stats["tempered_plays"], stats["greedy_plays"], stats["excluded_children"]) == want_stats and want_stats[0] >= 20 and want_stats[2] > 0
    # games 4 and 5 start on refilled slots, at a slot ply of 3: their first two plies are played at t0 again, and differ from t_final's
    assert [t[:3] for _, _, _, t in want[4:]] == [[2.0, 2.0, 0.25]] * 2
    late, _ = _restate_games(dict(args, temperature=dict(temp, plies=0)), starts, caps, salt, uniforms)
    assert any(a[0].chosen != b[0].chosen for a, b in zip(want[4:], late[4:])), "a game that began at the slot's ply would have been played differently"

    # playout cap with `fast`: fast plies at temperature 0, whatever the ply
    full_search = lambda g, ply: (g + ply) % 2 == 0
    args2 = {"C": 2, "num_searches": 24, "playout_cap": {"fast": 8, "p_full": 0.5}, "temperature": dict(temp, fast=0.0)}
    stats2 = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got2 = play_games(HashModel(salt=salt), args2, 6, c960=True, scharnagl=starts, uniforms=uniforms, full_search=full_search, max_plies=caps, learning=True,
                          n_boards=4, stats=stats2)
        want2, want_stats2 = _restate_games(args2, starts, caps, salt, uniforms, full_search)
    _check_games(got2, want2)
    assert (stats2["tempered_plays"], stats2["greedy_plays"], stats2["excluded_children"]) == want_stats2
    assert want_stats2[1] >= stats2["fast_plies"] > 0 and all(t == 0.0 for _, _, fulls, temps in want2 for f, t in zip(fulls, temps) if not f)
    # the callable override, and the key absent
    off_stats = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        zero = play_games(HashModel(salt=salt), args, 2, c960=True, scharnagl=starts[:2], uniforms=uniforms, temperature=lambda g, ply: 0.0, max_plies=2, learning=True)
        greedy = play_games(HashModel(salt=salt), {"C": 2, "num_searches": 24}, 2, c960=True, scharnagl=starts[:2], uniforms=lambda g, ply: -1.0, max_plies=2,
                            learning=True, stats=off_stats)
    assert [g["chosen_actions"] for g in zero] == [g["chosen_actions"] for g in greedy]
    assert off_stats["plies"] == 2 and not {"tempered_plays", "greedy_plays", "excluded_children"} & set(off_stats), "the key absent: the stats are what they were"
    with pytest.raises(ValueError):
        play_games(HashModel(salt=salt), {"C": 2, "num_searches": 24}, 1, temperature=lambda g, ply: 1.0)


def test_options_match_honours_the_key_per_side():
    from sigma_zero_amd.arena import play_options_match
    temp = {"t0": 1.0, "t_final": 0.0, "plies": 2, "visit_offset": -0.8}
    a, b = {"C": 2, "num_searches": 24, "temperature": temp}, {"C": 2, "num_searches": 24}
    out = [play_options_match(HashModel(salt=4), x, y, 1, chess960=True, scharnagl=[518], max_plies=4, seed=3, check_positions=True) for x, y in ((a, b), (b, b))]
    assert out[0]["plies"] == out[1]["plies"] == [4, 4] and out[0]["unfinished"] == 2
    with pytest.raises(ValueError):
        play_options_match(HashModel(salt=4), a, b, 1, sample_plies=1)
