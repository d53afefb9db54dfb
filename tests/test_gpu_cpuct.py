"""The visit-dependent exploration rate on the GPU (sz_set_cpuct / sz_debug_cpuct, args["cpuct"], a NON-REFERENCE option): the HIP engine against
the plain-Python restatement tests/puctref.py, bit for bit.  1. the device's rate on the CPU test's cases; 2. the engine ply after ply in the
configurations of puctref.configs() (plain; leaf batching + solver + reuse_subtree; forced playouts + FPU + endings + root noise; visit
targets; the move temperature; a kept root above num_searches), with settings that differ at root and tree: trees at search begin and end,
every network input row, the records, the position after sz_play and every counter; 3. (C, b, 0) is the engine without the option at
c_puct = C; 4. a change of the option keeps the kept subtree; 5. the setter rules; 6. sim.play_games on fewer slots than games.
tests/test_cpuct_ref.py proves on the CPU that the configurations reach the conditions they are there for; the same counters are asserted
here on the games the device was compared with."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine, cpuct_options_of
from hashmodel import HashModel, evaluate_packed, pack_planes
import puctref as PR
from puctref import Cpuct

pytestmark = pytest.mark.gpu

ST_PENDING = 2


# ------------------------------------------------------------------------------------------------ 1. the device's rate on the CPU test's cases
def test_device_rate_equals_restatement_bit_for_bit():
    hc = PR.hook_cases()
    n = len(hc.n_p)
    assert n >= 10000 and hc.opts.dtype.itemsize == C.sizeof(N.sz_cpuct_options) == 24
    want = PR.hook_reference(hc)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ins = [dev(x) for x in (hc.n_p, hc.is_root, hc.opts)]
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert N.lib().sz_debug_cpuct(*[ptr(t) for t in ins], ptr(out), n, s) == N.SZ_OK
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert not len(bad), "case %d (n_p %d, root %d, %s): device %r, restatement %r (%d differ)" % (
        bad[0], hc.n_p[bad[0]], hc.is_root[bad[0]], hc.opts[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    assert N.lib().sz_debug_cpuct(None, ptr(ins[1]), ptr(ins[2]), ptr(out), n, s) == N.SZ_ERR_INVALID
    assert N.lib().sz_debug_cpuct(*[ptr(t) for t in ins], ptr(out), 0, s) == N.SZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 2. the engine against the restatement
def _assert_tree(tag, eng, b, tree, proven):
    for x, y in zip(eng.debug_tree(b), tree):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: tree differs" % tag
    pr, co = eng.debug_tree_proven(b)
    assert np.array_equal(pr, proven[0]) and np.array_equal(co, proven[1]), "%s: proven labels / complete bits differ" % tag


def _steps(eng, searches, live, modes, tag, S):
    """the steps of one search on every live board b against searches[b]: boards pending, every network input row, step count"""
    B, L = eng.B, eng.L
    t = 0
    while True:
        torch.cuda.synchronize()
        status = eng.debug_pending()[4]
        pend = (status & ST_PENDING) != 0
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


_played = {}


def _drive(cfg, settings=None):
    """settings: per ply the Cpuct (or None = off) set before that ply's search in the configuration's place"""
    B = len(cfg.boards)
    eng = SelfPlayEngine(None, PR.engine_args(cfg), B, chess960=True, learning=cfg.learning, edges_per_board=PR.worst_case(cfg.S) if cfg.reuse else 0)
    games = [PR.new_game(cfg, b) for b in range(B)]
    modes = [(bd.mode, bd.salt) for bd in cfg.boards]
    gam = PR.gammas(cfg) if cfg.noise else None
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    if cfg.endings is not None:
        eng.set_endings(PR.FU.ER.options(**cfg.endings), [0] * B)
    n_plies = n_steps = 0                                       # what was actually driven and compared (asserted below: no vacuous pass)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(cfg.plies):
            live = [g.live for g in games]
            if not any(live):
                break
            n_plies += 1
            setting = cfg.cpuct[ply % len(cfg.cpuct)] if settings is None else settings[ply]
            eng.set_cpuct(setting)                                                  # anew before every ply: a setting of the search to come
            if cfg.targets is not None:
                eng.set_visit_targets([cfg.targets[ply][b] if live[b] else 0 for b in range(B)])
            if cfg.noise:
                eng.set_search_root_noise(torch.from_numpy(gam[ply]), [0] * B)
            if cfg.forced_k:
                eng.set_forced_playouts(cfg.forced_k, [1] * B)
            if cfg.temperature is not None:
                topt, T = cfg.temperature[ply % len(cfg.temperature)]
                eng.set_move_temperature({"visit_offset": topt.visit_offset, "value_cutoff": topt.value_cutoff if topt.use_cutoff else None}, np.full(B, T))
            for b, g in enumerate(games):
                if live[b]:
                    if settings is not None:
                        g.follow_config, g.cpuct = False, setting
                    PR.begin_ply(cfg, g, b, ply, gam)
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s board %d (%s) ply %d start=%s" % (cfg.name, b, cfg.boards[b].name, ply, games[b].starts[-1])
            eng.begin()
            if cfg.targets is not None:
                assert eng.search_goals().tolist() == [g.goals[-1] if live[b] else 0 for b, g in enumerate(games)], "%s ply %d: goals" % (cfg.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search begin", eng, b, g.search.begin_tree, g.search.begin_proven)
            n_steps += _steps(eng, [g.search for g in games], live, modes, "%s ply %d" % (cfg.name, ply), cfg.S)
            st = eng.check_errors()
            got = tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth"))
            assert got == tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits", "sum_depth")), "%s ply %d: sz_stats" % (cfg.name, ply)
            assert st["boards_pending"] == 0 and st["boards_done"] == sum(live)
            assert eng.solver_stats() == (sum(g.proven_stops for g in games), sum(g.proved for g in games)), "%s ply %d: solver counters" % (cfg.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search.tree(), g.search.tree_proven())
            u = np.array([cfg.boards[b].u(ply) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            rec = eng.fetch_ply()
            ends = eng.fetch_endings() if cfg.endings is not None else None
            for b, g in enumerate(games):
                if not live[b]:
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tag(b)
                    continue
                want = g.play(u[b])
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r, restatement %r" % (tag(b), got, want)
                if ends is not None:
                    assert int(ends["kind"][b]) == g.last[0], "%s: sz_fetch_endings" % tag(b)
                assert eng.debug_position(b)[0].tobytes() == PR.position_record(g.game), "%s: position record after sz_play" % tag(b)
            assert eng.forced_stats() == (sum(g.forced_selections for g in games), sum(g.pruned_visits for g in games)), "%s ply %d: sz_forced_stats" % (cfg.name, ply)
            if cfg.temperature is not None:
                assert eng.temperature_stats() == tuple(sum(g.temp_stats[i] for g in games) for i in range(3)), "%s ply %d: sz_temperature_stats" % (cfg.name, ply)
            if ends is not None:
                assert eng.ending_stats() == tuple(sum(g.ended[i] for g in games) for i in range(4)), "%s ply %d: sz_ending_stats" % (cfg.name, ply)
    eng.close()
    sims = sum(g.simulations for g in games)
    print("%s: %d plies, %d network steps, %d simulations, %d board searches compared" % (cfg.name, n_plies, n_steps, sims, sum(len(g.searches) for g in games)))
    assert n_plies >= 4 and n_steps >= 12 and sims >= 3 * cfg.S and st["simulations"] == sims
    return games


@pytest.mark.parametrize("name", [c.name for c in PR.configs()])
def test_engine_matches_restatement_ply_after_ply(name):
    cfg = next(c for c in PR.configs() if c.name == name)
    assert 3 <= len(cfg.boards) <= 8 and 24 <= cfg.S <= 48 and 4 <= cfg.plies <= 6
    games = _drive(cfg)
    assert all(cp is not None and PR.site(cp, True) != PR.site(cp, False) for g in games for cp in g.cpuct_plies), "the option is on, root and tree differ"
    if cfg.reuse:
        assert any(s == "reused" for g in games for s in g.starts)
    if cfg.forced_k:
        assert sum(g.forced_selections for g in games) > 0 and sum(g.pruned_visits for g in games) > 0
    if cfg.temperature is not None:
        assert sum(g.temp_stats[0] for g in games) > 0
    _played[name] = games


def test_configurations_coverage():
    """counted on the restatement, over the games the device was compared with (all of them replayed when this test runs alone)"""
    played = _played
    if len(played) < len(PR.configs()):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            played = {c.name: PR.play(c)[0] for c in PR.configs()}
    cov = PR.coverage(played.values())
    print("coverage:", {k: cov[k] for k in PR.COVERAGE})
    PR.assert_coverage(cov)


# ------------------------------------------------------------------------------------------------ 3. factor 0 is the engine without the option
STARTS = [0, 17, 518]


def _three_plies(eng):
    """three plies with HashModel evaluations -> (trees at the end of every search, records)"""
    eng.new_games(STARTS)
    trees, recs = [], []
    for ply in range(3):
        eng.search()
        eng.check_errors()
        trees.append([eng.debug_tree(b) + eng.debug_tree_proven(b) for b in range(eng.B)])
        eng.play([-1.0, 0.3, 0.7])
        recs.append(eng.fetch_ply())
    return trees, recs


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for ta, tb in zip(a, b) for x, y in zip(ta, tb))


@pytest.mark.parametrize("how", ["L4_solver_reuse", "forced_fpu"])
def test_factor_0_gives_the_trees_of_an_engine_without_the_option(how):
    Cc = 1.5
    if how == "L4_solver_reuse":
        base = {"combine_options": True, "reuse_subtree": True, "num_searches": 48, "leaves_per_step": 4, "solver": True}
    else:
        base = {"num_searches": 48, "forced_playouts": 2.0, "fpu": {"mode": "reduction", "value": 0.33, "root_mode": "absolute", "root_value": 1.0}}
    out, stats = [], []
    for args in (dict(base, C=Cc), dict(base, C=2, cpuct={"init": Cc, "base": 5, "factor": 0, "root_base": 11}), dict(base, C=2),
                 dict(base, C=Cc, cpuct={"init": Cc, "base": 4, "factor": 2})):
        eng = SelfPlayEngine(HashModel(mode="rational", salt=2), args, 3, chess960=True, learning=True)
        assert (eng.cpuct is None) == ("cpuct" not in args)
        out.append(_three_plies(eng))
        stats.append(eng.forced_stats())
        eng.close()
    (t0, r0), (t1, r1), (t2, _), (t3, _) = out
    assert stats[0] == stats[1] and (how != "forced_fpu" or (stats[0][0] > 0 and stats[0][1] > 0)), "forced selections were made and pruning ran: %r" % (stats,)
    for ply in range(3):
        assert _same(t0[ply], t1[ply]), "ply %d: trees" % ply
        assert all(r0[ply][k].tobytes() == r1[ply][k].tobytes() for k in r0[ply]), "ply %d: records" % ply
    assert not _same(t0[0], t2[0]), "C = 2, which the option's engine was created with, builds other trees: the option's init was read"
    assert not _same(t0[0], t3[0]), "... and so does a factor above 0"


# ------------------------------------------------------------------------------------------------ 4. a change on a kept subtree
def test_changing_the_option_keeps_the_subtree():
    cfg = next(c for c in PR.configs() if c.name == "L4_solver_reuse")._replace(plies=4)
    settings = [PR.A, PR.B_, None, Cpuct(1.5, 5.0, 0.0, 1.5, 11.0, 0.0)]
    games = _drive(cfg, settings)
    kept = [g for g in games if g.starts[:4] == ["new", "reused", "reused", "reused"]]
    assert len(kept) >= 2 and all(all(s.n_kept > 1 for s in g.searches[1:4]) for g in kept), [g.starts for g in games]
    assert all(g.cpuct_plies[:4] == [PR.checked(settings[0]), PR.checked(settings[1]), None, PR.checked(settings[3])][:len(g.cpuct_plies)] for g in games)


# ------------------------------------------------------------------------------------------------ 5. setter rules
def test_setter_rules():
    lib = N.lib()
    opt = lambda *v: C.byref(N.sz_cpuct_options(*v))
    nan, inf = float("nan"), float("inf")
    good = (1.25, 19652.0, 1.0, 1.25, 19652.0, 1.0)
    results = []
    for meddle in (False, True):
        eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 32, "reuse_subtree": True, "cpuct": {"init": 1.0, "base": 8, "factor": 2}}, 3,
                             chess960=True, learning=False)
        s = eng._stream()
        assert eng.cpuct == (1.0, 8.0, 2.0, 1.0, 8.0, 2.0)
        for field in range(6):                                       # each invalid field, at both sites
            kind = ("init", "base", "factor")[field % 3]
            for v in {"init": (nan, inf, -inf, -0.001, 100.5), "base": (nan, inf, 0.0, 0.999, -1.0, 1.1e9), "factor": (nan, inf, -inf, -0.001, 100.5)}[kind]:
                bad = list(good)
                bad[field] = v
                assert lib.sz_set_cpuct(eng._e, opt(*bad), s) == N.SZ_ERR_INVALID, (field, v)
        assert lib.sz_set_cpuct(None, None, s) == N.SZ_ERR_INVALID
        for ok in (good, (0.0, 1.0, 0.0, 100.0, 1e9, 100.0), (1.0, 8.0, 2.0, 1.0, 8.0, 2.0)):
            assert lib.sz_set_cpuct(eng._e, opt(*ok), s) == N.SZ_OK, ok
        eng.new_games(STARTS)
        eng.begin()
        for _ in range(5):
            eng.step(*eng.evaluate(eng.planes))
        if meddle:                                                   # during a search: refused, nothing changes
            assert lib.sz_set_cpuct(eng._e, None, s) == N.SZ_ERR_STATE
            assert lib.sz_set_cpuct(eng._e, opt(*good), s) == N.SZ_ERR_STATE
            with pytest.raises(N.NativeError):
                eng.set_cpuct((2.0, 4.0, 1.0, 2.0, 4.0, 1.0))
            assert eng.cpuct == (1.0, 8.0, 2.0, 1.0, 8.0, 2.0)
        for _ in range(27):
            eng.step(*eng.evaluate(eng.planes))
        assert eng.check_errors()["boards_done"] == 3
        trees = [[eng.debug_tree(b) for b in range(3)]]
        eng.play([-1.0, 0.3, 0.7])
        eng.search()                                                 # the next search too: a refused call left nothing behind for sz_search_begin
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(3)])
        eng.play([-1.0, 0.3, 0.7])
        if meddle:                                                   # between searches: off and on again, the kept subtrees stay
            eng.set_cpuct(None)
            assert eng.cpuct is None
            eng.set_cpuct((1.0, 8.0, 2.0, 1.0, 8.0, 2.0))
        eng.search()
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(3)])
        results.append(trees)
        eng.close()
    assert all(_same(a, b) for a, b in zip(results[0], results[1]))

    # off, then on again: the engine without the option in between
    runs = {}
    for how in ("off", "on_then_null", "on"):
        eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 32}, 3, chess960=True, learning=False)
        if how != "off":
            eng.set_cpuct((1.0, 8.0, 2.0, 2.5, 4.0, 1.0))
        if how == "on_then_null":
            assert lib.sz_set_cpuct(eng._e, None, eng._stream()) == N.SZ_OK
        runs[how] = _three_plies(eng)
        eng.close()
    assert _same(runs["off"][0][0], runs["on_then_null"][0][0]) and _same(runs["off"][0][2], runs["on_then_null"][0][2])
    assert not _same(runs["off"][0][0], runs["on"][0][0])

    # Gumbel's rule is a chain of its own: each refuses the other with SZ_ERR_STATE, in both directions
    g_on = SelfPlayEngine(HashModel(salt=3), {"C": 2, "num_searches": 24, "gumbel": {"m": 4}}, 8, chess960=True, learning=True)
    s = g_on._stream()
    assert lib.sz_set_cpuct(g_on._e, opt(*good), s) == N.SZ_ERR_STATE
    assert lib.sz_set_cpuct(g_on._e, None, s) == N.SZ_OK, "off is always accepted"
    g_on.set_gumbel(None)
    assert lib.sz_set_cpuct(g_on._e, opt(*good), s) == N.SZ_OK
    gopt = N.sz_gumbel_options(4, 50.0, 1.0)
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_ERR_STATE
    assert lib.sz_set_gumbel(g_on._e, None, None, s) == N.SZ_OK
    assert lib.sz_set_cpuct(g_on._e, None, s) == N.SZ_OK
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_OK
    g_on.close()
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 8, "cpuct": {"init": 1.25, "base": 0.5}}, 1)
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 24, "cpuct": {"init": 1.25}, "gumbel": {"m": 4}}, 2)


# ------------------------------------------------------------------------------------------------ 6. play_games end to end
def test_play_games_takes_the_option_from_args():
    from sigma_zero_amd.sim import play_games
    salt, starts, caps = 4, [0, 959, 518, 400, 77, 5], [4, 3, 4, 3, 3, 4]
    u = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    args = {"C": 2, "num_searches": 24, "cpuct": {"init": 1.0, "base": 8, "factor": 2, "root_init": 2.5, "root_base": 4, "root_factor": 1}}
    cp = Cpuct(*cpuct_options_of(args))
    assert cp == PR.A
    got = play_games(HashModel(salt=salt), args, 6, c960=True, scharnagl=starts, uniforms=u, max_plies=caps, learning=True, n_boards=4)
    off = play_games(HashModel(salt=salt), {"C": 2, "num_searches": 24}, 6, c960=True, scharnagl=starts, uniforms=u, max_plies=caps, learning=True, n_boards=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for g, (n, cap) in enumerate(zip(starts, caps)):
            ref = PR.Game(sz.ChessTensor(chess960=True, scharnagl=n), 24, None, reuse=False, c=2.0, learning=True, mode="dyadic", salt=salt, cpuct=cp)
            fractions, packed = [], []
            while ref.live and len(fractions) < cap:
                ref.begin()
                ref.run()
                assert ref.error is None
                rec = ref.play(u(g, len(fractions)))
                vis = rec["visits"][:rec["n_child"]].astype(np.int64)
                fractions.append((vis / int(vis.sum())).tolist())
                packed.append(rec["packed"])
            assert got[g]["chosen_actions"] == ref.chosen, "game %d: moves played" % g
            assert [list(a.values()) for a in got[g]["actions"]] == fractions, "game %d: the targets are the restatement's visit fractions" % g
            assert all(np.array_equal(a, b) for a, b in zip(got[g]["packed_states"], packed)), "game %d: root planes" % g
    assert [g["chosen_actions"] for g in got] != [g["chosen_actions"] for g in off], "the option changes the games: the comparison says something"
