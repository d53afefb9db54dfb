"""KLD-gain early stopping on the GPU (sz_set_kld_stop / sz_search_check_stop / sz_debug_kld_gain, args["kld_stop"], a NON-REFERENCE option): the
HIP engine against the plain-Python restatement tests/kldref.py, bit for bit.  1. the device's gain on the CPU test's cases; 2. the engine ply
after ply in the configurations of kldref.configs() (plain; leaf batching + solver + reuse_subtree; forced playouts + FPU + endings + root
noise + cpuct; visit targets; budgets): goals and trees at search begin, every network input row, the stop state and the trees after every
check, trees, records and every counter at the end; 3. the invariant: a board stopped at s has the tree, record and counters of the board
searched with goal s; 4. SelfPlayEngine.search() drives the checks and shrinks the batch, and sim.play_games takes the option from args on
fewer slots than games; 5. an engine that never saw the option and one that set and cleared it; 6. the setter rules.
tests/test_kld_ref.py proves on the CPU that the configurations reach the conditions they are there for; the same counters are asserted
here on the games the device was compared with."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine, kld_stop_options_of
from hashmodel import HashModel, evaluate_packed, pack_planes
import kldref as KR
from kldref import KldStop

pytestmark = pytest.mark.gpu

ST_PENDING = 2


# ------------------------------------------------------------------------------------------------ 1. the device's gain on the CPU test's cases
def test_device_gain_equals_restatement_bit_for_bit():
    gc = KR.gain_cases()
    n = len(gc.n_child)
    assert n >= 19000 and gc.prev.shape == gc.now.shape == (n, N.SZ_MAX_MOVES) and set(KR.WIDTHS) <= set(gc.n_child.tolist())
    want = KR.gain_reference(gc)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ins = [dev(x) for x in (gc.prev, gc.now, gc.n_child)]
    out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert N.lib().sz_debug_kld_gain(*[ptr(t) for t in ins], ptr(out), n, s) == N.SZ_OK
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert not len(bad), "case %d (K %d): device %r, restatement %r (%d differ)" % (bad[0], gc.n_child[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    assert len(set(want.tolist())) > 5000, "the cases are not a handful of values"
    assert N.lib().sz_debug_kld_gain(None, ptr(ins[1]), ptr(ins[2]), ptr(out), n, s) == N.SZ_ERR_INVALID
    assert N.lib().sz_debug_kld_gain(*[ptr(t) for t in ins], ptr(out), 0, s) == N.SZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 2. the engine against the restatement
def _assert_tree(tag, eng, b, tree, proven=None):
    for x, y in zip(eng.debug_tree(b), tree):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: tree differs" % tag
    if proven is not None:
        pr, co = eng.debug_tree_proven(b)
        assert np.array_equal(pr, proven[0]) and np.array_equal(co, proven[1]), "%s: proven labels / complete bits differ" % tag


def _steps(eng, searches, live, modes, tag, S, chunk):
    """the steps of one search on every live board b against searches[b], a check after every chunk-th step: boards pending, every network
    input row, and after every check the stop state of every live board and the tree of every board that took part -> (steps, checks)"""
    B, L = eng.B, eng.L
    state = {b: (-1, 0, KR.bits(float("nan"))) for b in range(B) if live[b]}
    logs = [{e[0]: e for e in s.kld_log} if live[b] else {} for b, s in enumerate(searches)]
    t = n_checks = 0
    while True:
        torch.cuda.synchronize()
        status = eng.debug_pending()[4]
        pend = (status & ST_PENDING) != 0
        want = [bool(live[b]) and t < len(s.steps) for b, s in enumerate(searches)]
        assert pend.tolist() == want, "%s step %d: boards waiting for the network %s, restatement %s" % (tag, t, pend.tolist(), want)
        if not pend.any():
            return t, n_checks
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
            n_checks += 1
            got = eng.fetch_kld_stop()
            for b in state:
                if t in logs[b]:
                    state[b] = logs[b][t][1:4]
                    _assert_tree("%s board %d after the check at step %d" % (tag, b, t), eng, b, logs[b][t][4])
                have = (int(got["stopped_at"][b]), int(got["checks"][b]), KR.bits(got["last_gain"][b]))
                assert have == state[b], "%s board %d after the check at step %d: stopped_at / checks / last_gain %r, restatement %r" % (tag, b, t, have, state[b])


_played = {}


def _drive(cfg, settings=None):
    """settings: per ply the KldStop (or None = off) set before that ply's search in the configuration's place"""
    B = len(cfg.boards)
    eng = SelfPlayEngine(None, KR.engine_args(cfg), B, chess960=True, learning=cfg.learning, edges_per_board=KR.worst_case(cfg.S) if cfg.reuse else 0)
    games = [KR.new_game(cfg, b) for b in range(B)]
    modes = [(bd.mode, bd.salt) for bd in cfg.boards]
    gam = KR.gammas(cfg) if cfg.noise else None
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    if cfg.endings is not None:
        eng.set_endings(KR.PR.FU.ER.options(**cfg.endings), [0] * B)
    if cfg.cpuct is not None:
        eng.set_cpuct(cfg.cpuct)
    n_plies = n_steps = n_checks = 0                           # what was actually driven and compared (asserted below: no vacuous pass)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(cfg.plies):
            live = [g.live for g in games]
            if not any(live):
                break
            n_plies += 1
            setting = cfg.kld if settings is None else settings[ply]
            eng.set_kld_stop(None if setting is None else tuple(setting))           # anew before every ply: a setting of the search to come
            if cfg.targets is not None:
                eng.set_visit_targets([cfg.targets[ply][b] if live[b] else 0 for b in range(B)])
            if cfg.budgets is not None:
                eng.set_budgets([cfg.budgets[ply][b] if live[b] else 0 for b in range(B)])
            if cfg.noise:
                eng.set_search_root_noise(torch.from_numpy(gam[ply]), [0] * B)
            if cfg.forced_k:
                eng.set_forced_playouts(cfg.forced_k, [1] * B)
            for b, g in enumerate(games):
                if live[b]:
                    g.kld_stop = setting
                    KR.begin_ply(cfg, g, b, ply, gam)
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s board %d (%s) ply %d start=%s" % (cfg.name, b, cfg.boards[b].name, ply, games[b].starts[-1])
            eng.begin()
            assert eng.search_goals().tolist() == [g.search.goal0 if live[b] else 0 for b, g in enumerate(games)], "%s ply %d: goals at begin" % (cfg.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search begin", eng, b, g.search.begin_tree, g.search.begin_proven)
            chunk = -(-setting.interval // cfg.L) if setting is not None else cfg.S + 1
            st, ch = _steps(eng, [g.search for g in games], live, modes, "%s ply %d" % (cfg.name, ply), cfg.S, chunk)
            n_steps, n_checks = n_steps + st, n_checks + ch
            st = eng.check_errors()
            got = tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth"))
            assert got == tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits", "sum_depth")), "%s ply %d: sz_stats" % (cfg.name, ply)
            assert st["boards_pending"] == 0 and st["boards_done"] == sum(live)
            assert eng.solver_stats() == (sum(g.proven_stops for g in games), sum(g.proved for g in games)), "%s ply %d: solver counters" % (cfg.name, ply)
            if setting is not None:
                fin = eng.fetch_kld_stop()
                for b, g in enumerate(games):
                    if live[b]:
                        s = g.search
                        have = (int(fin["stopped_at"][b]), int(fin["checks"][b]), KR.bits(fin["last_gain"][b]))
                        assert have == (s.stopped_at, s.checks, KR.bits(s.last_gain)), "%s: sz_fetch_kld_stop at the end %r" % (tag(b), have)
            assert eng.kld_stop_stats() == tuple(sum(g.kld_stats[i] for g in games) for i in range(3)), "%s ply %d: sz_kld_stop_stats" % (cfg.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search.tree(), g.search.tree_proven())
            u = np.array([cfg.boards[b].u(ply) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            assert N.lib().sz_search_check_stop(eng._e, eng._stream()) == (N.SZ_ERR_STATE if setting is not None else N.SZ_OK), "no search is open after sz_play"
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
                assert eng.debug_position(b)[0].tobytes() == KR.position_record(g.game), "%s: position record after sz_play" % tag(b)
            assert eng.forced_stats() == (sum(g.forced_selections for g in games), sum(g.pruned_visits for g in games)), "%s ply %d: sz_forced_stats" % (cfg.name, ply)
            if ends is not None:
                assert eng.ending_stats() == tuple(sum(g.ended[i] for g in games) for i in range(4)), "%s ply %d: sz_ending_stats" % (cfg.name, ply)
    eng.close()
    sims = sum(g.simulations for g in games)
    print("%s: %d plies, %d network steps, %d checks, %d simulations, %d board searches compared, stats %r"
          % (cfg.name, n_plies, n_steps, n_checks, sims, sum(len(g.searches) for g in games), [sum(g.kld_stats[i] for g in games) for i in range(3)]))
    assert n_plies >= 3 and n_steps >= 12 and st["simulations"] == sims
    return games


@pytest.mark.parametrize("name", [c.name for c in KR.configs()])
def test_engine_matches_restatement_ply_after_ply(name):
    cfg = next(c for c in KR.configs() if c.name == name)
    assert 4 <= len(cfg.boards) <= 8 and 32 <= cfg.S <= 64 and 4 <= cfg.kld.interval <= 8
    games = _drive(cfg)
    assert all(ks == KR.checked(cfg.kld, cfg.S) for g in games for ks in g.kld_plies), "the option is on"
    assert sum(g.kld_stats[0] for g in games) > 0 and sum(g.kld_stats[2] for g in games) > 0, "boards stopped early"
    assert any(s.stopped_at < 0 and s.sims == s.goal0 > 0 for g in games for s in g.searches), "... and not all of them"
    if cfg.reuse:
        assert any(s == "reused" for g in games for s in g.starts)
    if cfg.forced_k:
        assert sum(g.forced_selections for g in games) > 0
    _played[name] = games


def test_configurations_coverage():
    """counted on the restatement, over the games the device was compared with (all of them replayed when this test runs alone)"""
    played = _played
    if len(played) < len(KR.configs()):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            played = {c.name: KR.play(c)[0] for c in KR.configs()}
    cov = KR.coverage(played.values())
    print("coverage:", {k: cov[k] for k in KR.COVERAGE})
    KR.assert_coverage(cov)


def test_changing_the_option_keeps_the_subtree():
    cfg = next(c for c in KR.configs() if c.name == "visit_targets")
    settings = [cfg.kld, None, KldStop(0.5, 8, 4), cfg.kld]
    games = _drive(cfg, settings)
    assert all(g.starts[:4] == ["new", "reused", "reused", "reused"] for g in games), [g.starts for g in games]
    kept = [s.n_kept for g in games for s in g.searches[1:4]]
    assert all(n >= 1 for n in kept) and sum(n > 1 for n in kept) >= len(kept) // 2, kept       # a search stopped after a few simulations keeps little
    assert all(g.kld_plies[:4] == [None if s is None else KR.checked(s, cfg.S) for s in settings] for g in games)


# ------------------------------------------------------------------------------------------------ 3. the invariant
STARTS = [0, 17, 518, 77, 333, 959]
UNIFORMS = [-1.0, 0.3, 0.7, -1.0, 0.55, 0.1]
KLD = {"min_gain": 5e-3, "interval": 8, "min_simulations": 0}


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for ta, tb in zip(a, b) for x, y in zip(ta, tb))


@pytest.mark.parametrize("how", ["L1_budgets", "L4_reuse_visit_targets"])
def test_a_board_stopped_at_s_is_the_board_searched_with_goal_s(how):
    S, Bn = 48, len(STARTS)
    if how == "L1_budgets":
        base = {"C": 2, "num_searches": S}
    else:
        base = {"C": 2, "num_searches": S, "reuse_subtree": True, "visit_targets": True, "combine_options": True, "leaves_per_step": 4, "virtual_loss": 1.0}
    model = lambda: HashModel(mode="rational", salt=2)
    a = SelfPlayEngine(model(), dict(base, kld_stop=KLD), Bn, chess960=True, learning=True)
    b = SelfPlayEngine(model(), base, Bn, chess960=True, learning=True)
    assert a.kld_stop == (5e-3, 8, 0) and b.kld_stop is None
    a.new_games(STARTS)
    b.new_games(STARTS)
    n_stopped = n_full = 0
    for ply in range(3):
        a.search()
        sa = a.check_errors()
        goals = a.search_goals()
        stop = a.fetch_kld_stop()["stopped_at"]
        made = np.where(stop >= 0, stop, goals)
        assert ((stop < 0) | (stop <= goals)).all() and a.last_rows <= a.last_steps * Bn * a.L
        n_stopped, n_full = n_stopped + int((stop >= 0).sum()), n_full + int(((stop < 0) & (goals > 0)).sum())
        if how == "L1_budgets":
            b.set_budgets(made)
        else:
            b.set_visit_targets(made + S - goals)                   # goal = target + 1 - N_kept at a target of S, so N_kept - 1 = S - goal
        b.search()
        sb = b.check_errors()
        assert b.search_goals().tolist() == made.tolist(), "ply %d: the second engine's goals are where the first one's boards stopped" % ply
        for k in ("simulations", "expansions", "terminal_hits", "sum_depth", "sum_children", "boards_done"):
            assert sa[k] == sb[k], "ply %d: sz_get_stats %s %r against %r" % (ply, k, sa[k], sb[k])
        ta = [a.debug_tree(i) + a.debug_tree_proven(i) for i in range(Bn)]
        tb = [b.debug_tree(i) + b.debug_tree_proven(i) for i in range(Bn)]
        for i in range(Bn):
            assert _same([ta[i]], [tb[i]]), "ply %d board %d (stopped at %d of %d): trees" % (ply, i, stop[i], goals[i])
        a.play(UNIFORMS)
        b.play(UNIFORMS)
        ra, rb = a.fetch_ply(), b.fetch_ply()
        assert all(ra[k].tobytes() == rb[k].tobytes() for k in ra), "ply %d: records" % ply
    print("%s: %d board searches stopped early, %d ran their goal, stats %r" % (how, n_stopped, n_full, a.kld_stop_stats()))
    assert n_stopped >= 3 and a.kld_stop_stats()[0] == n_stopped and a.kld_stop_stats()[2] > 0 and b.kld_stop_stats() == (0, 0, 0)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. search() drives it; play_games
def test_search_drives_the_checks_and_shrinks_the_batch():
    S, Bn = 64, len(STARTS)
    eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": S, "kld_stop": KLD}, Bn, chess960=True, learning=True)
    eng.new_games(STARTS)
    eng.search()
    eng.check_errors()
    stop = eng.fetch_kld_stop()
    made = np.where(stop["stopped_at"] >= 0, stop["stopped_at"], S)
    print("stopped_at %s, checks %s, steps %d, rows %d" % (stop["stopped_at"].tolist(), stop["checks"].tolist(), eng.last_steps, eng.last_rows))
    assert (stop["stopped_at"] >= 0).any() and made.min() < made.max(), "boards stop, and not all at once"
    assert eng.n_rows < Bn, "the batch shrank to the boards still searching"
    assert eng.last_steps == made.max() and eng.last_rows < eng.last_steps * Bn * eng.L
    assert eng.last_rows >= int(made.sum()), "every simulation of a fresh search at L = 1 is one network row"
    assert eng.search_goals().tolist() == [S] * Bn
    eng.play(UNIFORMS)
    rec = eng.fetch_ply()
    assert [int(rec["visits"][b].sum()) for b in range(Bn)] == (made - 1).tolist(), "a fresh root's children hold the simulations made but the root's own"
    st = eng.kld_stop_stats()
    assert st[0] == int((stop["stopped_at"] >= 0).sum()) and st[1] == int(stop["checks"].sum()) and st[2] == int((S - made).sum())
    eng.search()                                                   # the next ply: the caller's mapping is back, every board searches again
    eng.check_errors()
    assert eng.search_goals().tolist() == [S] * Bn and eng.kld_stop_stats()[1] > st[1]
    eng.close()


def test_play_games_takes_the_option_from_args():
    from sigma_zero_amd.sim import play_games
    salt, starts, caps = 4, [0, 959, 518, 400, 77, 5], [4, 3, 4, 3, 3, 4]
    u = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    args = {"C": 2, "num_searches": 48, "kld_stop": {"min_gain": 8e-3, "interval": 8, "min_simulations": 16}}
    ks = KldStop(*kld_stop_options_of(args))
    assert ks == KldStop(8e-3, 8, 16)
    got = play_games(HashModel(salt=salt), args, 6, c960=True, scharnagl=starts, uniforms=u, max_plies=caps, learning=True, n_boards=4)
    off = play_games(HashModel(salt=salt), {"C": 2, "num_searches": 48}, 6, c960=True, scharnagl=starts, uniforms=u, max_plies=caps, learning=True, n_boards=4)
    n_stopped = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for g, (n, cap) in enumerate(zip(starts, caps)):
            ref = KR.Game(sz.ChessTensor(chess960=True, scharnagl=n), 48, None, reuse=False, c=2.0, learning=True, mode="dyadic", salt=salt, kld_stop=ks)
            fractions, packed = [], []
            while ref.live and len(fractions) < cap:
                ref.begin()
                ref.run()
                assert ref.error is None
                rec = ref.play(u(g, len(fractions)))
                vis = rec["visits"][:rec["n_child"]].astype(np.int64)
                fractions.append((vis / int(vis.sum())).tolist())
                packed.append(rec["packed"])
            n_stopped += ref.kld_stats[0]
            assert got[g]["chosen_actions"] == ref.chosen, "game %d: moves played" % g
            assert [list(a.values()) for a in got[g]["actions"]] == fractions, "game %d: the targets are the restatement's visit fractions" % g
            assert all(np.array_equal(a, b) for a, b in zip(got[g]["packed_states"], packed)), "game %d: root planes" % g
    assert n_stopped >= 3, "searches stopped early, a refilled slot's included: %d" % n_stopped
    assert [[list(a.values()) for a in g["actions"]] for g in got] != [[list(a.values()) for a in g["actions"]] for g in off], "the option changes the records"


# ------------------------------------------------------------------------------------------------ 5. option off
def _three_plies(eng, meddle=False):
    eng.new_games(STARTS[:3])
    trees, recs = [], []
    for ply in range(3):
        eng.begin()
        for t in range(eng.S):
            eng.step(*eng.evaluate(eng.planes))
            if meddle and t % 5 == 4:
                assert N.lib().sz_search_check_stop(eng._e, eng._stream()) == N.SZ_OK
        eng.check_errors()
        trees.append([eng.debug_tree(b) + eng.debug_tree_proven(b) for b in range(eng.B)])
        eng.play(UNIFORMS[:3])
        recs.append(eng.fetch_ply())
    return trees, recs


def test_option_off_is_the_engine_without_it():
    runs = {}
    for how in ("never", "set_then_cleared", "never_with_checks", "on"):
        eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 32, "reuse_subtree": True}, 3, chess960=True, learning=False)
        assert N.lib().sz_search_check_stop(eng._e, eng._stream()) == N.SZ_OK, "off: a no-op that succeeds, before a search too"
        if how in ("set_then_cleared", "on"):
            eng.set_kld_stop((0.5, 4, 0))
            assert N.lib().sz_search_check_stop(eng._e, eng._stream()) == N.SZ_ERR_STATE, "on: before a search"
        if how == "set_then_cleared":
            eng.set_kld_stop(None)
            assert eng.kld_stop is None and eng.kld_stop_stats() == (0, 0, 0)
        runs[how] = _three_plies(eng, meddle=how != "never")
        if how == "never":
            assert eng.kld_stop_stats() == (0, 0, 0)
            with pytest.raises(N.NativeError):
                eng.fetch_kld_stop()
        eng.close()
    for how in ("set_then_cleared", "never_with_checks"):
        for ply in range(3):
            assert _same(runs["never"][0][ply], runs[how][0][ply]), "%s ply %d: trees" % (how, ply)
            assert all(runs["never"][1][ply][k].tobytes() == runs[how][1][ply][k].tobytes() for k in runs["never"][1][ply]), "%s ply %d: records" % (how, ply)
    assert not _same(runs["never"][0][0], runs["on"][0][0]), "a threshold of 0.5 stops every board: the option was read"


# ------------------------------------------------------------------------------------------------ 6. setter rules
def test_setter_rules():
    lib = N.lib()
    opt = lambda *v: C.byref(N.sz_kld_stop_options(*v))
    nan, inf = float("nan"), float("inf")
    assert C.sizeof(N.sz_kld_stop_options) == 16
    results = []
    for meddle in (False, True):
        eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 32, "reuse_subtree": True, "kld_stop": {"min_gain": 3e-2, "interval": 8}}, 3,
                             chess960=True, learning=False)
        s = eng._stream()
        assert eng.kld_stop == (3e-2, 8, 0)
        for bad in ((nan, 8, 0), (inf, 8, 0), (-inf, 8, 0), (0.0, 8, 0), (-1e-6, 8, 0), (1.0000001, 8, 0), (8e-3, 0, 0), (8e-3, -1, 0), (8e-3, 33, 0),
                    (8e-3, 8, -1), (8e-3, 8, 33)):
            assert lib.sz_set_kld_stop(eng._e, opt(*bad), s) == N.SZ_ERR_INVALID, bad
        assert lib.sz_set_kld_stop(None, None, s) == N.SZ_ERR_INVALID and lib.sz_search_check_stop(None, s) == N.SZ_ERR_INVALID
        for ok in ((1.0, 1, 0), (5e-324, 32, 32), (3e-2, 8, 0)):
            assert lib.sz_set_kld_stop(eng._e, opt(*ok), s) == N.SZ_OK, ok
        eng.new_games(STARTS[:3])
        eng.begin()
        for _ in range(5):
            eng.step(*eng.evaluate(eng.planes))
        if meddle:                                                   # during a search: refused, nothing changes
            assert lib.sz_set_kld_stop(eng._e, None, s) == N.SZ_ERR_STATE
            assert lib.sz_set_kld_stop(eng._e, opt(0.5, 4, 0), s) == N.SZ_ERR_STATE
            with pytest.raises(N.NativeError):
                eng.set_kld_stop((0.5, 4, 0))
            assert eng.kld_stop == (3e-2, 8, 0)
        for t in range(5, 32):
            eng.step(*eng.evaluate(eng.planes))
            if t % 8 == 7:
                eng.check_stop()
        assert eng.check_errors()["boards_done"] == 3
        trees = [[eng.debug_tree(b) for b in range(3)]]
        stops = [eng.fetch_kld_stop()["stopped_at"].tolist()]
        eng.play(UNIFORMS[:3])
        eng.search()                                                 # the next search too: a refused call left nothing behind
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(3)])
        stops.append(eng.fetch_kld_stop()["stopped_at"].tolist())
        eng.play(UNIFORMS[:3])
        if meddle:                                                   # between searches: off and on again, the kept subtrees stay
            eng.set_kld_stop(None)
            assert eng.kld_stop is None
            eng.set_kld_stop((3e-2, 8, 0))
        eng.search()
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(3)])
        stops.append(eng.fetch_kld_stop()["stopped_at"].tolist())
        assert any(int(t[2][0]) > 1 for t in [eng.debug_tree(b) for b in range(3)]), "kept subtrees"
        results.append((trees, stops))
        eng.close()
    assert all(_same(a, b) for a, b in zip(results[0][0], results[1][0])) and results[0][1] == results[1][1]
    assert any(x >= 0 for row in results[0][1] for x in row), "boards stopped: %r" % (results[0][1],)

    # sequential halving plans on the goal: each refuses the other with SZ_ERR_STATE, in both directions
    g_on = SelfPlayEngine(HashModel(salt=3), {"C": 2, "num_searches": 24, "gumbel": {"m": 4}}, 8, chess960=True, learning=True)
    s = g_on._stream()
    good = (8e-3, 8, 0)
    assert lib.sz_set_kld_stop(g_on._e, opt(*good), s) == N.SZ_ERR_STATE
    assert lib.sz_set_kld_stop(g_on._e, None, s) == N.SZ_OK, "off is always accepted"
    g_on.set_gumbel(None)
    assert lib.sz_set_kld_stop(g_on._e, opt(*good), s) == N.SZ_OK
    gopt = N.sz_gumbel_options(4, 50.0, 1.0)
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_ERR_STATE
    assert lib.sz_set_gumbel(g_on._e, None, None, s) == N.SZ_OK
    assert lib.sz_set_kld_stop(g_on._e, None, s) == N.SZ_OK
    assert lib.sz_set_gumbel(g_on._e, C.byref(gopt), None, s) == N.SZ_OK
    g_on.close()
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 8, "kld_stop": {"interval": 9}}, 1)
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 24, "kld_stop": {}, "gumbel": {"m": 4}}, 2)
