"""First-play urgency for unvisited children on the GPU (sz_set_fpu / sz_debug_select_fpu, args["fpu"], a NON-REFERENCE option): the HIP
engine against the plain-Python restatement tests/fpuref.py, bit for bit and ply after ply — whole trees at search begin and end, proven
labels, every network input row of every step, step counts, the counters, the training records, the position after sz_play — plus the
device's selection function on seeded cases with the scores compared as bit patterns, ABSOLUTE 0 against the option switched off, a change
of the option on a kept subtree, the refusals and the Python surface.  tests/test_fpu_ref.py proves on the CPU that the scenarios and hook
cases reach the conditions they are there for; the same counters are asserted here on the games the device was compared with."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
from hashmodel import HashModel, evaluate_packed, pack_planes
import fpuref as FP
from fpuref import ABSOLUTE, REDUCTION, REFERENCE, Fpu

pytestmark = pytest.mark.gpu

ST_PENDING = 2


def _args_of(fp):
    """an Fpu as args["fpu"]"""
    if fp is None:
        return None
    return {"mode": FP.MODE_NAMES[fp.tree_mode], "value": fp.tree_value, "root_mode": FP.MODE_NAMES[fp.root_mode], "root_value": fp.root_value}


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


# ------------------------------------------------------------------------------------------------ 1. whole searches against the restatement
_played = {}


def _drive(sc, L, solver, reuse, settings=None):
    """settings: per ply the Fpu set before that ply's search (set_fpu between plies); None: the scenario's, given once as args["fpu"]"""
    B = len(sc.boards)
    args = {"combine_options": True, "C": 2, "num_searches": sc.S, "solver": solver, "leaves_per_step": L}
    if reuse:
        args["reuse_subtree"] = True
    if settings is None:
        args["fpu"] = _args_of(sc.fpu)
    eng = SelfPlayEngine(None, args, B, chess960=sc.c960, learning=sc.learning, edges_per_board=FP.worst_case(sc.S) if reuse else 0)
    games = [FP.new_game(sc, bd, L, solver, reuse) for bd in sc.boards]
    modes = [(bd.mode, bd.salt) for bd in sc.boards]
    gam = FP.gammas(sc) if sc.extras is not None else None
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    n_plies = n_steps = 0                                       # what was actually driven and compared (asserted below: no vacuous pass)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(sc.plies):
            live = [g.live for g in games]
            if not any(live):
                break
            n_plies += 1
            if sc.extras is not None:
                eng.set_visit_targets([sc.extras.targets[ply] if live[b] else 0 for b in range(B)])
                eng.set_search_root_noise(torch.from_numpy(gam[ply]), [0] * B)
                eng.set_forced_playouts(sc.extras.k[ply], [1] * B)
            if settings is not None:
                eng.set_fpu(settings[ply])
            for b, g in enumerate(games):
                if live[b]:
                    if settings is not None:
                        g.fpu = settings[ply]
                    FP.begin_ply(sc, g, b, ply, gam)
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s L=%d solver=%d reuse=%d board %d (%s) ply %d start=%s" % (sc.name, L, solver, reuse, b, sc.boards[b].name, ply, games[b].starts[-1])
            eng.begin()
            if sc.extras is not None:
                assert eng.search_goals().tolist() == [g.goals[-1] if live[b] else 0 for b, g in enumerate(games)], "%s ply %d: goals" % (sc.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search begin", eng, b, g.search.begin_tree, g.search.begin_proven)
            n_steps += _steps(eng, [g.search for g in games], live, modes, "%s ply %d" % (sc.name, ply), sc.S)
            st = eng.check_errors()
            got = tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth"))
            assert got == tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits", "sum_depth")), "%s ply %d: sz_stats" % (sc.name, ply)
            assert st["boards_pending"] == 0 and st["boards_done"] == sum(live)
            assert eng.solver_stats() == (sum(g.proven_stops for g in games), sum(g.proved for g in games)), "%s ply %d: solver counters" % (sc.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search.tree(), g.search.tree_proven())
            u = np.array([sc.boards[b].u(ply) if live[b] else 0.0 for b in range(B)], np.float64)
            eng.play(u)
            rec = eng.fetch_ply()
            for b, g in enumerate(games):
                if not live[b]:
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tag(b)
                    continue
                want = g.play(u[b])
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r" % (tag(b), got)
                assert eng.debug_position(b)[0].tobytes() == FP.position_record(g.game), "%s: position record of the new root" % tag(b)
            assert eng.forced_stats() == (sum(g.forced_selections for g in games), sum(g.pruned_visits for g in games)), "%s ply %d: sz_forced_stats" % (sc.name, ply)
    eng.close()
    sims = sum(g.simulations for g in games)
    print("%s L=%d solver=%d reuse=%d: %d plies, %d network steps, %d simulations, %d board searches compared"
          % (sc.name, L, solver, reuse, n_plies, n_steps, sims, sum(len(g.searches) for g in games)))
    assert n_plies >= 3 and n_steps >= 12 and sims >= 3 * sc.S and st["simulations"] == sims
    return games


@pytest.mark.parametrize("name,L,solver,reuse", [(sc.name, L, solver, reuse) for sc, L, solver, reuse in FP.runs()])
def test_whole_searches_match_restatement(name, L, solver, reuse):
    sc = next(s for s in FP.scenarios() if s.name == name)
    games = _drive(sc, L, solver, reuse)
    assert all(s is not None for g in games for s in g.fpu_plies)
    if reuse:
        assert any(s == "reused" for g in games for s in g.starts)
    else:
        assert all(s == "new" for g in games for s in g.starts)
    if sc.extras is not None:
        assert sum(g.forced_selections for g in games) > 0 and sum(g.pruned_visits for g in games) > 0
    _played[(name, L, solver, reuse)] = games


def test_whole_searches_coverage():
    """counted on the restatement, over the games the device was compared with (all of them replayed when this test runs alone)"""
    played = _played
    if len(played) < len(FP.runs()):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            played = {(sc.name, L, solver, reuse): FP.play(sc, L, solver, reuse) for sc, L, solver, reuse in FP.runs()}
    cov = FP.coverage(played.values())
    print("coverage:", {k: cov[k] for k in FP.COVERAGE})
    FP.assert_coverage(cov)


# ------------------------------------------------------------------------------------------------ 2. the device function on seeded cases
def _debug_select_fpu(hc):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    n, total = len(hc.parent), len(hc.N)
    ins = [dev(x) for x in (hc.offsets, hc.N, hc.K, hc.W, hc.P)]
    R = None if hc.R is None else dev(hc.R)
    tail = [dev(x) for x in (hc.parent, hc.parent_n, hc.parent_w, hc.c, hc.is_root)]
    opts = torch.from_numpy(np.frombuffer(hc.opts.tobytes(), np.uint8).copy()).cuda()
    assert opts.numel() == 16 * n
    scores = torch.full((total,), float("nan"), dtype=torch.float32, device="cuda")
    sel = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    rc = N.lib().sz_debug_select_fpu(*[ptr(t) for t in ins], None if R is None else ptr(R), *[ptr(t) for t in tail], ptr(opts), C.c_float(hc.lam),
                                     ptr(scores), ptr(sel), n, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == N.SZ_OK
    torch.cuda.synchronize()
    return scores.cpu().numpy(), sel.cpu().numpy()


@pytest.mark.parametrize("solver", [False, True])
def test_device_selection_on_seeded_cases(solver):
    hc = FP.hook_cases(solver=solver)
    widths = np.diff(hc.offsets)
    assert len(widths) >= 3000 and set(FP.HOOK_K) <= set(widths.tolist())
    scores, sel, cov = FP.hook_reference(hc)
    got_scores, got_sel = _debug_select_fpu(hc)
    print("hook cases solver=%d: %d cases, %d children; %s" % (solver, len(widths), len(hc.N), dict(cov)))
    bad = np.nonzero(got_scores.view(np.uint32) != scores.view(np.uint32))[0]                  # bit patterns
    assert not len(bad), "score of flat child %d: device %r, restatement %r (%d differ)" % (bad[0], got_scores[bad[0]], scores[bad[0]], len(bad))
    bad = np.nonzero(got_sel != sel)[0]
    assert not len(bad), "case %d (K = %d): selected %d, restatement %d (%d differ)" % (bad[0], widths[bad[0]], got_sel[bad[0]], sel[bad[0]], len(bad))
    FP.assert_coverage(cov, [k for k in FP.HOOK_COVERAGE if solver or k not in ("win_skipped", "all_win")])
    assert all(cov["site_%s_%s" % (site, mode)] > 0 for site in ("root", "tree") for mode in FP.MODE_NAMES.values())


# ------------------------------------------------------------------------------------------------ 3. ABSOLUTE 0, a change on a kept subtree
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


@pytest.mark.parametrize("L,solver", [(1, False), (4, True)])
def test_absolute_0_gives_the_trees_of_an_engine_without_the_option(L, solver):
    base = {"combine_options": True, "reuse_subtree": True, "C": 2, "num_searches": 48, "leaves_per_step": L, "solver": solver}
    out = []
    for fpu in (None, {"mode": "absolute", "value": 0.0}, {"mode": "reduction", "value": 0.33, "root_mode": "absolute", "root_value": 1.0}):
        eng = SelfPlayEngine(HashModel(mode="rational", salt=2), dict(base, fpu=fpu) if fpu else base, 3, chess960=True, learning=True)
        assert (eng.fpu is None) == (fpu is None)
        out.append(_three_plies(eng))
        eng.close()
    (t0, r0), (t1, r1), (t2, r2) = out
    for ply in range(3):
        assert _same(t0[ply], t1[ply]), "ply %d: trees" % ply
        assert all(r0[ply][k].tobytes() == r1[ply][k].tobytes() for k in r0[ply]), "ply %d: records" % ply
    assert not _same(t0[0], t2[0])                              # ... and another setting does build other trees from the same inputs


def test_changing_the_option_keeps_the_subtree():
    sc = FP.scenarios()[0]
    settings = [sc.fpu, FP.CONFIGS["ref_root_absm1_tree"], None]
    games = _drive(sc, 1, False, True, settings)
    # the greedy boards play their most visited move: the next search starts from the kept root, whatever the option was changed to
    kept = [g for g in games if g.starts == ["new", "reused", "reused"]]
    assert len(kept) >= 2 and all(g.searches[1].n_kept > 1 and g.searches[2].n_kept > 1 for g in kept), [g.starts for g in games]
    assert all(g.fpu_plies[:3] == [FP.checked(settings[0]), FP.checked(settings[1]), None][:len(g.fpu_plies)] for g in games)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_setter_rules():
    lib = N.lib()
    opt = lambda *v: C.byref(N.sz_fpu_options(*v))
    results = []
    for meddle in (False, True):
        eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 32, "fpu": {"mode": "reduction", "value": 0.5}}, 3, chess960=True, learning=False)
        s = eng._stream()
        for bad in ((3, 0.0, 0, 0.0), (-1, 0.0, 0, 0.0), (0, 0.0, 3, 0.0), (0, 0.0, 7, 0.5),
                    (ABSOLUTE, float("nan"), 0, 0.0), (ABSOLUTE, float("inf"), 0, 0.0), (ABSOLUTE, 1.5, 0, 0.0), (ABSOLUTE, -1.0001, 0, 0.0),
                    (0, 0.0, ABSOLUTE, float("nan")), (0, 0.0, ABSOLUTE, -float("inf")), (0, 0.0, ABSOLUTE, 1.0001),
                    (REDUCTION, float("nan"), 0, 0.0), (REDUCTION, float("inf"), 0, 0.0), (REDUCTION, -0.25, 0, 0.0), (REDUCTION, 2.5, 0, 0.0),
                    (0, 0.0, REDUCTION, -1.0), (0, 0.0, REDUCTION, 2.0001), (ABSOLUTE, 0.5, REDUCTION, float("nan"))):
            assert lib.sz_set_fpu(eng._e, opt(*bad), s) == N.SZ_ERR_INVALID, bad
        for good in ((ABSOLUTE, -1.0, ABSOLUTE, 1.0), (REDUCTION, 0.0, REDUCTION, 2.0), (REFERENCE, 0.0, REFERENCE, 0.0), (REDUCTION, 0.5, REDUCTION, 0.5)):
            assert lib.sz_set_fpu(eng._e, opt(*good), s) == N.SZ_OK, good
        assert lib.sz_set_fpu(None, None, s) == N.SZ_ERR_INVALID
        eng.new_games(STARTS)
        eng.begin()
        for _ in range(5):
            eng.step(*eng.evaluate(eng.planes))
        if meddle:                                                   # during a search: refused, nothing changes
            assert lib.sz_set_fpu(eng._e, None, s) == N.SZ_ERR_STATE
            assert lib.sz_set_fpu(eng._e, opt(ABSOLUTE, 1.0, ABSOLUTE, 1.0), s) == N.SZ_ERR_STATE
            with pytest.raises(N.NativeError):
                eng.set_fpu((ABSOLUTE, -1.0, ABSOLUTE, -1.0))
            assert eng.fpu == (REDUCTION, 0.5, REDUCTION, 0.5)
        for _ in range(27):
            eng.step(*eng.evaluate(eng.planes))
        assert eng.check_errors()["boards_done"] == 3
        trees = [[eng.debug_tree(b) for b in range(3)]]
        eng.play([-1.0, 0.3, 0.7])
        eng.search()                                                 # the next search too: a refused call left nothing behind for sz_search_begin
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(3)])
        if meddle:                                                   # between searches: accepted; NULL switches off
            assert lib.sz_set_fpu(eng._e, None, s) == N.SZ_OK
        results.append(trees)
        eng.close()
    assert _same(results[0][0], results[1][0]) and _same(results[0][1], results[1][1])
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 8, "fpu": {"mode": "absolute", "value": 2.0}}, 1)


# ------------------------------------------------------------------------------------------------ 5. Python surface
def test_play_games_takes_the_option_from_args():
    from sigma_zero_amd.sim import play_games
    starts, max_plies, salt = [0, 17, 518], [3, 4, 3], 4
    fp = Fpu(REDUCTION, 0.33, ABSOLUTE, 1.0)
    keys = {"C": 2, "num_searches": 32, "fpu": _args_of(fp)}
    u = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    got = play_games(HashModel(salt=salt), keys, 3, c960=True, scharnagl=starts, uniforms=u, max_plies=max_plies, learning=False)
    off = play_games(HashModel(salt=salt), {"C": 2, "num_searches": 32}, 3, c960=True, scharnagl=starts, uniforms=u, max_plies=max_plies, learning=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for g, (n, plies) in enumerate(zip(starts, max_plies)):
            ref = FP.Game(sz.ChessTensor(chess960=True, scharnagl=n), 32, None, reuse=False, c=2.0, learning=False, mode="dyadic", salt=salt, fpu=fp)
            fractions = []
            for ply in range(plies):
                ref.begin()
                ref.run()
                rec = ref.play(u(g, ply))
                vis = rec["visits"][:rec["n_child"]].astype(np.int64)
                fractions.append((vis / int(vis.sum())).tolist())
            assert got[g]["chosen_actions"] == ref.chosen, "game %d: moves played" % g
            assert [list(a.values()) for a in got[g]["actions"]] == fractions, "game %d: the targets are the restatement's visit fractions" % g
    assert any([list(a.values()) for a in got[g]["actions"]] != [list(a.values()) for a in off[g]["actions"]] for g in range(3))
