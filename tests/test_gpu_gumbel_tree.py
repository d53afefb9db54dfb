"""Completed-Q selection below the root of a Gumbel search on the GPU (sz_set_gumbel_tree / sz_gumbel_tree_stats / sz_debug_gumbel_tree /
sz_debug_tree_values, args["gumbel_tree"], a NON-REFERENCE option): the HIP engine against the plain-Python restatement
tests/gumbeltreeref.py, bit for bit — the selected child, every score and v_mix on seeded child sets; whole searches tree by tree and node
value by node value after every step, with the counters after every search and the records, the improved policy, v_mix and the position
after sz_play — plus off-means-off, the setter's rules and play_games.  tests/test_gumbel_tree_ref.py proves on the CPU that the scenarios
and hook cases reach the conditions they are there for; the same counters are asserted here on the games the device was compared with."""
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
import gumbelref as GB
import gumbeltreeref as GT
from gumbelref import Gumbel

pytestmark = pytest.mark.gpu

ST_PENDING, ST_DONE, ST_ERROR, ST_SEARCHING = 2, 4, 16, 32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ (a) the device function on seeded cases
def test_device_rule_on_seeded_cases():
    hc = GT.hook_cases()
    widths = np.diff(hc.offsets)
    n, total = len(hc.vhat), len(hc.N)
    assert n >= 500 and set(GT.HOOK_K) <= set(widths.tolist()) and widths.min() == 1 and widths.max() == 218
    sel, score, vmix, cov = GT.hook_reference(hc)
    ins = [_dev(x) for x in (hc.offsets, hc.N, hc.W, hc.P, hc.vhat)]
    opts = torch.from_numpy(np.frombuffer(hc.opts.tobytes(), np.uint8).copy()).cuda()
    assert opts.numel() == 12 * n
    gscore = torch.full((total,), float("nan"), dtype=torch.float64, device="cuda")
    gsel = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    gvmix = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    rc = N.lib().sz_debug_gumbel_tree(*[_ptr(t) for t in ins], _ptr(opts), _ptr(gscore), _ptr(gsel), _ptr(gvmix), n, _stream())
    assert rc == N.SZ_OK
    torch.cuda.synchronize()
    gscore, gsel, gvmix = gscore.cpu().numpy(), gsel.cpu().numpy(), gvmix.cpu().numpy()
    print("hook cases: %d cases, %d children; %s" % (n, total, dict(cov)))
    bad = np.nonzero(gvmix.view(np.uint64) != vmix.view(np.uint64))[0]
    assert not len(bad), "v_mix of case %d (K = %d): device %r, restatement %r (%d differ)" % (bad[0], widths[bad[0]], gvmix[bad[0]], vmix[bad[0]], len(bad))
    bad = np.nonzero(gscore.view(np.uint64) != score.view(np.uint64))[0]
    assert not len(bad), "score of flat child %d: device %r, restatement %r (%d differ)" % (bad[0], gscore[bad[0]], score[bad[0]], len(bad))
    bad = np.nonzero(gsel != sel)[0]
    assert not len(bad), "selection, case %d (K = %d): device %d, restatement %d (%d differ)" % (bad[0], widths[bad[0]], gsel[bad[0]], sel[bad[0]], len(bad))
    GT.assert_coverage(cov, GT.HOOK_COVERAGE)


# ------------------------------------------------------------------------------------------------ (b) whole searches against the restatement
_played = {}


def _fpu_args(fp):
    return {"mode": FP.MODE_NAMES[fp.tree_mode], "value": fp.tree_value, "root_mode": FP.MODE_NAMES[fp.root_mode], "root_value": fp.root_value}


def _assert_tree(tag, eng, b, tree, values):
    for x, y in zip(eng.debug_tree(b), tree):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: tree differs" % tag
    got = eng.debug_tree_values(b)
    assert _bits_equal(got, values), "%s: node values differ" % tag


def _steps(eng, games, live, modes, tag, S, slot, compact):
    """test_gpu_gumbel's step loop, with the node values beside the tree after every step"""
    B = eng.B
    searches = [g.search for g in games]
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
        if compact:
            searching = ((status & ST_SEARCHING) != 0) & ((status & (ST_DONE | ST_ERROR)) == 0)
            if searching.sum() < (slot >= 0).sum():
                assert eng.compact_searching() == int(searching.sum())
                slot = np.where(searching, np.cumsum(searching) - 1, -1)
        planes = pack_planes(eng.planes.float().cpu().numpy())
        pol = np.zeros((B, N.SZ_ACTIONS), np.float32)
        val = np.zeros(B, np.float32)
        for b in np.nonzero(pend)[0]:
            row = searches[b].steps[t]
            assert len(row) == 1 and slot[b] >= 0 and np.array_equal(planes[slot[b]], row[0]), "%s step %d board %d: network input row differs" % (tag, t, b)
            pol[slot[b]], val[slot[b]] = evaluate_packed(row[0], *modes[b])
        eng.step(torch.from_numpy(pol).cuda(), torch.from_numpy(val).cuda())
        torch.cuda.synchronize()
        for b in np.nonzero(pend)[0]:
            _assert_tree("%s board %d after step %d" % (tag, b, t), eng, b, searches[b].step_trees[t], searches[b].step_values[t])
        t += 1


def _drive(sc):
    B = len(sc.boards)
    args = {"C": 2, "num_searches": sc.S, "gumbel": {"m": sc.gumbel.m, "c_visit": sc.gumbel.c_visit, "c_scale": sc.gumbel.c_scale}, "gumbel_tree": True}
    if sc.fpu is not None:
        args["fpu"] = _fpu_args(sc.fpu)                            # on, and ignored below the root
    eng = SelfPlayEngine(None, args, B, chess960=True, learning=sc.learning)
    assert eng.gumbel == tuple(GB.checked(sc.gumbel)) and eng.gumbel_tree is True
    games = [GT.new_game(sc, bd) for bd in sc.boards]
    modes = [(bd.mode, bd.salt) for bd in sc.boards]
    gs = GT.gumbels(sc)
    for b, g in enumerate(games):
        eng.upload_game(b, g.game)
    n_plies = n_steps = errors = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for ply in range(sc.plies):
            live = [g.live for g in games]
            if not any(live):
                break
            n_plies += 1
            eng.set_budgets([sc.boards[b].budgets[ply] if live[b] else 0 for b in range(B)])
            eng.set_gumbel(eng.gumbel, None if gs is None else gs[ply])          # as play_games does at every ply: the flag stays
            for b, g in enumerate(games):
                if live[b]:
                    g.begin(sc.boards[b].budgets[ply], None if gs is None else gs[ply][b])
                    g.run()
                    assert g.error is None
            tag = lambda b: "%s board %d (%s) ply %d" % (sc.name, b, sc.boards[b].name, ply)
            slot = np.arange(B)
            if sc.compact:
                assert eng.compact() == sum(live)
                slot = np.where(live, np.cumsum(live) - 1, -1)
            eng.begin()
            assert eng.search_goals().tolist() == [g.goals[-1] if live[b] else 0 for b, g in enumerate(games)], "%s ply %d: goals" % (sc.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search begin", eng, b, g.search.begin_tree, np.full(1, np.nan, np.float32))
            n_steps += _steps(eng, games, live, modes, "%s ply %d" % (sc.name, ply), sc.S, slot, sc.compact)
            st = eng.stats()
            got = tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth"))
            assert got == tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits", "sum_depth")), "%s ply %d: sz_stats" % (sc.name, ply)
            assert st["boards_pending"] == 0 and st["boards_done"] == sum(live) and st["boards_error"] == errors
            assert eng.gumbel_stats() == (sum(g.gumbel_selections for g in games), 0), "%s ply %d: sz_gumbel_stats" % (sc.name, ply)
            assert eng.gumbel_tree_stats() == sum(g.tree_selections for g in games), "%s ply %d: sz_gumbel_tree_stats" % (sc.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    s = g.search
                    _assert_tree(tag(b) + " at search end", eng, b, s.tree(), s.tree_values() if s.tree_rule else np.full(1, np.nan, np.float32))
            u = np.full(B, 0.5, np.float64)                        # not read
            eng.play(u)
            rec, out = eng.fetch_ply(), eng.fetch_gumbel()
            status = eng.debug_pending()[4]
            for b, g in enumerate(games):
                if not live[b]:
                    assert not rec["active"][b], "%s: a record for a board that did not play" % tag(b)
                    continue
                want = GB.play_or_flag(g, u[b])
                if want is None:                                   # nothing to play: SZ_ERR_ZERO_VISITS, as without the option
                    errors += 1
                    assert (status[b] & ST_ERROR) and not rec["active"][b], "%s: zero visits not flagged" % tag(b)
                    continue
                assert rec["active"][b] == 1 and np.array_equal(rec["packed"][b], want["packed"]), "%s: training record, root planes" % tag(b)
                assert np.array_equal(rec["action"][b], want["action"]) and np.array_equal(rec["visits"][b], want["visits"]), "%s: training record, visits" % tag(b)
                got = tuple(int(rec[k][b]) for k in ("n_child", "colour", "chosen", "game_over", "result"))
                assert got == tuple(int(want[k]) for k in ("n_child", "colour", "chosen", "game_over", "result")), "%s: training record %r" % (tag(b), got)
                assert _bits_equal(out["policy"][b], want["policy"]), "%s: improved policy" % tag(b)
                assert np.float64(out["v_mix"][b]).tobytes() == np.float64(want["v_mix"]).tobytes(), "%s: v_mix" % tag(b)
                assert np.float32(out["root_value"][b]).tobytes() == np.float32(want["root_value"]).tobytes(), "%s: root value" % tag(b)
                assert eng.debug_position(b)[0].tobytes() == GT.position_record(g.game), "%s: position record of the new root" % tag(b)
            st = eng.stats()
            assert st["boards_error"] == errors and (errors == 0 or st["first_error"] == N.SZ_ERR_ZERO_VISITS)
    eng.close()
    print("%s: %d plies, %d network steps, %d simulations, %d selections below the root, %d board searches compared"
          % (sc.name, n_plies, n_steps, sum(g.simulations for g in games), sum(g.tree_selections for g in games), sum(len(g.searches) for g in games)))
    assert n_plies == 3 and n_steps >= 100 and sum(g.tree_selections for g in games) > 0
    return games


@pytest.mark.parametrize("name", [sc.name for sc in GT.scenarios()])
def test_whole_searches_match_restatement(name):
    sc = next(s for s in GT.scenarios() if s.name == name)
    games = _drive(sc)
    assert all(g.tree_plies and all(g.tree_plies) for g in games)
    _played[name] = games


def test_whole_searches_coverage():
    """counted on the restatement, over the games the device was compared with (all of them replayed when this test runs alone)"""
    scs = GT.scenarios()
    played = _played
    if len(played) < len(scs):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            played = {sc.name: GT.play(sc) for sc in scs}
    ordered = [played[sc.name] for sc in scs]
    cov = GT.coverage(ordered)
    print("coverage:", {k: cov[k] for k in GT.COVERAGE})
    GT.assert_coverage(cov)
    GT.assert_every_board_selects(scs, ordered)


# ------------------------------------------------------------------------------------------------ (c) off means off
STARTS = [0, 17, 518]


def _three_plies(eng):
    eng.new_games(STARTS)
    trees, recs = [], []
    for ply in range(3):
        eng.search()
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(eng.B)])
        eng.play([-1.0, 0.3, 0.7])
        recs.append(eng.fetch_ply())
    return trees, recs


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def _equal_runs(got, want):
    for ply in range(3):
        assert _same(got[0][ply], want[0][ply]), "ply %d: trees" % ply
        assert all(got[1][ply][k].tobytes() == want[1][ply][k].tobytes() for k in want[1][ply]), "ply %d: records" % ply


def test_off_means_off():
    base = {"C": 2, "num_searches": 32, "gumbel": {"m": 4}}
    model = lambda: HashModel(mode="rational", salt=2)
    fresh = SelfPlayEngine(model(), base, 3, chess960=True, learning=False)
    want = _three_plies(fresh)                                       # Gumbel alone, the flag never set
    assert fresh.gumbel_tree_stats() == 0 and fresh.gumbel_tree is False
    with pytest.raises(N.NativeError):
        fresh.debug_tree_values(0)                                   # never switched on: no values to show
    fresh.close()
    used = SelfPlayEngine(model(), dict(base, gumbel_tree=True), 3, chess960=True, learning=False)
    t_on, _ = _three_plies(used)                                     # the rule in use ...
    n_on = used.gumbel_tree_stats()
    assert n_on > 0 and not _same(t_on[0], want[0][0])               # ... builds other trees from the same inputs
    used.set_gumbel_tree(False)                                      # ... and switched off
    assert used.gumbel_tree is False
    _equal_runs(_three_plies(used), want)
    with pytest.raises(N.NativeError):
        used.debug_tree_values(0)                                    # the search begun last kept none
    used.set_gumbel_tree(True)                                       # set and cleared again without a search in between
    used.set_gumbel_tree(False)
    _equal_runs(_three_plies(used), want)
    used.set_gumbel_tree(True)
    used.set_gumbel(None)                                            # sz_set_gumbel(NULL) clears the flag ...
    assert used.gumbel is None and used.gumbel_tree is False
    used.set_gumbel((4, 50.0, 1.0))                                  # ... and sz_set_gumbel(opt) leaves it cleared: gumbelref's trees
    _equal_runs(_three_plies(used), want)
    assert used.gumbel_tree_stats() == n_on                          # nothing was selected by the rule since
    used.close()
    # the trees with the flag off are the restatement's, gumbelref's (STARTS[1], ply 0)
    ref = GB.Game(sz.ChessTensor(chess960=True, scharnagl=STARTS[1]), 32, None, reuse=False, c=2.0, learning=False, mode="rational", salt=2, gumbel=Gumbel(4, 50.0, 1.0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ref.begin(None, None)
        ref.run()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(want[0][0][1], ref.search.tree()))


# ------------------------------------------------------------------------------------------------ (d) the setter's rules
def test_setter_rules():
    lib = N.lib()
    gopt = lambda *v: C.byref(N.sz_gumbel_options(*v))
    out = (C.c_uint64 * 1)()
    eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 32}, 3, chess960=True, learning=False)
    s = eng._stream()
    assert lib.sz_set_gumbel_tree(None, 1, s) == N.SZ_ERR_INVALID and lib.sz_gumbel_tree_stats(None, out, s) == N.SZ_ERR_INVALID
    assert lib.sz_gumbel_tree_stats(eng._e, None, s) == N.SZ_ERR_INVALID
    assert lib.sz_set_gumbel_tree(eng._e, 1, s) == N.SZ_ERR_STATE          # Gumbel is not on for the next search
    assert lib.sz_set_gumbel_tree(eng._e, 0, s) == N.SZ_OK                 # switching off is always accepted between searches
    assert lib.sz_gumbel_tree_stats(eng._e, out, s) == N.SZ_OK and out[0] == 0
    assert lib.sz_set_gumbel(eng._e, gopt(4, 50.0, 1.0), None, s) == N.SZ_OK
    assert lib.sz_set_gumbel_tree(eng._e, 1, s) == N.SZ_OK
    assert lib.sz_set_fpu(eng._e, C.byref(N.sz_fpu_options(FP.REDUCTION, 0.33, FP.ABSOLUTE, 1.0)), s) == N.SZ_OK      # accepted beside the rule
    assert lib.sz_set_fpu(eng._e, None, s) == N.SZ_OK
    assert lib.sz_set_gumbel(eng._e, None, None, s) == N.SZ_OK             # clears the flag ...
    assert lib.sz_set_gumbel(eng._e, gopt(4, 50.0, 1.0), None, s) == N.SZ_OK
    eng.new_games(STARTS)
    eng.search()
    assert eng.gumbel_tree_stats() == 0                                    # ... so this search ran without the rule
    n = C.c_int32()
    assert lib.sz_debug_tree_values(eng._e, 0, 0, None, C.byref(n), s) == N.SZ_ERR_STATE
    assert lib.sz_debug_tree_values(eng._e, 3, 0, None, C.byref(n), s) == N.SZ_ERR_INVALID and lib.sz_debug_tree_values(eng._e, 0, 0, None, None, s) == N.SZ_ERR_INVALID
    eng.close()
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 8, "gumbel_tree": True}, 1)
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 8, "gumbel": {"m": 4}, "gumbel_tree": 1}, 1)
    # during a search: refused, nothing changes; and a call between a search's end and its sz_play changes neither that sz_play nor that tree
    results = []
    for meddle in (False, True):
        eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 32, "gumbel": {"m": 4}, "gumbel_tree": True}, 3, chess960=True, learning=False)
        s = eng._stream()
        eng.new_games(STARTS)
        eng.begin()
        for _ in range(5):
            eng.step(*eng.evaluate(eng.planes))
        if meddle:
            assert lib.sz_set_gumbel_tree(eng._e, 0, s) == N.SZ_ERR_STATE
            assert lib.sz_set_gumbel_tree(eng._e, 1, s) == N.SZ_ERR_STATE
            with pytest.raises(N.NativeError):
                eng.set_gumbel_tree(False)
            assert eng.gumbel_tree is True
        for _ in range(27):
            eng.step(*eng.evaluate(eng.planes))
        assert eng.check_errors()["boards_done"] == 3
        if meddle:
            eng.set_gumbel_tree(False)                                     # accepted: the search has ended; it holds from the next sz_search_begin on
        trees = [[eng.debug_tree(b) for b in range(3)]]
        values = [eng.debug_tree_values(b) for b in range(3)]              # still the ended search's
        eng.play([0.5] * 3)
        outs = [eng.fetch_gumbel(), eng.fetch_ply()]
        if meddle:
            eng.set_gumbel_tree(True)
        eng.search()
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(3)])
        results.append((trees, values, outs, eng.gumbel_tree_stats()))
        eng.close()
    (t0, v0, o0, n0), (t1, v1, o1, n1) = results
    assert _same(t0[0], t1[0]) and _same(t0[1], t1[1]) and n0 == n1 > 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(v0, v1)) and all(np.isfinite(v[0]) for v in v0)
    assert all(o0[i][k].tobytes() == o1[i][k].tobytes() for i in range(2) for k in o0[i])


# ------------------------------------------------------------------------------------------------ (e) Python surface
def test_play_games_takes_the_flag_from_args():
    from sigma_zero_amd.sim import play_games
    starts, max_plies, salt = [0, 17, 518, 77], [3, 2, 3, 2], 4
    gb = Gumbel(4, 50.0, 1.0)
    keys = {"C": 2, "num_searches": 32, "gumbel": {"m": 4}, "gumbel_tree": True}
    u = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    noise = lambda g, ply: -np.log(-np.log(np.random.default_rng(1000 * g + ply).random(N.SZ_MAX_MOVES)))
    stats = {}
    got = play_games(HashModel(salt=salt), keys, 4, c960=True, scharnagl=starts, uniforms=u, max_plies=max_plies, learning=True, n_boards=2,
                     gumbel_noise=noise, stats=stats)
    assert stats["gumbel_fallbacks"] == 0
    differs = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for g, (n, plies) in enumerate(zip(starts, max_plies)):
            ref = GT.Game(sz.ChessTensor(chess960=True, scharnagl=n), 32, None, reuse=False, c=2.0, learning=True, mode="dyadic", salt=salt, gumbel=gb, gumbel_tree=True)
            off = GB.Game(sz.ChessTensor(chess960=True, scharnagl=n), 32, None, reuse=False, c=2.0, learning=True, mode="dyadic", salt=salt, gumbel=gb)
            targets = []
            for ply in range(plies):
                ref.begin(None, noise(g, ply))
                ref.run()
                rec = ref.play(u(g, ply))
                targets.append(rec["policy"][:rec["n_child"]].astype(np.float64).tolist())
                if off.chosen == ref.chosen[:ply]:
                    off.begin(None, noise(g, ply))
                    off.run()
                    differs |= any(x.tobytes() != y.tobytes() for x, y in zip(off.search.tree(), ref.search.tree()))
                    off.play(u(g, ply))
            assert ref.tree_selections > 0
            assert got[g]["chosen_actions"] == ref.chosen, "game %d: moves played" % g
            assert [list(a.values()) for a in got[g]["actions"]] == targets, "game %d: the targets" % g
    assert differs                                                           # the flag reached the engine: gumbelref's trees are others
    with pytest.raises(ValueError):
        play_games(HashModel(salt=salt), {"C": 2, "num_searches": 32, "gumbel_tree": True}, 1, c960=True, scharnagl=[0], uniforms=u, max_plies=1)


def test_options_match_plays_the_tree_rule():
    """arena.play_options_match with the key on one side: Gumbel with the rule against Gumbel without it, deterministic searches"""
    from sigma_zero_amd.arena import play_options_match
    a = {"C": 2, "num_searches": 16, "gumbel": {"m": 4}, "gumbel_tree": True}
    b = {"C": 2, "num_searches": 16, "gumbel": {"m": 4}}
    runs = [play_options_match(HashModel(salt=3), a, b, 1, scharnagl=[77], sample_plies=0, max_plies=4, check_positions=True) for _ in range(2)]
    assert runs[0]["plies"] == [4, 4] and runs[0]["results"] == runs[1]["results"]
