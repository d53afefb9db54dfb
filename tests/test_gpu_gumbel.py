"""The Gumbel root search on the GPU (sz_set_gumbel / sz_fetch_gumbel / sz_gumbel_stats / sz_debug_gumbel, args["gumbel"], a NON-REFERENCE
option): the HIP engine against the plain-Python restatement tests/gumbelref.py, bit for bit — slog, sexp and the level walk on the CPU
test's inputs, root selection, sz_play's move and the improved policy on seeded child sets, whole searches tree by tree after every step with
the records, the improved policy, v_mix and the root's network value after sz_play — plus off-means-off, the refusals in both directions and
play_games.  tests/test_gumbel_ref.py proves on the CPU that the scenarios and hook cases reach the conditions they are there for; the same
counters are asserted here on the games the device was compared with."""
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


# ------------------------------------------------------------------------------------------------ 1. the device functions on seeded cases
def _debug_maths(x):
    xd = _dev(np.asarray(x, np.float64))
    a, b = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    rc = N.lib().sz_debug_gumbel(_ptr(xd), _ptr(a), _ptr(b), *([None] * 16), len(x), _stream())
    assert rc == N.SZ_OK
    torch.cuda.synchronize()
    return a.cpu().numpy(), b.cpu().numpy()


def test_device_slog_sexp_bit_equal_to_the_restatement():
    x = np.concatenate([GB.powers_of_two_f32(), GB.random_priors(3000)])
    y = GB.exp_grid(2001)
    assert len(x) + len(y) >= 5000 and (x > 0).all() and (y <= 0).all()
    got = _debug_maths(x)[0]
    want = np.array([GB.slog(v) for v in x], np.float64)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert not len(bad), "slog(%r): device %r, restatement %r (%d differ)" % (x[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    got = _debug_maths(y)[1]
    want = np.array([GB.sexp(v) for v in y], np.float64)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert not len(bad), "sexp(%r): device %r, restatement %r (%d differ)" % (y[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    assert (want[y < GB.EXP_CUTOFF] == 0.0).all() and want[y >= GB.EXP_CUTOFF].min() > 0.0


def test_device_level_walk_equals_the_phase_loop():
    tnm = GB.level_cases(70, 20)
    assert len(tnm) == 20 * sum(range(1, 71))
    td = _dev(tnm)
    out = torch.full((len(tnm),), -7, dtype=torch.int32, device="cuda")
    rc = N.lib().sz_debug_gumbel(None, None, None, _ptr(td), _ptr(out), *([None] * 14), len(tnm), _stream())
    assert rc == N.SZ_OK
    torch.cuda.synchronize()
    want = np.array([GB.level(int(t), int(n), int(m)) for t, n, m in tnm], np.int32)
    bad = np.nonzero(out.cpu().numpy() != want)[0]
    assert not len(bad), "level%r: device %d, restatement %d (%d differ)" % (tuple(tnm[bad[0]]), out[bad[0]].item(), want[bad[0]], len(bad))


def _debug_rules(hc, with_g):
    n, total = len(hc.visit), len(hc.N)
    ins = [_dev(x) for x in (hc.offsets, hc.N, hc.W, hc.P)]
    g = _dev(hc.g) if with_g else None
    tail = [_dev(x) for x in (hc.visit, hc.goal, hc.vhat)]
    opts = torch.from_numpy(np.frombuffer(hc.opts.tobytes(), np.uint8).copy()).cuda()
    assert opts.numel() == 12 * n
    sel, fbk, fin = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    pol = torch.full((total,), float("nan"), dtype=torch.float32, device="cuda")
    vmix = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    rc = N.lib().sz_debug_gumbel(None, None, None, None, None, *[_ptr(t) for t in ins], _ptr(g), *[_ptr(t) for t in tail], _ptr(opts),
                                 _ptr(sel), _ptr(fbk), _ptr(fin), _ptr(pol), _ptr(vmix), n, _stream())
    assert rc == N.SZ_OK
    torch.cuda.synchronize()
    return sel.cpu().numpy(), fbk.cpu().numpy(), fin.cpu().numpy(), pol.cpu().numpy(), vmix.cpu().numpy()


@pytest.mark.parametrize("with_g", [True, False])
def test_device_rules_on_seeded_cases(with_g):
    hc = GB.hook_cases()
    widths = np.diff(hc.offsets)
    assert len(widths) >= 500 and set(GB.HOOK_K) <= set(widths.tolist()) and widths.min() == 1 and widths.max() == 218
    sel, fbk, fin, pol, vmix, cov = GB.hook_reference(hc, with_g)
    gsel, gfbk, gfin, gpol, gvmix = _debug_rules(hc, with_g)
    print("hook cases g=%d: %d cases, %d children; %s" % (with_g, len(widths), len(hc.N), dict(cov)))
    for name, got, want in (("root selection", gsel, sel), ("fall-back", gfbk, fbk), ("sz_play's move", gfin, fin)):
        bad = np.nonzero(got != want)[0]
        assert not len(bad), "%s, case %d (K = %d): device %d, restatement %d (%d differ)" % (name, bad[0], widths[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    bad = np.nonzero(gvmix.view(np.uint64) != vmix.view(np.uint64))[0]
    assert not len(bad), "v_mix of case %d: device %r, restatement %r (%d differ)" % (bad[0], gvmix[bad[0]], vmix[bad[0]], len(bad))
    bad = np.nonzero(gpol.view(np.uint32) != pol.view(np.uint32))[0]
    assert not len(bad), "policy of flat child %d: device %r, restatement %r (%d differ)" % (bad[0], gpol[bad[0]], pol[bad[0]], len(bad))
    GB.assert_coverage(cov, [k for k in GB.HOOK_COVERAGE if not with_g or k != "tie_by_index"])


# ------------------------------------------------------------------------------------------------ 2. whole searches against the restatement
_played = {}


def _fpu_args(fp):
    return {"mode": FP.MODE_NAMES[fp.tree_mode], "value": fp.tree_value, "root_mode": FP.MODE_NAMES[fp.root_mode], "root_value": fp.root_value}


def _assert_tree(tag, eng, b, tree):
    for x, y in zip(eng.debug_tree(b), tree):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: tree differs" % tag


def _steps(eng, games, live, modes, tag, S, slot, compact):
    """the steps of one search on every live board b against games[b].search: boards pending, every network input row, the tree of every
    searching board after every step.  slot: network row of board b.  compact: shrink the batch whenever a board has finished"""
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
            _assert_tree("%s board %d after step %d" % (tag, b, t), eng, b, searches[b].step_trees[t])
        t += 1


def _drive(sc):
    B = len(sc.boards)
    args = {"C": 2, "num_searches": sc.S, "gumbel": {"m": sc.gumbel.m, "c_visit": sc.gumbel.c_visit, "c_scale": sc.gumbel.c_scale}}
    if sc.fpu is not None:
        args["fpu"] = _fpu_args(sc.fpu)
    eng = SelfPlayEngine(None, args, B, chess960=True, learning=sc.learning)
    assert eng.gumbel == tuple(GB.checked(sc.gumbel))
    games = [GB.new_game(sc, bd) for bd in sc.boards]
    modes = [(bd.mode, bd.salt) for bd in sc.boards]
    gs = GB.gumbels(sc)
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
            eng.set_gumbel(eng.gumbel, None if gs is None else gs[ply])
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
                    _assert_tree(tag(b) + " at search begin", eng, b, g.search.begin_tree)
            n_steps += _steps(eng, games, live, modes, "%s ply %d" % (sc.name, ply), sc.S, slot, sc.compact)
            st = eng.stats()
            got = tuple(st[k] for k in ("simulations", "expansions", "terminal_hits", "sum_depth"))
            assert got == tuple(sum(getattr(g, k) for g in games) for k in ("simulations", "expansions", "terminal_hits", "sum_depth")), "%s ply %d: sz_stats" % (sc.name, ply)
            assert st["boards_pending"] == 0 and st["boards_done"] == sum(live) and st["boards_error"] == errors
            assert eng.gumbel_stats() == (sum(g.gumbel_selections for g in games), 0), "%s ply %d: sz_gumbel_stats" % (sc.name, ply)
            for b, g in enumerate(games):
                if live[b]:
                    _assert_tree(tag(b) + " at search end", eng, b, g.search.tree())
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
                assert eng.debug_position(b)[0].tobytes() == GB.position_record(g.game), "%s: position record of the new root" % tag(b)
            st = eng.stats()
            assert st["boards_error"] == errors and (errors == 0 or st["first_error"] == N.SZ_ERR_ZERO_VISITS)
    eng.close()
    sims = sum(g.simulations for g in games)
    print("%s: %d plies, %d network steps, %d simulations, %d board searches compared, %d boards with nothing to play"
          % (sc.name, n_plies, n_steps, sims, sum(len(g.searches) for g in games), errors))
    assert n_plies == 3 and n_steps >= 100 and errors >= 2
    return games


@pytest.mark.parametrize("name", [sc.name for sc in GB.scenarios()])
def test_whole_searches_match_restatement(name):
    sc = next(s for s in GB.scenarios() if s.name == name)
    games = _drive(sc)
    assert all(s is not None for g in games for s in g.gumbel_plies)
    _played[name] = games


def test_whole_searches_coverage():
    """counted on the restatement, over the games the device was compared with (all of them replayed when this test runs alone)"""
    played = _played
    if len(played) < len(GB.scenarios()):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            played = {sc.name: GB.play(sc) for sc in GB.scenarios()}
    cov = GB.coverage(played.values())
    print("coverage:", {k: cov[k] for k in GB.COVERAGE})
    GB.assert_coverage(cov)


# ------------------------------------------------------------------------------------------------ 3. off means off
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


def test_off_means_off():
    base = {"C": 2, "num_searches": 32}
    used = SelfPlayEngine(HashModel(mode="rational", salt=2), dict(base, gumbel={"m": 4}), 3, chess960=True, learning=True)
    t_on, r_on = _three_plies(used)                                  # the option in use ...
    assert used.gumbel_stats()[0] > 0
    used.set_gumbel(None)                                            # ... and switched off
    assert used.gumbel is None
    got = _three_plies(used)
    used.close()
    fresh = SelfPlayEngine(HashModel(mode="rational", salt=2), base, 3, chess960=True, learning=True)
    want = _three_plies(fresh)
    with pytest.raises(N.NativeError):
        fresh.fetch_gumbel()                                         # never switched on: nothing to fetch
    fresh.close()
    for ply in range(3):
        assert _same(got[0][ply], want[0][ply]), "ply %d: trees" % ply
        assert all(got[1][ply][k].tobytes() == want[1][ply][k].tobytes() for k in want[1][ply]), "ply %d: records" % ply
    assert not _same(t_on[0], want[0][0])                            # ... while the option does build other trees from the same inputs


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_setter_rules():
    lib = N.lib()
    gopt = lambda *v: C.byref(N.sz_gumbel_options(*v))
    good = (16, 50.0, 1.0)
    eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 32}, 3, chess960=True, learning=True)
    s = eng._stream()
    for bad in ((0, 50.0, 1.0), (-3, 50.0, 1.0), (219, 50.0, 1.0), (16, float("nan"), 1.0), (16, float("inf"), 1.0), (16, -1.0, 1.0),
                (16, 50.0, float("nan")), (16, 50.0, -float("inf")), (16, 50.0, -0.5)):
        assert lib.sz_set_gumbel(eng._e, gopt(*bad), None, s) == N.SZ_ERR_INVALID, bad
    assert lib.sz_set_gumbel(None, None, None, s) == N.SZ_ERR_INVALID
    assert lib.sz_fetch_gumbel(eng._e, None, None, None, s) == N.SZ_ERR_STATE
    # the other option is on first: Gumbel is refused, and accepted once it is off again
    ending = N.sz_ending_options(-0.9, 3, 0, 0.0, 0, 0, 0)
    sopt = lambda L, solver: C.byref(N.sz_search_options(L, 1.0, solver))
    gamma = torch.ones(3, N.SZ_MAX_MOVES, dtype=torch.float32, device="cuda")
    others = [(lambda: lib.sz_set_leaf_batching(eng._e, 2, 1.0, s), lambda: lib.sz_set_leaf_batching(eng._e, 1, 1.0, s), N.SZ_ERR_INVALID),
              (lambda: lib.sz_set_solver(eng._e, 1, s), lambda: lib.sz_set_solver(eng._e, 0, s), N.SZ_ERR_INVALID),
              (lambda: lib.sz_set_search_options(eng._e, sopt(4, 0), s), lambda: lib.sz_set_search_options(eng._e, sopt(1, 0), s), N.SZ_ERR_INVALID),
              (lambda: lib.sz_set_search_options(eng._e, sopt(1, 1), s), lambda: lib.sz_set_search_options(eng._e, sopt(1, 0), s), N.SZ_ERR_INVALID),
              (lambda: lib.sz_set_forced_playouts(eng._e, 2.0, None, s), lambda: lib.sz_set_forced_playouts(eng._e, 0.0, None, s), N.SZ_ERR_INVALID),
              (lambda: lib.sz_set_endings(eng._e, C.byref(ending), None, s), lambda: lib.sz_set_endings(eng._e, None, None, s), N.SZ_ERR_INVALID),
              (lambda: lib.sz_set_root_noise(eng._e, _ptr(gamma)), lambda: lib.sz_set_root_noise(eng._e, None), N.SZ_ERR_STATE),
              (lambda: lib.sz_set_search_root_noise(eng._e, _ptr(gamma), None, s), lambda: lib.sz_set_search_root_noise(eng._e, None, None, s), N.SZ_ERR_STATE)]
    for on, off, code in others:
        assert on() == N.SZ_OK
        assert lib.sz_set_gumbel(eng._e, gopt(*good), None, s) == code
        assert lib.sz_set_gumbel(eng._e, None, None, s) == N.SZ_OK                 # switching off is always accepted
        assert off() == N.SZ_OK
    # Gumbel is on first: every one of them is refused, switching them off is not
    assert lib.sz_set_gumbel(eng._e, gopt(*good), None, s) == N.SZ_OK
    for on, off, code in others:
        assert on() == code
        assert off() == N.SZ_OK
    assert lib.sz_set_fpu(eng._e, C.byref(N.sz_fpu_options(FP.REDUCTION, 0.33, FP.ABSOLUTE, 1.0)), s) == N.SZ_OK      # works with FPU
    assert lib.sz_set_fpu(eng._e, None, s) == N.SZ_OK
    eng.close()
    reuse = SelfPlayEngine(HashModel(), {"C": 2, "num_searches": 16, "reuse_subtree": True}, 1, chess960=True, learning=True)
    assert lib.sz_set_gumbel(reuse._e, gopt(*good), None, reuse._stream()) == N.SZ_ERR_INVALID
    assert lib.sz_set_gumbel(reuse._e, None, None, reuse._stream()) == N.SZ_OK
    reuse.close()
    # during a search: refused, nothing changes; a refused call leaves nothing behind for the next sz_search_begin either
    results = []
    for meddle in (False, True):
        eng = SelfPlayEngine(HashModel(mode="rational", salt=2), {"C": 2, "num_searches": 32, "gumbel": {"m": 4}}, 3, chess960=True, learning=False)
        s = eng._stream()
        eng.new_games(STARTS)
        eng.begin()
        for _ in range(5):
            eng.step(*eng.evaluate(eng.planes))
        if meddle:
            assert lib.sz_set_gumbel(eng._e, None, None, s) == N.SZ_ERR_STATE
            assert lib.sz_set_gumbel(eng._e, gopt(1, 0.0, 9.0), None, s) == N.SZ_ERR_STATE
            with pytest.raises(N.NativeError):
                eng.set_gumbel((2, 1.0, 1.0))
            assert eng.gumbel == (4, 50.0, 1.0)
            assert lib.sz_set_gumbel(eng._e, gopt(0, 50.0, 1.0), None, s) == N.SZ_ERR_INVALID
        for _ in range(27):
            eng.step(*eng.evaluate(eng.planes))
        assert eng.check_errors()["boards_done"] == 3
        trees = [[eng.debug_tree(b) for b in range(3)]]
        eng.play([0.5] * 3)
        out = [eng.fetch_gumbel()]
        eng.search()
        eng.check_errors()
        trees.append([eng.debug_tree(b) for b in range(3)])
        results.append((trees, out))
        eng.close()
    (t0, o0), (t1, o1) = results
    assert _same(t0[0], t1[0]) and _same(t0[1], t1[1]) and all(o0[0][k].tobytes() == o1[0][k].tobytes() for k in o0[0])
    with pytest.raises(ValueError):
        SelfPlayEngine(None, {"C": 2, "num_searches": 8, "gumbel": {"m": 0}}, 1)


# ------------------------------------------------------------------------------------------------ 5. Python surface
def test_play_games_takes_the_option_from_args():
    from sigma_zero_amd.sim import play_games
    starts, max_plies, salt = [0, 17, 518, 77], [3, 2, 3, 2], 4
    gb = Gumbel(4, 50.0, 1.0)
    keys = {"C": 2, "num_searches": 32, "gumbel": {"m": 4}}
    u = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
    noise = lambda g, ply: -np.log(-np.log(np.random.default_rng(1000 * g + ply).random(N.SZ_MAX_MOVES)))
    stats = {}
    got = play_games(HashModel(salt=salt), keys, 4, c960=True, scharnagl=starts, uniforms=u, max_plies=max_plies, learning=True, n_boards=2,
                     gumbel_noise=noise, stats=stats)
    off = play_games(HashModel(salt=salt), {"C": 2, "num_searches": 32}, 4, c960=True, scharnagl=starts, uniforms=u, max_plies=max_plies, learning=True,
                     n_boards=2)
    assert stats["gumbel_fallbacks"] == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for g, (n, plies) in enumerate(zip(starts, max_plies)):
            for games, option in ((got, gb), (off, None)):
                ref = GB.Game(sz.ChessTensor(chess960=True, scharnagl=n), 32, None, reuse=False, c=2.0, learning=True, mode="dyadic", salt=salt, gumbel=option)
                targets = []
                for ply in range(plies):
                    ref.begin(None, noise(g, ply) if option is not None else None)
                    ref.run()
                    rec = ref.play(u(g, ply))
                    k = rec["n_child"]
                    vis = rec["visits"][:k].astype(np.int64)
                    targets.append(rec["policy"][:k].astype(np.float64).tolist() if option is not None else (vis / int(vis.sum())).tolist())
                assert games[g]["chosen_actions"] == ref.chosen, "game %d (option %r): moves played" % (g, option)
                assert [list(a.values()) for a in games[g]["actions"]] == targets, "game %d (option %r): the targets" % (g, option)
                assert all(type(x) is float for a in games[g]["actions"] for x in a.values())
    assert set(got[0]) == set(off[0]) and set(stats) - {"gumbel_fallbacks"} == {
        "sims", "nn_rows", "plies", "full_plies", "fast_plies", "searches_without_network", "forced_selections", "pruned_visits", "resigned", "adjudicated_draws",
        "adjudicated_proven", "holdout_games", "holdout_marks", "host_seconds"}
    assert any([list(a.values()) for a in got[g]["actions"]] != [list(a.values()) for a in off[g]["actions"]] for g in range(4))


def test_options_match_plays_a_gumbel_configuration():
    """arena.play_options_match with "gumbel" on one side: a learning=False engine with g = NULL, a deterministic search"""
    from sigma_zero_amd.arena import play_options_match
    runs = [play_options_match(HashModel(salt=3), {"C": 2, "num_searches": 16, "gumbel": {"m": 4}}, {"C": 2, "num_searches": 16}, 1, scharnagl=[77],
                               sample_plies=0, max_plies=4, check_positions=True) for _ in range(2)]
    assert runs[0]["plies"] == [4, 4] and runs[0]["results"] == runs[1]["results"]
