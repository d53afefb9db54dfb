"""include/sigmazero.h: "all device work is enqueued on the caller's stream".  Every family of entry points behind the gate of tests/streamgate.py, on
a non-default, non-blocking stream: a delay kernel holds the stream, the region's device inputs hold poison until a copy BEHIND the delay brings the true
ones, the region is issued, its outputs are snapshot on the same stream, and everything the region wrote or returned is held to a default-stream run of the
same program on a fresh engine, torch.equal on raw bits.  A launch, copy or fill that went to another stream reads poison; a host read that waited for
another stream returns what was there before the region ran.  For regions that do not block the host the gate is SEEN holding (the delay's event is still
pending once the region and its snapshots are issued), else the test fails as inconclusive.  The teeth tests issue one region per family on the default
stream on purpose and require the comparison to see it.

All engine runs replay evaluations made on the host from a seeded generator (no host round trip inside a region): probability rows and values, poison =
the true batch rolled by one board.  8 boards, 12 searches, Chess960 starts, 3 plies unless noted.  Every region is gated (about 10 ms each); no family
needed the every-third-step relief, so the gate has none.  Two streams with work in flight at once are out of scope (the pacing counters and trainconv._scratch are documented
as one stream at a time), and so is the "makes that device current" half of the header's sentence, which needs a second GPU."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
import streamgate as G
import fullref as FU
import gumbelref as GB
import puctref as PR

pytestmark = pytest.mark.gpu

B, S, PLIES = 8, 12, 3
STARTS = (0, 959, 518, 400, 77, 5, 811, 333)
LAYOUTS = {"f32": torch.float32, "bf16": torch.bfloat16, "nhwc128": "nhwc128", "bits128": "bits128"}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """the module keeps networks, staging rows and side-stream allocator pools alive while it runs; the tests behind it in the same process get the device
    as they would without it"""
    yield
    for cached in (_rows, _net, _module):
        cached.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _h(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ctx(sess):
    """what is not a region (building the engine) runs on the session's stream too"""
    return torch.cuda.stream(sess.stream) if sess.gated else contextlib.nullcontext()


def _engine(sess, args, n=B, **kw):
    with _ctx(sess):
        eng = SelfPlayEngine(None, args, n, chess960=True, learning=True, **kw)
    torch.cuda.synchronize()
    return eng


@functools.lru_cache(maxsize=None)
def _rows(key, n):
    """(policy pool [n+1,4672] f32, value pool [n+1] f32) on the device for one search step: staging tensors, filled once and left unchanged"""
    p, v = G.policy_pool(n + 1, np.random.default_rng([11] + list(key)))
    out = _dev(p), _dev(v)
    torch.cuda.synchronize()
    return out


def _eval_inputs(bufs, key, n):
    (pp, vp), (pb, vb) = _rows(key, n), bufs
    pt, ppo = G.shifted(pp, n)
    vt, vpo = G.shifted(vp, n)
    return [(pb, pt, ppo), (vb, vt, vpo)]


def _check(rc, what):
    assert rc == N.SZ_OK, "%s returned %d" % (what, rc)
    return rc


def _judge(family, base, gated):
    """a gated pass: every region equal to the baseline, every gate of a non-blocking region seen holding, the figures written down"""
    G.write_report(family, gated)
    assert len(gated) == len(base), "%s: %d regions gated, %d in the baseline" % (family, len(gated), len(base))
    bad = G.compare(base, gated)
    assert not bad, "%s: off the caller's stream, or read before the stream was waited for: %s" % (family, bad[:6])
    n = G.assert_held(gated)
    print("%s: %d regions bit-equal to the default-stream baseline, %d gates seen holding, %d blocking regions judged by their values"
          % (family, len(gated), n, len(gated) - n))
    return n


def _bite(family, base, gated, region):
    """a misrouted pass: the comparison must see it, in a device output or a host value"""
    assert any(r.misrouted for r in gated), "%s: region %s was never issued" % (family, region)
    G.assert_held([r for r in gated if not r.misrouted])
    bad = G.compare(base, gated)
    print("%s, %s issued on the default stream: %s" % (family, region, bad[:4]))
    assert bad, "%s: %s ran on the default stream behind the gate's back and nothing differs from the baseline: the gate has no teeth here" % (family, region)


# ---------------------------------------------------------------------------------------------------------------- shared pieces of the programs
def _stats(eng):
    return tuple(sorted(eng.stats().items()))


def _trees(eng, proven=False):
    out = [eng.debug_tree(b) for b in range(eng.B)]
    if proven:
        out += [eng.debug_tree_proven(b) for b in range(eng.B)]
    return out


def _root_children(sess, eng, tag):
    lib, e = N.lib(), eng._e
    outs = [eng.root_action, eng.root_visits, eng.root_nchild, eng.root_prior, eng.root_wsum]
    sess.region("root_children#%s" % tag, lambda: _check(lib.sz_root_children(e, *[_p(t) for t in outs], _st()), "sz_root_children"), outputs=outs)


def _search(sess, eng, bufs, ply, extra=(), first_extra=(), n_steps=S, k0=0, begin=True, rows=None):
    """sz_search_begin and the steps of one search, one region each; with leaf batching sz_pending_boards after every step decides when it is over.
    extra: gated inputs of every region (device arrays a setter handed over and the kernels read later); first_extra: of begin and the first step;
    rows: network rows evaluated (default: every board's), the size of bufs"""
    lib, e, rows = N.lib(), eng._e, eng.B * eng.L if rows is None else rows
    assert bufs[0].shape[0] == rows
    if begin:
        sess.region("begin#%d" % ply, lambda: _check(lib.sz_search_begin(e, _p(eng.planes), _st()), "sz_search_begin"),
                    inputs=list(extra) + list(first_extra), outputs=[eng.planes])
    for k in range(k0, k0 + n_steps):
        ins = _eval_inputs(bufs, (ply, k), rows) + list(extra) + (list(first_extra) if k == 0 else [])
        sess.region("step#%d/%d" % (ply, k), lambda: _check(lib.sz_search_step(e, _p(bufs[0]), _p(bufs[1]), _p(eng.planes), _st()), "sz_search_step"),
                    inputs=ins, outputs=[eng.planes])
        if eng.L > 1 and sess.region("pending#%d/%d" % (ply, k), eng.pending_boards, blocking=True) == 0:
            break


def _eval_bufs(eng, rows=None):
    rows = eng.B * eng.L if rows is None else rows
    return torch.zeros(rows, N.SZ_ACTIONS, device="cuda"), torch.zeros(rows, device="cuda")


def _play(sess, eng, ply, extra=()):
    lib, e = N.lib(), eng._e
    u = G.gate_uniforms(eng.B, np.random.default_rng([12, ply]))
    ut, up = _dev(u), _dev(G.poison_uniforms(u))
    sess.region("play#%d" % ply, lambda: _check(lib.sz_play(e, _p(eng.uniforms), _st()), "sz_play"), inputs=[(eng.uniforms, ut, up)] + list(extra))
    return sess.region("fetch_ply#%d" % ply, eng.fetch_ply, blocking=True)


# ---------------------------------------------------------------------------------------------------------------- engine core
def _core_program(layout, reuse):
    data = {}

    def program(sess):
        args = {"C": 2, "num_searches": S}
        if reuse:
            args["reuse_subtree"] = True
        eng = _engine(sess, args, planes_dtype=LAYOUTS[layout])
        lib, e = N.lib(), eng._e
        bufs, moves = _eval_bufs(eng), torch.zeros(B, dtype=torch.int32, device="cuda")
        sch = np.array(STARTS, np.int32)
        sess.region("new_games", lambda: _check(lib.sz_new_games(e, _h(sch), None, _st()), "sz_new_games"), blocking=True)
        sch2, mask = np.array([(3 * n + 7) % 960 for n in STARTS], np.int32), np.array([0, 1, 0, 0, 1, 0, 0, 0], np.uint8)
        sess.region("new_games_masked", lambda: _check(lib.sz_new_games(e, _h(sch2), _h(mask), _st()), "sz_new_games"), blocking=True)
        up = sz.ChessTensor(chess960=True, scharnagl=100)
        for k in range(2):
            up.push_action(sorted(up.legal_action_indices())[3 + k])
        ring, ply0, _ = up.export_ring()
        sess.region("upload_game", lambda: _check(lib.sz_upload_game(e, 7, ring, int(ply0), _st()), "sz_upload_game"), blocking=True)
        mirror = [sz.ChessTensor(chess960=True, scharnagl=int(sch2[b] if mask[b] else sch[b])) for b in range(B - 1)] + [up]
        for ply in range(PLIES):
            _search(sess, eng, bufs, ply)
            _root_children(sess, eng, ply)
            st = dict(sess.region("stats#%d" % ply, lambda: _stats(eng), blocking=True))
            assert st["boards_error"] == 0 and st["simulations"] > 0
            sess.region("debug_tree#%d" % ply, lambda: _trees(eng), blocking=True)
            rec = _play(sess, eng, ply)
            if reuse:
                sess.region("debug_tree_kept#%d" % ply, lambda: _trees(eng), blocking=True)
            if ("moves", ply) not in data:                              # the baseline pass records the given moves: two legal moves of the position reached
                assert not sess.gated
                for b in range(B):
                    if rec["active"][b] and rec["chosen"][b] >= 0:
                        mirror[b].push_action(int(rec["chosen"][b]))
                legal = [[] if rec["game_over"][b] else mirror[b].legal_action_indices() for b in range(B)]
                data["moves", ply] = G.gate_actions(legal, np.random.default_rng([13, ply]))
                for b, a in enumerate(data["moves", ply][0]):
                    if a >= 0:
                        mirror[b].push_action(int(a))
            true, poison = data["moves", ply]
            assert (true != poison).sum() >= B - 1
            sess.region("play_moves#%d" % ply, lambda: _check(lib.sz_play_moves(e, _p(moves), _st()), "sz_play_moves"), inputs=[(moves, _dev(true), _dev(poison))])
            rec = sess.region("fetch_moves#%d" % ply, eng.fetch_ply, blocking=True)
            assert rec["chosen"].tolist() == true.tolist()
        st = dict(sess.region("stats#end", lambda: _stats(eng), blocking=True))
        assert st["boards_error"] == 0
        eng.close()

    return program


@pytest.mark.parametrize("reuse", [False, True], ids=["plain", "reuse_subtree"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_engine_core_stays_on_the_callers_stream(layout, reuse):
    base, gated = G.run_pair(_core_program(layout, reuse))
    n = _judge("engine core %s %s" % (layout, "reuse" if reuse else "plain"), base, gated)
    assert n >= PLIES * (S + 4)


# ---------------------------------------------------------------------------------------------------------------- ragged batch
def _ragged_program(sess):
    eng = _engine(sess, {"C": 2, "num_searches": S})
    lib, e = N.lib(), eng._e
    sch = np.array(STARTS, np.int32)
    sess.region("new_games", lambda: _check(lib.sz_new_games(e, _h(sch), None, _st()), "sz_new_games"), blocking=True)
    budgets = np.array([S, 4, S, S, 4, S, S, 4], np.int32)              # three boards end eight steps early
    sess.region("set_search_budgets", lambda: _check(lib.sz_set_search_budgets(e, budgets.ctypes.data_as(C.POINTER(C.c_int32)), _st()), "sz_set_search_budgets"), blocking=True)
    active = np.array([1, 1, 0, 1, 1, 0, 1, 1], np.uint8)

    def compact():
        _check(lib.sz_set_active(e, _h(active), _st()), "sz_set_active")
        n = C.c_int32(-1)
        _check(lib.sz_compact(e, 1, C.byref(n), _st()), "sz_compact")
        return int(n.value)

    n_live = sess.region("set_active+compact", compact, blocking=True)
    assert n_live == 6
    bufs = _eval_bufs(eng, n_live)                                      # the network runs on n_live rows from here on: policy and value have no more
    _search(sess, eng, bufs, 0, n_steps=0, rows=n_live)
    goals = sess.region("search_goals", eng.search_goals, blocking=True)
    assert goals.tolist() == [S, 4, 0, S, 4, 0, S, 4]
    _search(sess, eng, bufs, 0, n_steps=4, begin=False, rows=n_live)
    assert sess.region("pending_boards#4", eng.pending_boards, blocking=True) == 3

    def shrink():
        n = C.c_int32(-1)
        _check(lib.sz_compact_searching(e, _p(eng.planes), C.byref(n), _st()), "sz_compact_searching")
        return int(n.value)

    before = eng.planes.clone()
    n_live = sess.region("compact_searching", shrink, outputs=[eng.planes], blocking=True)
    assert n_live == 3
    bufs = _eval_bufs(eng, n_live)                                      # ... and on three rows behind the shrink
    assert not torch.equal(before[:3], eng.planes[:3]), "the pending rows of the boards that still search moved down"
    _search(sess, eng, bufs, 0, n_steps=S - 4, k0=4, begin=False, rows=n_live)
    assert sess.region("pending_boards#end", eng.pending_boards, blocking=True) == 0
    st = dict(sess.region("stats", lambda: _stats(eng), blocking=True))
    assert st["boards_error"] == 0 and st["simulations"] > 0
    _root_children(sess, eng, "end")
    sess.region("debug_tree", lambda: _trees(eng), blocking=True)
    eng.close()


def test_ragged_batch_stays_on_the_callers_stream():
    base, gated = G.run_pair(_ragged_program)
    _judge("ragged batch", base, gated)


# ---------------------------------------------------------------------------------------------------------------- options whose device arrays are read later
def _pool(shape_tail, key, make):
    pool = _dev(make(np.random.default_rng([14] + list(key)), (B + 1,) + shape_tail))
    return G.shifted(pool, B)


def _full_program(sess):
    """the option set of tests/test_gpu_full_config.py (FU.args_of: subtree reuse with visit targets and root noise, quiet plies, forced playouts, first-play
    urgency, the ending rules), leaf batching L = 4 and the solver switched on through sz_set_search_options under the gate"""
    cfg = FU.play_config()
    args = dict(FU.args_of(cfg, 1, False), num_searches=S, playout_cap={"fast": 4, "p_full": 0.5})
    eng = _engine(sess, args)
    lib, e = N.lib(), eng._e
    sess.region("set_search_options", lambda: eng.set_search_options(4, 1.0, True), blocking=True)
    assert eng.L == 4 and eng.planes.shape[0] == 4 * B
    bufs, gamma = _eval_bufs(eng), torch.zeros(B, N.SZ_MAX_MOVES, device="cuda")
    sch = np.array(cfg.starts, np.int32)
    sess.region("new_games", lambda: _check(lib.sz_new_games(e, _h(sch), None, _st()), "sz_new_games"), blocking=True)
    end = N.sz_ending_options(*[args["endings"][k] for k in ("resign_value", "resign_patience", "resign_min_ply", "draw_value", "draw_patience", "draw_min_ply")], 0)
    for ply in range(PLIES):
        targets = np.array([S if (b + ply) % 2 == 0 else 4 for b in range(B)], np.int32)
        quiet = np.array([(b + ply) % 3 == 0 for b in range(B)], np.uint8)
        forced = np.array([(b + ply) % 4 != 1 for b in range(B)], np.uint8)
        holdout = np.array([b in (2, 5) for b in range(B)], np.uint8)
        sess.region("set_visit_targets#%d" % ply, lambda: _check(lib.sz_set_visit_targets(e, targets.ctypes.data_as(C.POINTER(C.c_int32)), _st()), "sz_set_visit_targets"), blocking=True)
        # the setter returns at once with the POISONED array's address; sz_search_begin (kept roots) and the step behind it (fresh roots) read it
        sess.region("set_search_root_noise#%d" % ply, lambda: _check(lib.sz_set_search_root_noise(e, _p(gamma), _h(quiet), _st()), "sz_set_search_root_noise"), blocking=True)
        sess.region("set_forced_playouts#%d" % ply, lambda: _check(lib.sz_set_forced_playouts(e, float(cfg.forced_k), _h(forced), _st()), "sz_set_forced_playouts"), blocking=True)
        sess.region("set_endings#%d" % ply, lambda: _check(lib.sz_set_endings(e, C.byref(end), _h(holdout), _st()), "sz_set_endings"), blocking=True)
        gt, gp = _pool((N.SZ_MAX_MOVES,), (0, ply), lambda rng, shape: (rng.standard_gamma(0.3, size=shape) + 1e-6).astype(np.float32))
        _search(sess, eng, bufs, ply, first_extra=[(gamma, gt, gp)])
        st = dict(sess.region("stats#%d" % ply, lambda: _stats(eng), blocking=True))
        assert st["boards_error"] == 0
        sess.region("solver_stats#%d" % ply, eng.solver_stats, blocking=True)
        sess.region("forced_stats#%d" % ply, eng.forced_stats, blocking=True)
        _root_children(sess, eng, ply)
        root, child = torch.zeros(B, dtype=torch.int8, device="cuda"), torch.zeros(B, N.SZ_MAX_MOVES, dtype=torch.int8, device="cuda")
        sess.region("root_proven#%d" % ply, lambda: _check(lib.sz_root_proven(e, _p(root), _p(child), _st()), "sz_root_proven"), outputs=[root, child])
        sess.region("debug_tree#%d" % ply, lambda: _trees(eng, proven=True), blocking=True)
        _play(sess, eng, ply)
        sess.region("fetch_endings#%d" % ply, eng.fetch_endings, blocking=True)
        sess.region("ending_stats#%d" % ply, eng.ending_stats, blocking=True)
        sess.region("forced_stats_after_play#%d" % ply, eng.forced_stats, blocking=True)
    assert st["simulations"] > 0
    eng.close()


def _gumbel_program(sess):
    """the option set of tests/test_gpu_gumbel.py's seeded scenario (Gumbel(16, 50, 1)); the draws g_dev are read by every step's root selection and by sz_play"""
    sc = GB.scenarios()[0]
    opts = (sc.gumbel.m, sc.gumbel.c_visit, sc.gumbel.c_scale)
    eng = _engine(sess, {"C": 2, "num_searches": S, "gumbel": {"m": opts[0], "c_visit": opts[1], "c_scale": opts[2]}})
    lib, e = N.lib(), eng._e
    bufs, g = _eval_bufs(eng), torch.zeros(B, N.SZ_MAX_MOVES, dtype=torch.float64, device="cuda")
    sch = np.array(STARTS, np.int32)
    sess.region("new_games", lambda: _check(lib.sz_new_games(e, _h(sch), None, _st()), "sz_new_games"), blocking=True)
    o = N.sz_gumbel_options(int(opts[0]), float(opts[1]), float(opts[2]))
    for ply in range(PLIES):
        sess.region("set_gumbel#%d" % ply, lambda: _check(lib.sz_set_gumbel(e, C.byref(o), _p(g), _st()), "sz_set_gumbel"), blocking=True)
        if ply == 1:
            sess.region("set_gumbel_tree", lambda: _check(lib.sz_set_gumbel_tree(e, 1, _st()), "sz_set_gumbel_tree"), blocking=True)
        draws = [(g,) + _pool((N.SZ_MAX_MOVES,), (1, ply), lambda rng, shape: -np.log(-np.log(rng.random(size=shape))))]
        _search(sess, eng, bufs, ply, extra=draws)
        st = dict(sess.region("stats#%d" % ply, lambda: _stats(eng), blocking=True))
        assert st["boards_error"] == 0
        sess.region("gumbel_stats#%d" % ply, eng.gumbel_stats, blocking=True)
        sess.region("gumbel_tree_stats#%d" % ply, eng.gumbel_tree_stats, blocking=True)
        sess.region("debug_tree#%d" % ply, lambda: _trees(eng), blocking=True)
        _play(sess, eng, ply, extra=draws)
        sess.region("fetch_gumbel#%d" % ply, eng.fetch_gumbel, blocking=True)
    assert eng.gumbel_stats()[0] > 0
    eng.close()


def _temperature_program(sess):
    """move-selection temperature (temps_dev is read by sz_play), the visit-dependent exploration rate (the settings of tests/puctref.py's configurations)
    and the solver switched on through its own setter, sz_set_solver (in _full_program sz_set_search_options switches it on)"""
    eng = _engine(sess, {"C": 2, "num_searches": S})
    lib, e = N.lib(), eng._e
    bufs, temps = _eval_bufs(eng), torch.ones(B, dtype=torch.float64, device="cuda")
    sch = np.array(STARTS, np.int32)
    sess.region("new_games", lambda: _check(lib.sz_new_games(e, _h(sch), None, _st()), "sz_new_games"), blocking=True)
    cp = N.sz_cpuct_options(*[float(x) for x in PR.A])
    sess.region("set_cpuct", lambda: _check(lib.sz_set_cpuct(e, C.byref(cp), _st()), "sz_set_cpuct"), blocking=True)
    sess.region("set_solver", lambda: _check(lib.sz_set_solver(e, 1, _st()), "sz_set_solver"), blocking=True)
    root, child = torch.zeros(B, dtype=torch.int8, device="cuda"), torch.zeros(B, N.SZ_MAX_MOVES, dtype=torch.int8, device="cuda")
    values = np.array([0.5, 1.0, 0.25, 2.0, 0.75, 1.5, 0.0, 1.25, 3.0])
    for ply, (offset, cutoff) in enumerate([(0.0, None), (-0.8, 0.1), (2.0, 0.0)]):
        o = N.sz_temperature_options(float(offset), 0.0 if cutoff is None else float(cutoff), int(cutoff is not None))
        sess.region("set_move_temperature#%d" % ply, lambda: _check(lib.sz_set_move_temperature(e, C.byref(o), _p(temps), _st()), "sz_set_move_temperature"), blocking=True)
        _search(sess, eng, bufs, ply)
        st = dict(sess.region("stats#%d" % ply, lambda: _stats(eng), blocking=True))
        assert st["boards_error"] == 0
        sess.region("solver_stats#%d" % ply, eng.solver_stats, blocking=True)
        sess.region("root_proven#%d" % ply, lambda: _check(lib.sz_root_proven(e, _p(root), _p(child), _st()), "sz_root_proven"), outputs=[root, child])
        pool = _dev(np.roll(values, ply))
        _play(sess, eng, ply, extra=[(temps,) + G.shifted(pool, B)])
        sess.region("fetch_temperature#%d" % ply, eng.fetch_temperature, blocking=True)
        sess.region("temperature_stats#%d" % ply, eng.temperature_stats, blocking=True)
    assert eng.temperature_stats()[0] > 0
    eng.close()


OPTION_PROGRAMS = {"full_config": _full_program, "gumbel": _gumbel_program, "temperature_cpuct_solver": _temperature_program}


@pytest.mark.parametrize("name", list(OPTION_PROGRAMS))
def test_option_arrays_read_later_stay_on_the_callers_stream(name):
    base, gated = G.run_pair(OPTION_PROGRAMS[name])
    _judge("options %s" % name, base, gated)


# ---------------------------------------------------------------------------------------------------------------- setters that refuse inside a search
def _setters(e, _st=_st):
    """every setter that is valid only between searches, with the argument that switches its option off: accepted in every engine state, so that
    SZ_ERR_STATE can only come from the question whether the engine searches, which is answered from the stream"""
    lib, one = N.lib(), N.sz_search_options(1, 1.0, 0)
    return [("sz_set_search_budgets", lambda: lib.sz_set_search_budgets(e, None, _st())),
            ("sz_set_visit_targets", lambda: lib.sz_set_visit_targets(e, None, _st())),
            ("sz_set_search_root_noise", lambda: lib.sz_set_search_root_noise(e, None, None, _st())),
            ("sz_set_leaf_batching", lambda: lib.sz_set_leaf_batching(e, 1, 1.0, _st())),
            ("sz_set_solver", lambda: lib.sz_set_solver(e, 0, _st())),
            ("sz_set_search_options", lambda: lib.sz_set_search_options(e, C.byref(one), _st())),
            ("sz_set_forced_playouts", lambda: lib.sz_set_forced_playouts(e, 0.0, None, _st())),
            ("sz_set_fpu", lambda: lib.sz_set_fpu(e, None, _st())),
            ("sz_set_cpuct", lambda: lib.sz_set_cpuct(e, None, _st())),
            ("sz_set_gumbel", lambda: lib.sz_set_gumbel(e, None, None, _st())),
            ("sz_set_gumbel_tree", lambda: lib.sz_set_gumbel_tree(e, 0, _st())),
            ("sz_set_endings", lambda: lib.sz_set_endings(e, None, None, _st())),
            ("sz_set_move_temperature", lambda: lib.sz_set_move_temperature(e, None, None, _st()))]


def _default_st():
    return C.c_void_p(torch.cuda.default_stream().cuda_stream)


def _refusal_program(sess, wrong_stream=False):
    """wrong_stream (the teeth): on the gated pass the setters are handed the default stream, while sz_search_begin goes to S"""
    eng = _engine(sess, {"C": 2, "num_searches": S})
    lib, e = N.lib(), eng._e
    bufs = _eval_bufs(eng)
    sch = np.array(STARTS, np.int32)
    sess.region("new_games", lambda: _check(lib.sz_new_games(e, _h(sch), None, _st()), "sz_new_games"), blocking=True)
    wrong = wrong_stream and sess.gated
    setters = _setters(e, _default_st) if wrong else _setters(e)
    # a setter that waited for another stream sees the engine as it was BEFORE the call issued in front of it: between searches here ...
    got = sess.region("begin+setters", lambda: [_check(lib.sz_search_begin(e, _p(eng.planes), _st()), "sz_search_begin")] + [f() for _, f in setters], blocking=True)
    if wrong_stream:
        eng.close()
        return
    assert got[1:] == [N.SZ_ERR_STATE] * len(setters), "inside a search: %s" % dict(zip([n for n, _ in setters], got[1:]))
    for k in range(S):
        step = lambda: _check(lib.sz_search_step(e, _p(bufs[0]), _p(bufs[1]), _p(eng.planes), _st()), "sz_search_step")
        if k in (0, 5, S - 1):
            got = sess.region("step+setters#%d" % k, lambda: [step()] + [f() for _, f in setters], inputs=_eval_inputs(bufs, (0, k), B), outputs=[eng.planes], blocking=True)
            # ... and still searching behind the search's last step
            want = N.SZ_OK if k == S - 1 else N.SZ_ERR_STATE
            assert got[1:] == [want] * len(setters), "step %d of %d: %s" % (k, S, dict(zip([n for n, _ in setters], got[1:])))
        else:
            sess.region("step#0/%d" % k, step, inputs=_eval_inputs(bufs, (0, k), B), outputs=[eng.planes])
    sess.region("debug_tree", lambda: _trees(eng), blocking=True)
    eng.close()


def test_setters_answer_from_the_callers_stream():
    base, gated = G.run_pair(_refusal_program)
    _judge("refusing setters", base, gated)


# ---------------------------------------------------------------------------------------------------------------- inference networks
# every form the networks have.  The per-block kernels and the separate heads exist for bf16 operands only: FastPolicyNet(operands="fp16") raises ValueError
# ("fp16 operands need the persistent tower" / "... the fused heads") when either is switched off, so fp16 runs in its one form, persistent tower + fused heads
NETS = ["fast_bf16", "fast_bf16_blocks", "fast_bf16_separate_heads", "fast_fp16", "split_bf16", "split_fp16"]


@functools.lru_cache(maxsize=None)
def _module():
    torch.manual_seed(0)
    return sz.policyNN({}).cuda().eval()


@functools.lru_cache(maxsize=None)
def _net(kind):
    from sigma_zero_amd.fastnet import FastPolicyNet, SplitPolicyNet
    if kind.startswith("split"):
        return SplitPolicyNet(_module(), operands=kind[6:])
    net = FastPolicyNet(_module(), operands="fp16" if kind == "fast_fp16" else "bf16")
    if kind == "fast_bf16_blocks":
        net.persistent_tower = False
    if kind == "fast_bf16_separate_heads":
        net.fused_heads = False
    return net


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _net_program(net, true, poison, want_overflow):
    """a network is stateless but for its buffers and its range flag: the same object serves both passes, the flag is read (and so cleared) first"""
    def program(sess):
        buf = torch.empty_like(true)
        out = {}

        def forward(inference):
            out["pv"] = net(buf, inference=inference)

        with _ctx(sess):                                                # first use on this stream: buffers, function attributes, the pacing counters
            buf.copy_(poison)
            forward(True)
            net.overflowed()
        torch.cuda.synchronize()
        sess.region("forward_inference", lambda: forward(True), inputs=[(buf, true, poison)], outputs=lambda _: out["pv"])

        def logits_and_flag():
            forward(False)
            return bool(net.overflowed())                               # reads the device word the forward just wrote: it must wait for THAT forward

        assert sess.region("forward_logits+overflowed", logits_and_flag, inputs=[(buf, true, poison)], outputs=lambda _: out["pv"], blocking=True) == want_overflow

    return program


def _planes(n, layout, seed):
    img = G.nhwc128(G.random_planes(n + 1, np.random.default_rng([15, seed])))
    pool = _dev(G.pack_bits128(img)) if layout == "bits128" else _dev(img).to(torch.bfloat16)
    return G.shifted(pool, n)


@pytest.mark.parametrize("layout", ["bits128", "nhwc128"])
@pytest.mark.parametrize("kind", NETS)
def test_inference_networks_stay_on_the_callers_stream(kind, layout):
    """B = 1 and 8: the one-board form, 8 a paced grid; 37; #CUs + 3: the two-board form; 2 #CUs + 5: the head-plus-remainder double launch"""
    net, n_cu = _net(kind), _n_cu()
    for n in (1, 8, 37, n_cu + 3, 2 * n_cu + 5):
        true, poison = _planes(n, layout, n)
        base, gated = G.run_pair(_net_program(net, true, poison, False))
        _judge("network %s %s B=%d" % (kind, layout, n), base, gated)
        pol = base[0].snaps[0]
        assert torch.isfinite(pol).all() and float((pol.sum(dim=1) - 1).abs().max()) < 1e-3, "the baseline's policy rows are probabilities"


def test_overflow_flag_is_read_from_the_callers_stream(kind="fast_fp16"):
    """one tests/f16range.py network of which one board of four leaves f16's range: overflowed() behind the gated forward must see the flag that forward set"""
    import f16range as FR
    import copy
    from sigma_zero_amd.fastnet import FastPolicyNet
    net = FastPolicyNet(copy.deepcopy(FR.one_bad_board()[0]).cuda(), operands="fp16")
    img = G.nhwc128(FR.boards().numpy().astype(np.uint8))
    true = _dev(G.pack_bits128(img))
    poison = torch.roll(true, 1, 0)
    assert all(not torch.equal(true[b], poison[b]) for b in range(true.shape[0]))
    base, gated = G.run_pair(_net_program(net, true, poison, True))
    _judge("network %s overflowing" % kind, base, gated)


# ---------------------------------------------------------------------------------------------------------------- train kernels
def _train_program(n, node):
    from sigma_zero_amd.trainconv import ConvBNAct, SplitConv3x3
    gen = torch.Generator().manual_seed(100 + n)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=gen) * scale).cuda()
    xt, xp = G.shifted(r(n + 1, 256, 8, 8, scale=0.5), n)
    gt, gp = G.shifted(r(n + 1, 256, 8, 8), n)
    res = r(n, 256, 8, 8, scale=0.5)
    weights = [r(256, 256, 3, 3, scale=0.03) for _ in range(2)]
    gammas, betas = [torch.rand(256, generator=gen).cuda() + 0.5 for _ in range(2)], [r(256, scale=0.1) for _ in range(2)]
    torch.cuda.synchronize()

    def program(sess):
        gy = torch.empty_like(gt)
        models = []
        for i in range(2):                                              # two models with a state and an input of their own each; trainconv._scratch is shared
            m = dict(w=weights[i].clone().requires_grad_(), gamma=gammas[i].clone().requires_grad_(), beta=betas[i].clone().requires_grad_(),
                     mean=torch.zeros(256, device="cuda"), var=torch.ones(256, device="cuda"), x=torch.empty_like(xt).requires_grad_())
            models.append(m)

        def fwd(m):
            if node == "conv":
                m["y"] = SplitConv3x3.apply(m["x"], m["w"])
            else:
                m["y"] = ConvBNAct.apply(m["x"], m["w"], m["gamma"], m["beta"], res, m["mean"], m["var"], 0.1, 1e-5)

        def bwd(m):
            leaves = (m["x"], m["w"]) if node == "conv" else (m["x"], m["w"], m["gamma"], m["beta"])
            m["g"] = torch.autograd.grad(m["y"], leaves, gy)

        with _ctx(sess):                                                # first use on this stream: the allocator's blocks
            with torch.no_grad():
                models[0]["x"].copy_(xp); gy.copy_(gp)
            fwd(models[0]); bwd(models[0])
        torch.cuda.synchronize()
        # one node forward and backward, then two models stepped alternately: program order on ONE stream keeps the shared scratch correct
        for tag, m in (("", models[0]), ("_alt0", models[0]), ("_alt1", models[1])):
            sess.region("forward" + tag, lambda: fwd(m), inputs=[(m["x"], xt, xp)], outputs=lambda _: [m["y"]] + ([] if node == "conv" else [m["mean"], m["var"]]))
            if tag != "_alt0":
                sess.region("backward" + tag, lambda: bwd(m), inputs=[(gy, gt, gp)], outputs=lambda _: list(m["g"]))
        m = models[0]                                                   # model 0's backward behind model 1's whole step: its own saved buffers, the shared partial sums
        sess.region("backward_alt0", lambda: bwd(m), inputs=[(gy, gt, gp)], outputs=lambda _: list(m["g"]))

    return program


@pytest.mark.parametrize("node", ["conv_bn_act", "conv"])
def test_train_kernels_stay_on_the_callers_stream(node):
    for n in (1, 3, _n_cu() // 2 + 1):
        base, gated = G.run_pair(_train_program(n, node))
        _judge("train %s B=%d" % (node, n), base, gated)
        assert all(torch.isfinite(t).all() for r in base for t in r.snaps)


# ---------------------------------------------------------------------------------------------------------------- the Python layer, end to end
def _python_program(misroute_evaluator=False):
    def program(sess):
        fast = _net("fast_bf16")
        with _ctx(sess):
            eng = SelfPlayEngine(fast, {"C": 2, "num_searches": S}, B, chess960=True, learning=True, planes_dtype="bits128")
            eng.new_games(list(STARTS))
        torch.cuda.synchronize()

        def evaluate(planes):                                           # the bug class "a torch op beside a native call on another stream", made on purpose
            with torch.cuda.stream(torch.cuda.default_stream()):
                return eng.evaluate(planes)

        def ply(k):
            eng.search(evaluate if misroute_evaluator and sess.gated else None)
            eng.play(G.gate_uniforms(B, np.random.default_rng([16, k])))
            rec = eng.fetch_ply()
            return rec, tuple(sorted(eng.check_errors().items()))

        for k in range(1 if misroute_evaluator else PLIES):
            sess.region("search+play+fetch_ply+check_errors#%d" % k, lambda: ply(k), blocking=True)
        eng.close()

    return program


def test_selfplay_engine_on_a_side_stream_equals_the_default_stream_run():
    base, gated = G.run_pair(_python_program())
    _judge("python layer SelfPlayEngine", base, gated)


class _EvaluatorElsewhere:
    """a network whose calls go to the default stream whatever stream is current: the Python layer's bug class, made on purpose (the teeth)"""

    def __init__(self, net):
        self._net = net

    def __getattr__(self, name):
        return getattr(self._net, name)

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def __call__(self, planes, inference=True):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return self._net(planes, inference=inference)


def _play_games_program(misroute_evaluator=False):
    """misroute_evaluator (the teeth): four games of one ply on four slots, so that every evaluation is issued while the gate still stands"""
    def program(sess):
        from sigma_zero_amd.sim import play_games
        n, caps = (4, [1] * 4) if misroute_evaluator else (6, [3, 1, 2, 3, 1, 3])
        starts = [(3 * g + 5) % 960 for g in range(n)]
        uniforms = lambda g, ply: ((g * 7919 + ply * 104729 + 4711) % 1000003) / 1000003.0
        net = _net("fast_bf16")
        if misroute_evaluator and sess.gated:
            net = _EvaluatorElsewhere(net)

        def run():
            games = play_games(net, {"C": 2, "num_searches": 8}, n, c960=True, scharnagl=starts, uniforms=uniforms, max_plies=caps,
                               learning=True, planes_dtype="bits128", n_boards=4)
            return [FU.record_of(g) for g in games]

        recs = sess.region("play_games", run, blocking=True)
        assert len(recs) == n and [len(r["chosen_actions"]) for r in recs] == caps

    return program


def test_play_games_on_a_side_stream_equals_the_default_stream_run():
    base, gated = G.run_pair(_play_games_program())
    _judge("python layer play_games", base, gated)


# ---------------------------------------------------------------------------------------------------------------- two engines, two streams, one after the other
def _one_engine(sess, starts, salt):
    """a short program as a generator: it yields behind every region, so that two engines' calls can alternate"""
    eng = _engine(sess, {"C": 2, "num_searches": S})
    lib, e = N.lib(), eng._e
    bufs = _eval_bufs(eng)
    sch = np.array(starts, np.int32)
    sess.region("new_games", lambda: _check(lib.sz_new_games(e, _h(sch), None, _st()), "sz_new_games"), blocking=True)
    yield
    for ply in range(2):
        sess.region("begin#%d" % ply, lambda: _check(lib.sz_search_begin(e, _p(eng.planes), _st()), "sz_search_begin"), outputs=[eng.planes])
        yield
        for k in range(S):
            sess.region("step#%d/%d" % (ply, k), lambda: _check(lib.sz_search_step(e, _p(bufs[0]), _p(bufs[1]), _p(eng.planes), _st()), "sz_search_step"),
                        inputs=_eval_inputs(bufs, (salt, ply, k), B), outputs=[eng.planes])
            yield
        sess.region("debug_tree#%d" % ply, lambda: _trees(eng), blocking=True)
        yield
        u = G.gate_uniforms(B, np.random.default_rng([17, salt, ply]))
        sess.region("play#%d" % ply, lambda: _check(lib.sz_play(e, _p(eng.uniforms), _st()), "sz_play"), inputs=[(eng.uniforms, _dev(u), _dev(G.poison_uniforms(u)))])
        yield
        sess.region("fetch_ply#%d" % ply, eng.fetch_ply, blocking=True)
        yield
    eng.close()


def _two_engines(misroute=None, stop_after=None):
    """engine A on S1, engine B on S2, their calls alternating, each gated; never in flight together (every region ends with its stream synchronised).
    misroute / stop_after: a region of engine A issued on the default stream (the teeth); A stops behind stop_after, B plays on.
    -> [(baseline regions, gated regions) of A, of B]"""
    plans = [(STARTS, 1), (tuple(reversed(STARTS)), 2)]
    bases = []
    for starts, salt in plans:
        base = G.Baseline()
        for _ in _one_engine(base, starts, salt):
            pass
        torch.cuda.synchronize()
        bases.append(base)
    sessions = [G.Gated(bases[0], stream=G.independent_stream(), misroute=misroute, stop_after=stop_after), G.Gated(bases[1], stream=G.independent_stream())]
    assert sessions[0].stream != sessions[1].stream
    live = [_one_engine(s, *plan) for s, plan in zip(sessions, plans)]
    while live:
        for r in list(live):
            try:
                if next(r, "end") == "end":
                    live.remove(r)
            except G.Misrouted:
                live.remove(r)
    torch.cuda.synchronize()
    assert G.compare(bases[0].regions, bases[1].regions), "the two engines play different games"
    return [(b.regions, s.regions) for b, s in zip(bases, sessions)]


def test_two_engines_on_two_streams_keep_to_themselves():
    for name, (base, gated) in zip("AB", _two_engines()):
        _judge("two engines, engine %s" % name, base, gated)


def test_the_gate_sees_a_misrouted_region_of_one_of_two_engines():
    """this family's own harness (two sessions built by hand, two interleaved generators) sees a misrouted launch: a step of engine A goes to the default
    stream while engine B's calls alternate with A's; A differs from its baseline, B still equals its own with every gate held"""
    (base_a, gated_a), (base_b, gated_b) = _two_engines(misroute="step#0/3", stop_after="debug_tree#0")
    _bite("two engines, engine A", base_a, gated_a, "step#0/3")
    assert len(gated_a) < len(base_a)
    _judge("two engines, engine B beside a misrouted A", base_b, gated_b)


# ---------------------------------------------------------------------------------------------------------------- teeth
def _net_teeth(kind):
    true, poison = _planes(8, "bits128", 8)
    return _net_program(_net(kind), true, poison, False)


TEETH = {                                                               # family: (program, the region issued on the default stream, the last region compared)
    "engine core: sz_search_step": (lambda: _core_program("bits128", False), "step#0/3", "debug_tree#0"),
    "engine core: sz_play": (lambda: _core_program("f32", True), "play#0", "fetch_ply#0"),
    "engine core: sz_play_moves": (lambda: _core_program("bf16", True), "play_moves#0", "fetch_moves#0"),
    "ragged batch: sz_search_step behind sz_compact": (lambda: _ragged_program, "step#0/2", "debug_tree"),
    "options: root noise at sz_search_begin and the step behind it": (lambda: _full_program, "step#0/0", "debug_tree#0"),
    "options: a step of the Gumbel search": (lambda: _gumbel_program, "step#0/1", "debug_tree#0"),
    # ply 0: no offset, no cutoff, so every visited child is eligible and p_chosen depends on the board's temperature; the test asserts from the baseline
    # that boards have two or more.  (Ply 1, offset -0.8 with a cutoff after 12 simulations, does not serve: a misrouted sz_play left every record as it
    # was there, which one eligible child per board would explain: any temperature and uniform then play that move with probability 1.)
    "options: temps_dev of sz_set_move_temperature": (lambda: _temperature_program, "play#0", "fetch_temperature#0"),
    "network FastPolicyNet bf16": (lambda: _net_teeth("fast_bf16"), "forward_inference", "forward_inference"),
    "network FastPolicyNet bf16 per-block": (lambda: _net_teeth("fast_bf16_blocks"), "forward_inference", "forward_inference"),
    "network FastPolicyNet fp16": (lambda: _net_teeth("fast_fp16"), "forward_logits+overflowed", "forward_logits+overflowed"),
    "network SplitPolicyNet bf16": (lambda: _net_teeth("split_bf16"), "forward_inference", "forward_inference"),
    "network SplitPolicyNet fp16": (lambda: _net_teeth("split_fp16"), "forward_inference", "forward_inference"),
    "train ConvBNAct forward": (lambda: _train_program(3, "conv_bn_act"), "forward", "forward"),
    "train SplitConv3x3 forward": (lambda: _train_program(3, "conv"), "forward_alt1", "backward_alt1"),
}


@pytest.mark.parametrize("family", list(TEETH))
def test_the_gate_sees_a_misrouted_region(family):
    """misroute=True: the region is issued on the DEFAULT stream while the gate stands on S.  It reads valid memory and valid inputs (the poison), so it
    cannot fault; it must differ from the baseline in at least one output array or host value"""
    make, region, stop = TEETH[family]
    base, gated = G.run_pair(make(), misroute=region, stop_after=stop)
    if region.startswith("play#"):                                      # u and 1 - u choose different children unless one child holds half of the visits
        ply = int(region[5:])
        rc = next((r for r in base if r.name == "root_children#%d" % ply), None)
        if rc is not None:
            visits, n_child = rc.snaps[1].cpu().numpy(), rc.snaps[2].cpu().numpy()
            assert any(not G.same_choice_possible(visits[b, :n_child[b]]) for b in range(B))
        ft = next((r for r in base if r.name == "fetch_temperature#%d" % ply), None)
        if ft is not None:
            assert (ft.host["n_eligible"] >= 2).sum() >= 2, "boards on which the temperature and the uniform can change the move: %s" % ft.host["n_eligible"].tolist()
    _bite(family, base, gated, region)


SPLIT_TEETH = {
    # the Python layer's own bug class: the engine's calls on S, the evaluator's torch and network calls on the default stream.  The evaluations run
    # during the delay, on the planes buffer as it was before sz_search_begin wrote it
    "python layer: the evaluator beside the engine": lambda: _python_program(True),
    "python layer: play_games with the evaluator beside the engine": lambda: _play_games_program(True),
    # a host read that waits for another stream than the call in front of it went to: the setters see the engine between searches and answer SZ_OK
    "refusing setters: sz_search_begin on S, the wait of the setters elsewhere": lambda: (lambda sess: _refusal_program(sess, True)),
}


@pytest.mark.parametrize("family", list(SPLIT_TEETH))
def test_the_gate_sees_two_halves_of_a_region_on_two_streams(family):
    """a whole region moved to the default stream is consistent in itself where nothing of it is a device input; here one half of it goes astray"""
    program = SPLIT_TEETH[family]()
    base = G.Baseline()
    program(base)
    torch.cuda.synchronize()
    gated = G.Gated(base)
    program(gated)
    torch.cuda.synchronize()
    bad = G.compare(base.regions, gated.regions)
    print("%s: %s" % (family, bad))
    assert bad, "%s: one half ran on another stream and everything equals the baseline: the gate has no teeth here" % family
