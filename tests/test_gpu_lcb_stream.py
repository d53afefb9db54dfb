"""include/sigmazero.h: "all device work is enqueued on the caller's stream", for the entry points of the value spread and LCB move selection
(sz_set_lcb, the SpreadOpts / LcbOpts instantiations behind sz_search_begin, sz_search_step and sz_play, sz_root_value_spread, sz_fetch_lcb,
sz_lcb_stats, sz_debug_tree_spread, sz_debug_lcb) behind the gate of tests/streamgate.py, in the manner of
tests/test_gpu_search_summary_stream.py: the program runs once on the default stream and once on a side stream held by a delay kernel with
poisoned inputs, and everything it wrote or returned must be equal, bit for bit.  sz_root_value_spread and k_play's rule have no input array
of their own: they read the tree, Q included, that the last step wrote.  So the last step of a search, the spread readout and the sz_play
behind it are ONE region: a launch that went to another stream runs during the delay, on a tree whose search is not done.  The teeth test
hands that sz_play the default stream while its step went to the session's and requires the comparison to see it; the hook has input arrays and
is misrouted the usual way.  8 boards, 24 searches, 2 plies, every play greedy; evaluations replayed from a seeded generator."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
import streamgate as G
import lcbref as LR

pytestmark = pytest.mark.gpu

B, S, PLIES = 8, 24, 2
STARTS = (0, 959, 518, 400, 77, 5, 811, 333)
OPTS = (0.0, 0.0, True)                                    # the best mean among the children with two visits: the rule decides and often differs from c*


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    yield
    _rows.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _rows(key, n):
    """(policy pool [n+1,4672] f32, value pool [n+1] f32) on the device for one search step: staging tensors, filled once and left unchanged"""
    p, v = G.policy_pool(n + 1, np.random.default_rng([31] + list(key)))
    out = torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    return out


def _check(rc, what):
    assert rc == N.SZ_OK, "%s returned %d" % (what, rc)
    return rc


def _program(plies=PLIES, stray_play=False):
    """stray_play: every sz_play is handed the DEFAULT stream while the step in front of it went to the session's"""
    def program(sess):
        with (torch.cuda.stream(sess.stream) if sess.gated else contextlib.nullcontext()):
            eng = SelfPlayEngine(None, {"C": 2, "num_searches": S}, B, chess960=True, learning=False)
        torch.cuda.synchronize()
        lib, e = N.lib(), eng._e
        pb, vb = torch.zeros(B, N.SZ_ACTIONS, device="cuda"), torch.zeros(B, device="cuda")
        q = torch.zeros(B, N.SZ_MAX_MOVES, dtype=torch.float64, device="cuda")
        sch = np.array(STARTS, np.int32)
        sess.region("new_games", lambda: _check(lib.sz_new_games(e, sch.ctypes.data_as(C.c_void_p), None, _st()), "sz_new_games"), blocking=True)
        sess.region("set_lcb", lambda: eng.set_lcb(OPTS), blocking=True)
        sess.region("fetch_lcb#before", eng.fetch_lcb, blocking=True)
        for ply in range(plies):
            sess.region("begin#%d" % ply, lambda: _check(lib.sz_search_begin(e, _p(eng.planes), _st()), "sz_search_begin"), outputs=[eng.planes])
            for k in range(S):
                (pp, vp) = _rows((ply, k), B)
                ins = [(pb, *G.shifted(pp, B)), (vb, *G.shifted(vp, B))]
                step = lambda: _check(lib.sz_search_step(e, _p(pb), _p(vb), _p(eng.planes), _st()), "sz_search_step")
                if k < S - 1:
                    sess.region("step#%d/%d" % (ply, k), step, inputs=ins, outputs=[eng.planes])
                    continue
                u = np.full(B, -1.0)                                     # greedy: the rule applies on every board
                ut, up = torch.from_numpy(u).cuda(), torch.from_numpy(np.full(B, 0.5)).cuda()

                def issue():
                    step()
                    _check(lib.sz_root_value_spread(e, _p(q), _st()), "sz_root_value_spread")
                    where = C.c_void_p(torch.cuda.default_stream().cuda_stream) if stray_play and sess.gated else _st()
                    _check(lib.sz_play(e, _p(eng.uniforms), where), "sz_play")
                sess.region("step+spread+play#%d" % ply, issue, inputs=ins + [(eng.uniforms, ut, up)], outputs=[q])
            sess.region("fetch_lcb#%d" % ply, eng.fetch_lcb, blocking=True)
            sess.region("lcb_stats#%d" % ply, eng.lcb_stats, blocking=True)
            sess.region("fetch_ply#%d" % ply, eng.fetch_ply, blocking=True)
        sess.region("begin#last", lambda: _check(lib.sz_search_begin(e, _p(eng.planes), _st()), "sz_search_begin"), outputs=[eng.planes])
        sess.region("debug_tree_spread", lambda: eng.debug_tree_spread(0), blocking=True)
        eng.close()
    return program


def _fetched(regions):
    return [r.host for r in regions if r.name.startswith("fetch_lcb#") and not r.name.endswith("before")]


def test_the_option_stays_on_the_callers_stream():
    base, gated = G.run_pair(_program())
    G.write_report("lcb", gated)
    assert len(gated) == len(base)
    bad = G.compare(base, gated)
    assert not bad, "off the caller's stream, or read before the stream was waited for: %s" % bad[:6]
    n = G.assert_held(gated)
    last = _fetched(base)[-1]
    print("%d regions bit-equal to the default-stream baseline, %d gates seen holding; last ply: move %s c* %s" % (len(gated), n, last["move"].tolist(), last["cstar"].tolist()))
    assert n >= PLIES * (S + 1)
    assert all((f["move"] >= 0).all() and f["decided"].all() for f in _fetched(base)), "every board played and the rule decided"
    stats = [r.host for r in base if r.name.startswith("lcb_stats#")]
    assert [s[0] for s in stats] == [B * (p + 1) for p in range(PLIES)] and stats[-1][1] > 0 and stats[-1][2] == 0
    spreads = [r.snaps[0].cpu().numpy() for r in base if r.name.startswith("step+spread+play#")]
    assert all((s >= 0).all() and s.sum() > 0 for s in spreads), "the readout saw the finished search's Q"


def test_the_gate_sees_a_play_on_another_stream():
    base = G.Baseline()
    _program(plies=1)(base)
    torch.cuda.synchronize()
    gated = G.Gated(base)
    _program(plies=1, stray_play=True)(gated)
    torch.cuda.synchronize()
    bad = G.compare(base.regions, gated.regions)
    print("sz_play on the default stream behind the gate's back: %s" % bad[:6])
    assert any(x.startswith("fetch_lcb#0") for x in bad), "k_play ran on the tree as it was before the last step and nothing it wrote differs: the gate has no teeth here"


def _hook_program(sess):
    hc = LR.hook_cases(n_cases=288)
    n = len(hc.opts)
    x = LR.ssqrt_arguments(500)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    fixed = [dev(a) for a in (hc.offsets, hc.opts)]                       # the layout of the cases stays; their numbers are poisoned
    true = [dev(a) for a in (hc.n, hc.N, hc.W, hc.Q, x)]
    poison = [dev(np.maximum(hc.n, 1)[::-1]), dev(np.maximum(hc.N, 2)[::-1]), dev(-hc.W[::-1]), dev(hc.Q[::-1] + 1.0), dev(np.abs(x[::-1]) + 1.0)]
    bufs = [torch.zeros_like(t) for t in true]
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda")
    outs = [i32(n), i32(n), i32(n), i32(n), torch.zeros(len(hc.n), dtype=torch.float64, device="cuda")]
    sx, xb = torch.zeros(len(x), dtype=torch.float64, device="cuda"), i32(len(x))
    torch.cuda.synchronize()
    call = lambda: _check(N.lib().sz_debug_lcb(_p(bufs[4]), _p(sx), _p(xb), len(x), _p(fixed[0]), _p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(bufs[3]), _p(fixed[1]),
                                               *[_p(t) for t in outs], n, _st()), "sz_debug_lcb")
    sess.region("debug_lcb", call, inputs=list(zip(bufs, true, poison)), outputs=outs + [sx, xb])


def test_the_hook_stays_on_the_callers_stream_and_the_gate_sees_it_elsewhere():
    base, gated = G.run_pair(_hook_program)
    G.write_report("lcb", gated)
    assert not G.compare(base, gated) and G.assert_held(gated) == 1
    hc = LR.hook_cases(n_cases=288)
    move, cstar, ncand, bad, lcb, _ = LR.hook_reference(hc)
    snaps = [t.cpu().numpy() for t in base[0].snaps]
    assert np.array_equal(snaps[0], move) and np.array_equal(snaps[1], cstar) and np.array_equal(snaps[2], ncand) and LR.same_bits(snaps[4], lcb).all(), \
        "the baseline is the restatement's answer"
    base, gated = G.run_pair(_hook_program, misroute="debug_lcb")
    bad = G.compare(base, gated)
    assert bad and all(x.startswith("debug_lcb") for x in bad), "a hook launched on the default stream read the poison: the gate has teeth"
