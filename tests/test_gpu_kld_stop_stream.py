"""include/sigmazero.h: "all device work is enqueued on the caller's stream", for the entry points of KLD-gain early stopping (sz_set_kld_stop,
sz_search_begin's goal and reset kernels, sz_search_check_stop, sz_fetch_kld_stop, sz_kld_stop_stats, sz_search_goals under the option) behind the
gate of tests/streamgate.py, in the manner of tests/test_gpu_stream_contract.py: the program runs once on the default stream and once on a side
stream held by a delay kernel with poisoned inputs, and everything it wrote or returned must be equal, bit for bit.  The check has no input
array of its own: it reads the tree the step in front of it wrote.  So a step and the check behind it are ONE region: a check that went to
another stream runs during the delay, on the tree as it was before the step.  The teeth test sends the check alone to the default stream and
requires the comparison to see it.  8 boards, 24 searches, interval 4, 2 plies; evaluations replayed from a seeded generator."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
import streamgate as G

pytestmark = pytest.mark.gpu

B, S, PLIES, INTERVAL = 8, 24, 2, 4
STARTS = (0, 959, 518, 400, 77, 5, 811, 333)
KLD = {"min_gain": 1e-1, "interval": INTERVAL, "min_simulations": 8}


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
    p, v = G.policy_pool(n + 1, np.random.default_rng([17] + list(key)))
    out = torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    return out


def _check(rc, what):
    assert rc == N.SZ_OK, "%s returned %d" % (what, rc)
    return rc


def _program(stray_check=False):
    """stray_check: every sz_search_check_stop is handed the DEFAULT stream while its step went to the session's: what a stream bug in a driver, or in
    the entry point, looks like"""
    def program(sess):
        with (torch.cuda.stream(sess.stream) if sess.gated else contextlib.nullcontext()):
            eng = SelfPlayEngine(None, {"C": 2, "num_searches": S, "reuse_subtree": True}, B, chess960=True, learning=True)
        torch.cuda.synchronize()
        lib, e = N.lib(), eng._e
        pb, vb = torch.zeros(B, N.SZ_ACTIONS, device="cuda"), torch.zeros(B, device="cuda")
        sch = np.array(STARTS, np.int32)
        sess.region("new_games", lambda: _check(lib.sz_new_games(e, sch.ctypes.data_as(C.c_void_p), None, _st()), "sz_new_games"), blocking=True)
        sess.region("set_kld_stop", lambda: eng.set_kld_stop((KLD["min_gain"], KLD["interval"], KLD["min_simulations"])), blocking=True)
        for ply in range(PLIES):
            sess.region("begin#%d" % ply, lambda: _check(lib.sz_search_begin(e, _p(eng.planes), _st()), "sz_search_begin"), outputs=[eng.planes])
            sess.region("goals#%d" % ply, eng.search_goals, blocking=True)
            for k in range(S):
                (pp, vp) = _rows((ply, k), B)
                ins = [(pb, *G.shifted(pp, B)), (vb, *G.shifted(vp, B))]
                check = k % INTERVAL == INTERVAL - 1

                def issue():
                    _check(lib.sz_search_step(e, _p(pb), _p(vb), _p(eng.planes), _st()), "sz_search_step")
                    if check:
                        where = C.c_void_p(torch.cuda.default_stream().cuda_stream) if stray_check and sess.gated else _st()
                        _check(lib.sz_search_check_stop(e, where), "sz_search_check_stop")
                sess.region("step%s#%d/%d" % ("+check" if check else "", ply, k), issue, inputs=ins, outputs=[eng.planes])
                if check:
                    sess.region("fetch_kld_stop#%d/%d" % (ply, k), eng.fetch_kld_stop, blocking=True)
            sess.region("kld_stop_stats#%d" % ply, eng.kld_stop_stats, blocking=True)
            sess.region("stats#%d" % ply, lambda: tuple(sorted(eng.stats().items())), blocking=True)
            sess.region("debug_tree#%d" % ply, lambda: [eng.debug_tree(b) for b in range(B)], blocking=True)
            u = G.gate_uniforms(B, np.random.default_rng([19, ply]))
            ut, up = torch.from_numpy(u).cuda(), torch.from_numpy(G.poison_uniforms(u)).cuda()
            sess.region("play#%d" % ply, lambda: _check(lib.sz_play(e, _p(eng.uniforms), _st()), "sz_play"), inputs=[(eng.uniforms, ut, up)])
            sess.region("fetch_ply#%d" % ply, eng.fetch_ply, blocking=True)
        sess.region("set_kld_stop_off", lambda: eng.set_kld_stop(None), blocking=True)
        eng.close()
    return program


def _fetched(regions):
    return [r.host for r in regions if r.name.startswith("fetch_kld_stop#")]


def test_the_stopping_rule_stays_on_the_callers_stream():
    base, gated = G.run_pair(_program())
    G.write_report("kld_stop", gated)
    assert len(gated) == len(base)
    bad = G.compare(base, gated)
    assert not bad, "off the caller's stream, or read before the stream was waited for: %s" % bad[:6]
    n = G.assert_held(gated)
    last = _fetched(base)[S // INTERVAL - 1]
    print("%d regions bit-equal to the default-stream baseline, %d gates seen holding; ply 0: stopped_at %s checks %s"
          % (len(gated), n, last["stopped_at"].tolist(), last["checks"].tolist()))
    assert n >= PLIES * (S + 2)
    assert (last["checks"] >= 1).all(), "every board formed a gain: the rule ran"
    assert any((f["stopped_at"] >= 0).any() for f in _fetched(base)), "a board stopped: the goal was lowered behind the gate too"


def test_the_gate_sees_a_check_on_another_stream():
    base = G.Baseline()
    _program()(base)
    torch.cuda.synchronize()
    gated = G.Gated(base)
    _program(stray_check=True)(gated)
    torch.cuda.synchronize()
    bad = G.compare(base.regions, gated.regions)
    print("sz_search_check_stop on the default stream behind the gate's back: %s" % bad[:6])
    assert any(x.startswith("fetch_kld_stop#") for x in bad), "the check ran on the tree as it was before its step and nothing it wrote differs: the gate has no teeth here"
