"""include/sigmazero.h: "all device work is enqueued on the caller's stream", for the entry points of the search summary (sz_set_search_summary,
sz_play's two summary kernels, sz_fetch_search_summary, sz_search_summary_stats, sz_debug_search_summary) behind the gate of tests/streamgate.py,
in the manner of tests/test_gpu_kld_stop_stream.py: the program runs once on the default stream and once on a side stream held by a delay kernel
with poisoned inputs, and everything it wrote or returned must be equal, bit for bit.  The summary kernels have no input array of their own:
k_summary_pre reads the tree the last step wrote, k_summary_post the record k_play wrote.  So the last step of a search and the sz_play behind
it are ONE region: summary kernels that went to another stream run during the delay, on a tree whose search is not done, and make no summary.
The teeth test hands that sz_play the default stream while its step went to the session's and requires the comparison to see it; the hook has
input arrays and is misrouted the usual way.  8 boards, 24 searches, 2 plies; evaluations replayed from a seeded generator."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import SelfPlayEngine
import streamgate as G
import summaryref as SR

pytestmark = pytest.mark.gpu

B, S, PLIES = 8, 24, 2
STARTS = (0, 959, 518, 400, 77, 5, 811, 333)


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
    p, v = G.policy_pool(n + 1, np.random.default_rng([23] + list(key)))
    out = torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    return out


def _check(rc, what):
    assert rc == N.SZ_OK, "%s returned %d" % (what, rc)
    return rc


def _program(plies=PLIES, stray_play=False):
    """stray_play: every sz_play is handed the DEFAULT stream while the step in front of it went to the session's: what a stream bug in a
    driver, or in the entry point, looks like"""
    def program(sess):
        with (torch.cuda.stream(sess.stream) if sess.gated else contextlib.nullcontext()):
            eng = SelfPlayEngine(None, {"C": 2, "num_searches": S}, B, chess960=True, learning=False)
        torch.cuda.synchronize()
        lib, e = N.lib(), eng._e
        pb, vb = torch.zeros(B, N.SZ_ACTIONS, device="cuda"), torch.zeros(B, device="cuda")
        sch = np.array(STARTS, np.int32)
        sess.region("new_games", lambda: _check(lib.sz_new_games(e, sch.ctypes.data_as(C.c_void_p), None, _st()), "sz_new_games"), blocking=True)
        sess.region("set_search_summary", lambda: eng.set_search_summary(True), blocking=True)
        sess.region("fetch_search_summary#before", eng.fetch_search_summary, blocking=True)
        for ply in range(plies):
            sess.region("begin#%d" % ply, lambda: _check(lib.sz_search_begin(e, _p(eng.planes), _st()), "sz_search_begin"), outputs=[eng.planes])
            for k in range(S):
                (pp, vp) = _rows((ply, k), B)
                ins = [(pb, *G.shifted(pp, B)), (vb, *G.shifted(vp, B))]
                step = lambda: _check(lib.sz_search_step(e, _p(pb), _p(vb), _p(eng.planes), _st()), "sz_search_step")
                if k < S - 1:
                    sess.region("step#%d/%d" % (ply, k), step, inputs=ins, outputs=[eng.planes])
                    continue
                u = G.gate_uniforms(B, np.random.default_rng([29, ply]))
                ut, up = torch.from_numpy(u).cuda(), torch.from_numpy(G.poison_uniforms(u)).cuda()

                def issue():
                    step()
                    where = C.c_void_p(torch.cuda.default_stream().cuda_stream) if stray_play and sess.gated else _st()
                    _check(lib.sz_play(e, _p(eng.uniforms), where), "sz_play")
                sess.region("step+play#%d" % ply, issue, inputs=ins + [(eng.uniforms, ut, up)])
            sess.region("fetch_search_summary#%d" % ply, eng.fetch_search_summary, blocking=True)
            sess.region("search_summary_stats#%d" % ply, eng.search_summary_stats, blocking=True)
            sess.region("fetch_ply#%d" % ply, eng.fetch_ply, blocking=True)
        sess.region("set_search_summary_off", lambda: eng.set_search_summary(False), blocking=True)
        eng.close()
    return program


def _fetched(regions):
    return [r.host for r in regions if r.name.startswith("fetch_search_summary#") and not r.name.endswith("before")]


def test_the_summary_stays_on_the_callers_stream():
    base, gated = G.run_pair(_program())
    G.write_report("search_summary", gated)
    assert len(gated) == len(base)
    bad = G.compare(base, gated)
    assert not bad, "off the caller's stream, or read before the stream was waited for: %s" % bad[:6]
    n = G.assert_held(gated)
    last = _fetched(base)[-1]
    print("%d regions bit-equal to the default-stream baseline, %d gates seen holding; last ply: valid %s root_q %s" % (len(gated), n, last["valid"].tolist(), last["root_q"].tolist()))
    assert n >= PLIES * (S + 1)
    assert all(f["valid"].all() and not np.isnan(f["surprise"]).any() for f in _fetched(base)), "every board played: both kernels ran"
    assert [r.host for r in base if r.name.startswith("search_summary_stats#")] == [(B * (p + 1), 0) for p in range(PLIES)]


def test_the_gate_sees_a_play_on_another_stream():
    base = G.Baseline()
    _program(plies=1)(base)
    torch.cuda.synchronize()
    gated = G.Gated(base)
    _program(plies=1, stray_play=True)(gated)
    torch.cuda.synchronize()
    bad = G.compare(base.regions, gated.regions)
    print("sz_play on the default stream behind the gate's back: %s" % bad[:6])
    assert any(x.startswith("fetch_search_summary#0") for x in bad), "the summary kernels ran on the tree as it was before the last step and nothing they wrote differs: the gate has no teeth here"


def _hook_program(sess):
    hc = SR.hook_cases(n_random=200)
    n = len(hc.n_child)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    true = [dev(x) for x in (hc.n_child, hc.tree_vc, hc.value_sum, hc.prior, hc.record_vc)]
    poison = [t.flip(0).contiguous() for t in true]                      # another valid case on every row but the middle one
    bufs = [torch.zeros_like(t) for t in true]
    out = torch.zeros(n, 3, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sess.region("debug_search_summary", lambda: _check(N.lib().sz_debug_search_summary(*[_p(t) for t in bufs], _p(out), n, _st()), "sz_debug_search_summary"),
                inputs=list(zip(bufs, true, poison)), outputs=[out])


def test_the_hook_stays_on_the_callers_stream_and_the_gate_sees_it_elsewhere():
    base, gated = G.run_pair(_hook_program)
    G.write_report("search_summary", gated)
    assert not G.compare(base, gated) and G.assert_held(gated) == 1
    hc = SR.hook_cases(n_random=200)
    assert not (~SR.same_bits(base[0].snaps[0].cpu().numpy(), SR.hook_reference(hc))).any(), "the baseline is the restatement's answer"
    base, gated = G.run_pair(_hook_program, misroute="debug_search_summary")
    bad = G.compare(base, gated)
    assert bad and all(x.startswith("debug_search_summary") for x in bad), "a hook launched on the default stream read the poison: the gate has teeth"
