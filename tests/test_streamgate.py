"""CPU checks of tests/streamgate.py, the gate tests/test_gpu_stream_contract.py holds every entry point's stream argument with: the poison builders
make valid inputs that differ from the true ones on every board (legal via the host mirror's szh_legal_actions), the delay arithmetic, and the
"gate held / inconclusive" bookkeeping on a fake event."""
import numpy as np
import pytest
import torch

import sigma_zero_amd as sz
import streamgate as G


def _games(starts=(0, 959, 518, 400, 77, 5, 811, 333), plies=2):
    """Chess960 positions as the GPU test records them: a start position and `plies` moves of the host mirror"""
    games = []
    for n in starts:
        g = sz.ChessTensor(chess960=True, scharnagl=n)
        for k in range(plies):
            acts = sorted(g.legal_action_indices())
            g.push_action(acts[(7 * n + k) % len(acts)])
        games.append(g)
    return games


# ---------------------------------------------------------------------------------------------------------------- poison
def test_policy_poison_is_a_valid_row_and_differs_on_every_board():
    for n in (1, 8, 32):
        p, v = G.policy_pool(n + 1, np.random.default_rng(3))
        (pt, pp), (vt, vp) = G.shifted(p, n), G.shifted(v, n)
        assert pt.shape == pp.shape == (n, 4672) and pt.dtype == pp.dtype == np.float32
        for rows in (pt, pp):
            assert np.isfinite(rows).all() and (rows > 0).all() and (rows < 1).all()
            assert np.abs(rows.sum(axis=1, dtype=np.float64) - 1.0).max() < 1e-5
        # the poison is the true batch rolled by one board: the same rows, hence the same mass row by row
        assert np.array_equal(pp[:-1], pt[1:]) and np.array_equal(pp.sum(axis=1)[:-1], pt.sum(axis=1)[1:])
        assert all(not np.array_equal(pt[b], pp[b]) for b in range(n))
        assert (np.abs(vt) < 1).all() and (np.abs(vp) < 1).all() and (vt != vp).all()


def test_uniform_poison_lies_in_range_and_cannot_choose_the_same_child():
    rng = np.random.default_rng(4)
    u = G.gate_uniforms(4096, rng)
    q = G.poison_uniforms(u)
    for x in (u, q):
        assert x.dtype == np.float64 and (x >= 0).all() and (x < 1).all()
    assert (np.abs(u - q) >= 0.5).all()
    # sz_play's cumulative rule: u and 1 - u fall on one child only if that child holds at least half of the visits
    same = 0
    for k in range(2000):
        visits = rng.integers(0, 6, size=int(rng.integers(2, 40))).astype(np.int64)
        if visits.sum() == 0:
            continue
        a, b = G.pick(visits, u[k]), G.pick(visits, q[k])
        assert visits[a] > 0 and visits[b] > 0
        if a == b:
            same += 1
            assert G.same_choice_possible(visits), (visits, u[k])
    assert same > 0, "the draw reached the case the GPU test has to exclude"
    assert G.pick([7, 1], 0.2) == G.pick([7, 1], 0.8) == 0 and G.same_choice_possible([7, 1]) and not G.same_choice_possible([3, 4, 2])
    assert G.pick([3, 4, 2], 0.2) == 0 and G.pick([3, 4, 2], 0.8) == 2


def test_action_poison_is_another_legal_move_of_the_recorded_position():
    games = _games()
    legal = [g.legal_action_indices() for g in games]
    true, poison = G.gate_actions(legal, np.random.default_rng(5))
    assert true.dtype == poison.dtype == np.int32 and len(true) == len(games)
    for g, t, p in zip(games, true, poison):
        acts = set(g.legal_action_indices())                             # szh_legal_actions of the position
        assert t in acts and p in acts and t != p and 0 <= t < 4672 and 0 <= p < 4672
        for a in (t, p):                                                 # ... and the host mirror plays both
            h = g.copy()
            h.push_action(int(a))
    over, _ = G.gate_actions([[], [5, 9]], np.random.default_rng(5))
    assert over[0] == -1 and over[1] in (5, 9)
    with pytest.raises(AssertionError):
        G.gate_actions([[17]], np.random.default_rng(5))


def test_planes_poison_is_a_valid_image_in_both_layouts():
    from sigma_zero_amd.selfplay import unpack_bits128
    from sigma_zero_amd.fastnet import planes_nchw_to_nhwc128
    for n in (1, 8):
        x = G.random_planes(n + 1, np.random.default_rng(6))
        assert x.dtype == np.uint8 and set(np.unique(x)) <= {0, 1}
        img = G.nhwc128(x)
        assert img.shape == (n + 1, 64, 128) and not img[:, :, 119:].any()
        assert torch.equal(torch.from_numpy(img).to(torch.bfloat16), planes_nchw_to_nhwc128(torch.from_numpy(x).float()))
        bits = G.pack_bits128(img)
        assert bits.shape == (n + 1, 1024) and bits.dtype == np.uint8
        assert torch.equal(unpack_bits128(torch.from_numpy(bits)), torch.from_numpy(img).to(torch.bfloat16))      # the engine's own decoder
        for lay in (img, bits):
            t, p = G.shifted(lay, n)
            assert all(not np.array_equal(t[b], p[b]) for b in range(n))


# ---------------------------------------------------------------------------------------------------------------- delay arithmetic
def test_delay_arithmetic():
    assert G.delay_ms(0.0) == 10.0 and G.delay_ms(0.0004) == 10.0        # 20 x 0.4 ms = 8 ms: the floor holds
    assert G.delay_ms(0.0005) == 10.0 and G.delay_ms(0.002) == pytest.approx(40.0) and G.delay_ms(0.1) == pytest.approx(2000.0)
    with pytest.raises(ValueError):
        G.delay_ms(float("nan"))
    # two timed delays with a fixed launch cost of 0.05 ms at 2000 units per ms: the slope recovers the rate, the cost drops out
    per_ms = G.units_per_ms(2_000_000, 1000.05, 20_000_000, 10000.05)
    assert per_ms == pytest.approx(2000.0)
    assert G.units_for(10.0, per_ms) >= 20000 and G.units_for(10.0, per_ms) / per_ms >= 10.0
    assert G.units_for(0.0101, 1000.0) == 11                             # rounds up: never shorter than asked
    for bad in ((2, 1.0, 1, 2.0), (1, 1.0, 2, 1.0), (1, 2.0, 2, 1.0), (0, 0.0, 2, 1.0)):
        with pytest.raises(G.Inconclusive):
            G.units_per_ms(*bad)
    with pytest.raises(ValueError):
        G.units_for(10.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------- bookkeeping
class FakeEvent:
    def __init__(self, done):
        self.done, self.queries = done, 0

    def query(self):
        self.queries += 1
        return self.done


def _region(name, held, blocking=False, delay=10.0):
    return G.Region(name, None, [], 1e-4, delay, held, blocking, False)


def test_gate_held_bookkeeping_on_a_fake_event():
    pending, done = FakeEvent(False), FakeEvent(True)
    assert G.gate_held(pending) is True and G.gate_held(done) is False and pending.queries == done.queries == 1
    ok = [_region("begin", True), _region("fetch_ply", None, blocking=True), _region("step#0", True)]
    assert G.unheld(ok) == [] and G.assert_held(ok) == 2                 # the blocking region is not judged by the event
    for bad in (False, None):                                            # seen finished, or never looked at: inconclusive either way
        rs = ok + [_region("step#1", bad)]
        assert G.unheld(rs) == ["step#1"]
        with pytest.raises(G.Inconclusive):
            G.assert_held(rs)
    assert issubclass(G.Inconclusive, AssertionError)                    # pytest reports it as a failure, never as a pass or a skip
    skipped = [_region("step#2", None, delay=None)]                      # a baseline region (no delay, no event) is not judged
    assert G.unheld(skipped) == [] and G.assert_held(skipped) == 0


def test_compare_reports_host_values_outputs_and_divergence():
    a = G.Region("play", (0, np.arange(3)), [torch.arange(4.0)], 0.0, None, None, False, False)
    same = G.Region("play", (0, np.arange(3)), [torch.arange(4.0)], 0.0, 10.0, True, False, False)
    assert G.compare([a], [same]) == []
    host = same._replace(host=(0, np.array([0, 1, 3])))
    dev = same._replace(snaps=[torch.tensor([0.0, 1.0, 2.0, -3.0])])
    zero = same._replace(snaps=[torch.tensor([-0.0, 1.0, 2.0, 3.0])])    # raw bits: -0.0 is not 0.0
    assert G.compare([a], [host]) == ["play: host values"] and G.compare([a], [dev]) == ["play: device output 0"] == G.compare([a], [zero])
    assert G.compare([a], [same._replace(name="step#0")])[0].startswith("region 0")
    assert G.compare([a, a], [same]) == []                               # a misrouted pass stops early
    lines = G.report_lines("engine core", [same, same._replace(name="fetch_ply", blocking=True, held=None)])
    assert len(lines) == 2 and "held 1/1" in lines[0] and "blocking" in lines[1]
