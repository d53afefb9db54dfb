"""The restatement of the move-selection temperature (tests/tempref.py) on the CPU: its cases reach every branch of the rule, at T = 1 it is the
sampling of sz_play bit for bit, it never plays a child that is not eligible, its probabilities agree with math.pow, and the Python layer's
schedule and validation (selfplay.temperature_at / temperature_options_of).  tests/test_gpu_temperature.py holds the device to it."""
import math

import numpy as np
import pytest

import tempref as TR
from reuseref import choose as plain_choose
from sigma_zero_amd.selfplay import temperature_at, temperature_options_of

TOP = float(np.nextafter(1.0, 0.0))
MEASURED_REL_ERR = 2.2e-14                                 # the largest deviation test_accuracy_against_pow has seen, at T = 0.05
REL_ERR_BOUND = 4 * MEASURED_REL_ERR

_played = {}


def _play(name, **kw):
    key = (name, tuple(sorted(kw.items(), key=str)))
    if key not in _played:
        _played[key] = TR.play(next(c for c in TR.CONFIGS if c.name == name), **kw)
    return _played[key]


def _same_record(a, b):
    if a is None or b is None:
        return a is b
    return all(np.array_equal(a[k], b[k]) for k in ("packed", "action", "visits")) and \
        all(int(a[k]) == int(b[k]) for k in ("n_child", "colour", "chosen", "game_over", "result"))


# ------------------------------------------------------------------------------------------------ 1. the cases reach every branch
def test_hook_cases_reach_every_branch():
    hc = TR.hook_cases()
    assert len(hc.T) >= 3000 and set(np.diff(hc.offsets).tolist()) == set(TR.HOOK_K)
    *_, cov = TR.hook_reference(hc)
    assert all(cov[k] > 0 for k in TR.HOOK_COVERAGE), {k: cov[k] for k in TR.HOOK_COVERAGE}
    combos = set()
    for i in range(len(hc.T)):
        off = float(hc.opts[i]["visit_offset"])
        lo, hi = int(hc.offsets[i]), int(hc.offsets[i + 1])
        okind = "minus_max" if off == -float(hc.n[lo:hi].max()) and off not in (-1.0, -2.0) else off
        combos.add(("nan" if math.isnan(hc.T[i]) else float(hc.T[i]), okind, float(hc.opts[i]["value_cutoff"]) if hc.opts[i]["use_cutoff"] else None))
    for T in TR.HOOK_T:
        for off in (0.0, -0.5, float(np.float32(-0.8)), 2.0, "minus_max"):
            for cut in (None, 0.0, float(np.float32(0.1)), 2.0):
                assert ("nan" if math.isnan(T) else T, off, cut) in combos, (T, off, cut)
    assert {0.0, TOP, -1.0} <= set(hc.u.tolist()) and len(set(hc.u.tolist())) > 100


def test_engine_configurations_reach_every_branch():
    cov = TR.coverage([g for cfg in TR.CONFIGS for g in _play(cfg.name)[0]])
    assert all(cov[k] > 0 for k in TR.COVERAGE), {k: cov[k] for k in TR.COVERAGE}
    assert cov["ended_resign"] > 0, "an ending fires under the option: the board plays no move and reads no temperature"
    for cfg in TR.CONFIGS:
        games, recs = _play(cfg.name)
        assert len(games) == 8 and cfg.S == 24 and len(recs) == 8
        assert all(sum(g.temp_stats[:2]) == len(g.choices) for g in games)
        temps = [TR.temps_of(ply) for ply in range(cfg.plies)]
        assert all(len(set(row)) > 1 for row in temps) and all(len({temps[p][b] for p in range(cfg.plies)}) > 1 for b in range(8)), "T differs per board and per ply"
    assert all(g.starts[1:] and all(s == "reused" for s in g.starts[1:]) for g in _play("reuse_subtree")[0] if len(g.starts) > 1)


# ------------------------------------------------------------------------------------------------ 2. T = 1 is today's sampling, bit for bit
def test_exact_at_temperature_1():
    rng = np.random.default_rng(7)
    plain = TR.options()
    for i in range(4000):
        k = (1, 2, 63, 64, 65, 218)[i % 6]
        n = rng.integers(0, (4, 40, 1000)[i % 3], size=k)
        if n.max() < 1:
            n[rng.integers(0, k)] = 1
        W = rng.uniform(-1, 1, size=k) * n
        u = (0.0, TOP, -1.0)[i % 5] if i % 5 < 3 else float(rng.random())
        ch = TR.choose(n, n, W, 1.0, u, plain)
        assert ch.move == plain_choose(n, u), (i, n.tolist(), u)
        if u >= 0.0:
            assert ch.weights == n.astype(np.float64).tolist() and ch.n_eligible == int((n >= 1).sum()) and ch.excluded == 0
            assert np.float64(ch.p_chosen).tobytes() == (np.float64(n[ch.move]) / np.float64(n.sum())).tobytes()
        zero = TR.choose(n, n, W, 0.0, abs(u), plain)                      # T = 0 is the negative uniform
        assert zero.kind == TR.GREEDY and zero.move == plain_choose(n, -1.0)


def test_games_at_temperature_1_are_the_games_without_the_option():
    for cfg in TR.CONFIGS:
        (off, recs_off), (on, recs_on) = _play(cfg.name, temperature=False), _play(cfg.name, opts=TR.options(), T=1.0)
        assert all(_same_record(a, b) for ra, rb in zip(recs_off, recs_on) for a, b in zip(ra, rb)), cfg.name
        assert [g.chosen for g in off] == [g.chosen for g in on] and sum(len(g.chosen) for g in on) > 40
        assert all(g.temp_stats == [0, 0, 0] and not g.choices for g in off) and sum(g.temp_stats[0] for g in on) > 30
        (zero, recs_zero), (greedy, recs_greedy) = _play(cfg.name, opts=TR.options(), T=0.0), _play(cfg.name, temperature=False, u=lambda b, ply: -1.0)
        assert all(_same_record(a, b) for ra, rb in zip(recs_zero, recs_greedy) for a, b in zip(ra, rb)), cfg.name
        assert all(g.temp_stats[0] == 0 for g in zero)


# ------------------------------------------------------------------------------------------------ 3. no child that is not eligible is played
def test_no_ineligible_child_is_played():
    rng = np.random.default_rng(8)
    n_cases = 0
    for i in range(3000):
        k = (2, 5, 63, 64, 65, 218)[i % 6]
        n = rng.integers(0, 6, size=k)
        if i % 4 == 0:
            n[-(k // 2):] = 0                                                  # trailing children of weight 0
        if i % 4 == 1:
            n[:k // 2] = 0                                                     # leading ones
        if n.max() < 1:
            n[rng.integers(0, k)] = 3
        W = rng.uniform(-1, 1, size=k) * n
        T = (0.05, 0.25, 0.5, 1.0, 1.5, 4.0)[int(rng.integers(0, 6))]
        o = TR.options((0.0, -0.5, -0.8, -1.0, -2.0, 2.0)[int(rng.integers(0, 6))], (None, 0.0, 0.1, 2.0)[int(rng.integers(0, 4))])
        for u in (0.0, TOP, float(rng.random()), int(rng.integers(0, 64)) / 64.0):
            ch = TR.choose(n, n, W, T, u, o)
            if ch.kind != TR.SAMPLED:
                continue
            n_cases += 1
            assert ch.eligible[ch.move] and ch.weights[ch.move] > 0.0 and n[ch.move] >= 1, (i, u, n.tolist(), ch)
            assert ch.eligible[TR.first_max(n)] and ch.weights[TR.first_max(n)] == (float(n.max()) + o.visit_offset if T == 1.0 else 1.0)
            assert 0.0 < ch.p_chosen <= 1.0 and ch.n_eligible + ch.excluded == int((n >= 1).sum())
    assert n_cases > 5000


# ------------------------------------------------------------------------------------------------ 4. accuracy against math.pow
def test_accuracy_against_pow():
    """w_c / S against (a_c / a_c*) ** (1 / T) normalised (math.pow, sums by math.fsum), over every sampled hook case: the hook's own T range,
    0.05 to 4, counts up to 800.  The largest relative deviation measured on the CPU is 2.2e-14 (case 794: T = 0.05, a = 21.2 against
    a* = 799.2, the exponent 20 multiplies slog's rounding); the bound is four times that, 8.8e-14."""
    hc = TR.hook_cases()
    worst, n_terms = 0.0, 0
    for i in range(len(hc.T)):
        lo, hi = int(hc.offsets[i]), int(hc.offsets[i + 1])
        o = TR.Temp(float(hc.opts[i]["visit_offset"]), float(hc.opts[i]["value_cutoff"]), int(hc.opts[i]["use_cutoff"]))
        ch = TR.choose(hc.n[lo:hi], hc.N[lo:hi], hc.W[lo:hi], hc.T[i], hc.u[i], o)
        if ch.kind != TR.SAMPLED:
            continue
        T = float(hc.T[i])
        a = [float(x) + o.visit_offset for x in hc.n[lo:hi]]
        amax = max(x for x, e in zip(a, ch.eligible) if e)
        ref = [math.pow(x / amax, 1.0 / T) if e else 0.0 for x, e in zip(a, ch.eligible)]
        s_ref, s = math.fsum(ref), math.fsum(ch.weights)
        for c in range(hi - lo):
            if ch.eligible[c] and ref[c] / s_ref > 1e-290:
                worst = max(worst, abs((ch.weights[c] / s) / (ref[c] / s_ref) - 1.0))
                n_terms += 1
    print("w / S against math.pow: %d terms, largest relative deviation %.3g (bound %.3g)" % (n_terms, worst, REL_ERR_BOUND))
    assert n_terms > 50000 and worst <= REL_ERR_BOUND


# ------------------------------------------------------------------------------------------------ 5. the schedule
def test_schedule():
    step = temperature_options_of({"temperature": {}})
    assert step == dict(t0=1.0, t_final=0.0, plies=60, halflife=None, fast=None, visit_offset=0.0, value_cutoff=None)
    assert [temperature_at(step, p) for p in (0, 1, 59, 60, 61, 500)] == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    az = temperature_options_of({"temperature": {"plies": 30, "t0": 1.0, "t_final": 0.25}})
    assert [temperature_at(az, p) for p in (0, 29, 30, 31)] == [1.0, 1.0, 0.25, 0.25]
    assert temperature_at(temperature_options_of({"temperature": {"plies": 0}}), 0) == 0.0
    half = temperature_options_of({"temperature": {"t0": 1.0, "t_final": 0.2, "plies": 10, "halflife": 8}})
    assert [temperature_at(half, p) for p in (0, 9, 10)] == [1.0, 1.0, 1.0]
    assert temperature_at(half, 18) == 0.2 + 0.8 * 0.5 and temperature_at(half, 26) == 0.2 + 0.8 * 0.25
    assert temperature_at(half, 14) == 0.2 + (1.0 - 0.2) * 0.5 ** (4 / 8.0)
    later = [temperature_at(half, p) for p in range(10, 200)]
    assert all(x >= y for x, y in zip(later, later[1:])) and later[-1] > 0.2 and later[-1] - 0.2 < 1e-6
    fast = temperature_options_of({"temperature": {"fast": 0.0, "plies": 30}, "playout_cap": {"fast": 8, "p_full": 0.25}, "num_searches": 32})
    assert temperature_at(fast, 3, full=False) == 0.0 and temperature_at(fast, 3, full=True) == 1.0 and temperature_at(fast, 3) == 1.0
    assert temperature_at(step, 3, full=False) == 1.0, "no 'fast': fast plies follow the schedule"
    assert isinstance(temperature_at(half, 14), float)


# ------------------------------------------------------------------------------------------------ 6. validation
def test_validation():
    assert temperature_options_of({}) is None and temperature_options_of({"temperature": None}) is None
    ok = temperature_options_of({"temperature": {"visit_offset": -0.8, "value_cutoff": 0.1, "t_final": 0.5, "halflife": 12.5}})
    assert ok["visit_offset"] == float(np.float32(-0.8)) and ok["value_cutoff"] == float(np.float32(0.1)) and ok["halflife"] == 12.5
    nan, inf = float("nan"), float("inf")
    bad = [5, {"T": 1.0}, {"t0": -0.5}, {"t0": nan}, {"t0": inf}, {"t0": True}, {"t0": "1"}, {"t_final": -1.0}, {"t_final": nan}, {"t_final": inf},
           {"plies": -1}, {"plies": 2.5}, {"plies": True}, {"halflife": 0}, {"halflife": -3.0}, {"halflife": nan}, {"halflife": inf}, {"halflife": "8"},
           {"fast": -0.1}, {"fast": nan}, {"visit_offset": nan}, {"visit_offset": inf}, {"visit_offset": 1e39}, {"visit_offset": None},
           {"value_cutoff": -0.1}, {"value_cutoff": nan}, {"value_cutoff": inf}, {"value_cutoff": True}]
    for t in bad:
        with pytest.raises(ValueError):
            temperature_options_of({"temperature": t, "playout_cap": {"fast": 8, "p_full": 0.5}, "num_searches": 32})
    with pytest.raises(ValueError):                                            # fast plies exist only under playout_cap
        temperature_options_of({"temperature": {"fast": 0.0}})
    with pytest.raises(ValueError):                                            # Gumbel chooses its own move
        temperature_options_of({"temperature": {}, "gumbel": {"m": 8}})
    from sigma_zero_amd import train_rl
    flags = train_rl.flag_parser()
    assert "temperature" not in train_rl.selfplay_args_of(flags.parse_args([]))
    a = train_rl.selfplay_args_of(flags.parse_args(["--temperature-plies", "30", "--temperature-final", "0.1", "--temperature-halflife", "20",
                                                    "--temperature-fast", "0", "--temp-visit-offset", "-0.8", "--temp-value-cutoff", "0.1",
                                                    "--playout-cap-fast", "8"]))
    assert a["temperature"] == {"plies": 30, "t_final": 0.1, "halflife": 20.0, "fast": 0.0, "visit_offset": -0.8, "value_cutoff": 0.1}
    assert temperature_options_of(dict(a, num_searches=32))["t0"] == 1.0
    from sigma_zero_amd.arena import play_options_match
    with pytest.raises(ValueError):                                            # the schedule says which plies are sampled
        play_options_match(None, {"C": 2, "num_searches": 8, "temperature": {}}, {"C": 2, "num_searches": 8}, 1, sample_plies=2)
