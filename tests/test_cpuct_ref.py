"""The restatement of the visit-dependent exploration rate (tests/puctref.py) on the CPU: c_of against math.log, exact at factor 0, bit for bit
the host compilation of csrc/sz_cpuct.h, fullref with c = C at (C, b, 0), the conditions the GPU configurations are there for, and the Python
layer's validation (selfplay.cpuct_options_of).  tests/test_gpu_cpuct.py holds the device to it."""
import math
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import fullref as FU
import puctref as PR
from puctref import Cpuct
from sigma_zero_amd.selfplay import cpuct_options_of

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sigma-zero_amd", "csrc")
_played = {}


def _play(name, **kw):
    key = (name, tuple(sorted(kw.items(), key=str)))
    if key not in _played:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _played[key] = PR.play(next(c for c in PR.configs() if c.name == name), **kw)
    return _played[key]


def _same_record(a, b):
    if a is None or b is None:
        return a is b
    return all(np.array_equal(a[k], b[k]) for k in ("packed", "action", "visits")) and \
        all(int(a[k]) == int(b[k]) for k in ("n_child", "colour", "chosen", "game_over", "result"))


# ------------------------------------------------------------------------------------------------ 1. the scalar rule
TRIPLES = (PR.ALPHAZERO, PR.A, PR.B_, Cpuct(1.745, 38739.0, 3.894, 2.0, 1.0, 100.0), Cpuct(0.0, 1e9, 0.5, 100.0, 3.0, 0.001))


def _ulp_distance(a, b):
    key = lambda x: (lambda i: i if i >= 0 else -(i & 0x7FFFFFFF))(int(np.float32(x).view(np.int32)))
    return abs(key(a) - key(b))


def test_c_of_is_within_one_f32_ulp_of_math_log():
    """sz_slog's f64 error is nine orders of magnitude below f32's half-ulp: the two differ only where the exact value sits on a rounding boundary"""
    rng = np.random.default_rng(5)
    ns = list(range(1, 301)) + [2 ** k for k in range(0, 31)] + [int(x) for x in 2.0 ** rng.uniform(0.0, 31.0, size=2000)]
    worst = n_cases = n_off = 0
    for o in TRIPLES:
        for root in (False, True):
            init, base, factor = (float(np.float32(x)) for x in PR.site(o, root))
            for n in ns:
                got = PR.c_of(o, n, root)
                want = np.float32(init + factor * math.log(((float(n) + base) + 1.0) / base))
                d = _ulp_distance(got, want)
                worst, n_cases, n_off = max(worst, d), n_cases + 1, n_off + (d > 0)
                assert got.dtype == np.float32 and d <= 1, (o, root, n, got, want)
    print("c_of against math.log: %d cases, %d differ, by at most %d f32 ulp" % (n_cases, n_off, worst))
    assert n_cases >= 20000
    # the growth the option is there for: AlphaZero's schedule at 800 and at 19652 + 19651 visits (x = 2: init + ln 2)
    assert 1.25 < float(PR.c_of(PR.ALPHAZERO, 0, True)) < 1.2502 and abs(float(PR.c_of(PR.ALPHAZERO, 800, True)) - (1.25 + math.log(20453 / 19652))) < 1e-6
    assert PR.c_of(PR.ALPHAZERO, 19651, False) == np.float32(1.25 + math.log(2.0))


def test_factor_0_gives_init_exactly():
    for init in (0.0, 1.25, 2.0, 100.0, float(np.float32(0.1)), 1e-30):
        for base in (1.0, 7.0, 19652.0, 1e9):
            o = Cpuct(init, base, 0.0, init, base, 0.0)
            for n in (0, 1, 63, 800, 2 ** 20, 2 ** 31 - 1):
                for root in (False, True):
                    assert PR.c_of(o, n, root).tobytes() == np.float32(init).tobytes(), (init, base, n)


PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "sz_cpuct.h"
struct Opts { float v[6]; };
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n <= 0) return 3;
    int* n_p = (int*)malloc(4 * (size_t)n); unsigned char* root = (unsigned char*)malloc(n); Opts* o = (Opts*)malloc(sizeof(Opts) * (size_t)n);
    float* c = (float*)malloc(4 * (size_t)n);
    if (fread(n_p, 4, n, f) != (size_t)n || fread(root, 1, n, f) != (size_t)n || fread(o, sizeof(Opts), n, f) != (size_t)n) return 4;
    fclose(f);
    for (int i = 0; i < n; i++) { const float* t = o[i].v + (root[i] ? 3 : 0); c[i] = sz_cpuct(t[0], t[1], t[2], n_p[i]); }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(c, 4, n, f) != (size_t)n) return 5;
    fclose(f);
    return 0;
}
"""


def test_host_compilation_of_the_header_equals_c_of_bit_for_bit(tmp_path):
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "a host C++ compiler is needed"
    assert os.path.exists(os.path.join(CSRC, "sz_cpuct.h")), "csrc/sz_cpuct.h: the rule's scalar function"
    hc = PR.hook_cases()
    n = len(hc.n_p)
    assert n >= 10000 and hc.opts.dtype.itemsize == 24 and {0, 1} == set(hc.is_root.tolist()) and int(hc.n_p.max()) == 2 ** 31 - 1
    src, exe, fin, fout = (str(tmp_path / x) for x in ("cpuct_host.cpp", "cpuct_host", "cases.bin", "c.bin"))
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([gxx, "-O2", "-ffp-contract=off", "-std=c++17", "-I", CSRC, src, "-o", exe])
    with open(fin, "wb") as f:
        f.write(np.int32(n).tobytes() + hc.n_p.tobytes() + hc.is_root.tobytes() + hc.opts.tobytes())
    subprocess.check_call([exe, fin, fout])
    got = np.fromfile(fout, np.float32)
    want = PR.hook_reference(hc)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(got) == n and not len(bad), "case %d (n_p %d, root %d, %s): host %r, restatement %r (%d differ)" % (
        bad[0], hc.n_p[bad[0]], hc.is_root[bad[0]], hc.opts[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    assert len(set(want.tolist())) > 5000, "the cases are not a handful of values"


# ------------------------------------------------------------------------------------------------ 2. whole searches
@pytest.mark.parametrize("name", ["L4_solver_reuse", "forced_fpu_endings_noise"])
def test_factor_0_is_fullref_with_c_equal_to_init(name):
    cfg = next(c for c in PR.configs() if c.name == name)
    C = 1.5
    games, recs = _play(name, cpuct=Cpuct(C, 5.0, 0.0, C, 11.0, 0.0), c=2.0)       # the games' own constant, 2, is never read
    plain, precs = _play(name, cpuct=None, c=C)
    other, _ = _play(name, cpuct=None, c=2.0)
    n_cmp = 0
    for ply, (ra, rb) in enumerate(zip(recs, precs)):
        assert all(_same_record(a, b) for a, b in zip(ra, rb)), "ply %d: records" % ply
    for g, p in zip(games, plain):
        assert g.starts == p.starts and g.chosen == p.chosen and len(g.searches) == len(p.searches)
        assert (g.forced_selections, g.pruned_visits, g.ended) == (p.forced_selections, p.pruned_visits, p.ended)
        for sa, sb in zip(g.searches, p.searches):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(sa.tree(), sb.tree())), "%s: trees" % name
            assert len(sa.steps) == len(sb.steps) and all(np.array_equal(x, y) for x, y in zip(sa.steps, sb.steps)), "%s: network input rows" % name
            n_cmp += 1
        assert all(type(s) is PR.Search for s in g.searches) and not any(type(s) is PR.Search for s in p.searches), "through the option's own selection"
    assert n_cmp >= 3 * len(cfg.boards)
    assert [g.chosen for g in plain] != [g.chosen for g in other], "c = 1.5 and c = 2 do not play the same games: the comparison says something"


def test_option_off_is_fullref():
    cfg = next(c for c in PR.configs() if c.name == "forced_fpu_endings_noise")
    games, recs = _play(cfg.name, cpuct=None)
    gam = PR.gammas(cfg)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for b, (bd, g) in enumerate(zip(cfg.boards, games)):
            ref = FU.Game(bd.make(), cfg.S, None, reuse=False, L=1, lam=1.0, solver=False, c=2.0, learning=True, mode=bd.mode, salt=bd.salt, fpu=cfg.fpu)
            ref.set_endings(FU.ER.options(**cfg.endings), False)
            for ply in range(cfg.plies):
                if not ref.live:
                    break
                ref.set_root_noise(True)
                ref.begin(None, gam[ply][b], False, cfg.forced_k)
                ref.run()
                assert _same_record(ref.play(bd.u(ply)), recs[ply][b]), (b, ply)
            assert ref.chosen == g.chosen and all(x.tobytes() == y.tobytes() for sa, sb in zip(ref.searches, g.searches) for x, y in zip(sa.tree(), sb.tree()))


def test_configurations_reach_what_they_are_there_for():
    cfgs = PR.configs()
    assert [c.name for c in cfgs] == ["plain", "L4_solver_reuse", "forced_fpu_endings_noise", "visit_targets_playout_cap", "temperature", "reuse_kept_root"]
    played = [_play(c.name)[0] for c in cfgs]
    cov = PR.coverage(played)
    print("coverage:", {k: cov[k] for k in PR.COVERAGE})
    PR.assert_coverage(cov)
    by = {c.name: PR.coverage([g]) for c, g in zip(cfgs, played)}
    assert by["L4_solver_reuse"]["cpuct_parent_in_flight"] > 0 and by["reuse_kept_root"]["cpuct_kept_root_above_num_searches"] > 0
    assert by["forced_fpu_endings_noise"]["cpuct_changed_pruning"] > 0
    assert sum(g.pruned_visits for g in played[2]) > 0 and sum(g.forced_selections for g in played[2]) > 0
    print({c.name: (by[c.name]["cpuct_changed_root"], by[c.name]["cpuct_changed_tree"]) for c in cfgs})
    assert all(by[c.name]["cpuct_changed_root"] > 0 for c in cfgs), "every configuration: the rate decides selections"
    assert any(s == "reused" for g in played[3] for s in g.starts) and any(0 < x < 32 for g in played[3] for x in g.goals)
    assert sum(g.temp_stats[0] for g in played[4]) > 0
    for c, games in zip(cfgs, played):
        assert sum(len(g.searches) for g in games) >= 3 * len(c.boards), c.name
        assert all(cp is not None for g in games for cp in g.cpuct_plies)


def test_changing_the_option_keeps_the_subtree():
    games, _ = _play("visit_targets_playout_cap")
    kept = [g for g in games if g.starts[:3] == ["new", "reused", "reused"]]
    assert len(kept) >= 2 and all(g.cpuct_plies[1] != g.cpuct_plies[2] for g in kept), [g.starts for g in games]


# ------------------------------------------------------------------------------------------------ 3. the Python layer
def test_cpuct_options_of():
    f32 = lambda x: float(np.float32(x))
    assert cpuct_options_of({}) is None and cpuct_options_of({"cpuct": None}) is None
    assert cpuct_options_of({"cpuct": {"init": 1.25}}) == (1.25, 19652.0, 1.0, 1.25, 19652.0, 1.0)
    assert cpuct_options_of({"cpuct": {"init": 0.1, "base": 8, "factor": 2, "root_base": 4}}) == (f32(0.1), 8.0, 2.0, f32(0.1), 4.0, 2.0)
    assert cpuct_options_of({"cpuct": {"init": 1, "root_init": 2.5, "root_factor": 0, "base": np.float32(16)}}) == (1.0, 16.0, 1.0, 2.5, 16.0, 0.0)
    assert cpuct_options_of({"cpuct": {"init": 100, "base": 1e9, "factor": 100, "root_init": 0, "root_base": 1, "root_factor": 0}}) == (100.0, 1e9, 100.0, 0.0, 1.0, 0.0)
    nan, inf = float("nan"), float("inf")
    for bad in ([1.25], 1.25, "alphazero", {"init": 1.25, "c_base": 3}, {}, {"base": 8}):
        with pytest.raises(ValueError):
            cpuct_options_of({"cpuct": bad})
    for key, values in (("init", (True, nan, inf, -0.5, 100.5, "1", None)), ("base", (False, nan, inf, 0.5, 0, 2e9, "8")), ("factor", (True, nan, -inf, -1, 101, [1])),
                        ("root_init", (nan, -1e-3, 1e3, True)), ("root_base", (nan, 0.999, 1e10, "x")), ("root_factor", (nan, inf, -2, 100.01, False))):
        for v in values:
            with pytest.raises(ValueError, match=r"\['cpuct'\]\[%r\]" % key):
                cpuct_options_of({"cpuct": dict({"init": 1.25}, **{key: v})})
    with pytest.raises(ValueError, match="needs 'init'"):
        cpuct_options_of({"cpuct": {"factor": nan}})
    with pytest.raises(ValueError, match="gumbel"):
        cpuct_options_of({"cpuct": {"init": 1.25}, "gumbel": {"m": 4}})
    # the order of the checks: the dict and its keys, init, base, factor, root_init, root_base, root_factor, the combinations
    order = ["init", "base", "factor", "root_init", "root_base", "root_factor"]
    for i, first in enumerate(order):
        opt = {"init": 1.25}
        opt.update({k: nan for k in order[i:]})
        with pytest.raises(ValueError, match=r"\['cpuct'\]\[%r\]" % first):
            cpuct_options_of({"cpuct": opt, "gumbel": {"m": 4}})
    with pytest.raises(ValueError, match="keys from"):
        cpuct_options_of({"cpuct": {"init": nan, "nope": 1}})
    with pytest.raises(ValueError, match=r"\['cpuct'\]\['init'\]"):
        cpuct_options_of({"cpuct": {"init": nan}, "gumbel": {"m": 4}})


def test_train_rl_flags_yield_the_key():
    from sigma_zero_amd import train_rl
    flags = train_rl.flag_parser()
    assert "cpuct" not in train_rl.selfplay_args_of(flags.parse_args([]))
    a = train_rl.selfplay_args_of(flags.parse_args(["--cpuct-init", "1.25"]))
    assert a["cpuct"] == {"init": 1.25} and cpuct_options_of(a) == (1.25, 19652.0, 1.0, 1.25, 19652.0, 1.0)
    a = train_rl.selfplay_args_of(flags.parse_args(["--cpuct-init", "1.745", "--cpuct-base", "38739", "--cpuct-factor", "3.894", "--cpuct-root-init", "2.5",
                                                    "--cpuct-root-base", "100", "--cpuct-root-factor", "0"]))
    assert a["cpuct"] == {"init": 1.745, "base": 38739.0, "factor": 3.894, "root_init": 2.5, "root_base": 100.0, "root_factor": 0.0}
    assert cpuct_options_of(a) == tuple(float(np.float32(x)) for x in (1.745, 38739.0, 3.894, 2.5, 100.0, 0.0))
    with pytest.raises(ValueError, match="needs 'init'"):
        cpuct_options_of(train_rl.selfplay_args_of(flags.parse_args(["--cpuct-base", "8"])))
    with pytest.raises(ValueError, match="gumbel"):
        cpuct_options_of(train_rl.selfplay_args_of(flags.parse_args(["--cpuct-init", "1.25", "--gumbel", "8"])))
