"""Per-board search budgets (sz_set_search_budgets / sz_compact_searching, a NON-REFERENCE option): the parts that need no GPU —
the segment computation of SelfPlayEngine.search, the C ABI declarations and their ctypes binding, and the validation of
args["playout_cap"] that happens before any engine exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sigma_zero_amd import _native as N
from sigma_zero_amd.selfplay import search_segments


# ------------------------------------------------------------------------------------------------ 1. segments
BUDGETS = [[5, 5, 64, 17, 0, 64], [2, 5, 16, 64, 1, 0, 2, 64], [3, 7, 32, 64], list(range(0, 41)), [100] * 3 + [800], [9, 10, 11, 12, 13, 14, 200]]


@pytest.mark.parametrize("budgets", BUDGETS)
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("max_shrinks", [0, 1, 4])
def test_segments(budgets, L, max_shrinks):
    segs = search_segments(budgets, L, max_shrinks)
    assert all(isinstance(n, int) and n > 0 for n in segs)
    assert sum(segs) == -(-max(budgets) // L)                       # at L = 1: max(budgets); at L > 1 the part that runs without asking the device
    ends = np.cumsum(segs).tolist()
    candidates = sorted({-(-s // L) for s in budgets if s > 0})     # a board with budget s cannot be done before step ceil(s / L)
    assert set(ends) <= set(candidates) and ends[-1] == candidates[-1]
    assert len(ends) - 1 <= max_shrinks                             # never more interior ends than shrinks allowed
    if len(candidates) - 1 <= max_shrinks:
        assert ends == candidates                                   # every distinct budget ends a segment when the cap allows
    else:
        assert len(ends) - 1 == max_shrinks                         # a shrink that drops boards always pays in rows: the cap is used up


def test_segments_choice_minimises_rows():
    """with more distinct budgets than shrinks the kept ends are the ones with the fewest network rows (brute force over all choices)"""
    import itertools
    budgets = [3, 3, 3, 4, 9, 9, 30, 31, 32, 64]
    cand = sorted(set(budgets))

    def rows(ends):
        total, lo = 0, 0
        for e in ends:
            total += (e - lo) * sum(1 for s in budgets if s > lo)
            lo = e
        return total

    for m in (1, 2, 3):
        best = min(rows(list(c) + [cand[-1]]) for c in itertools.combinations(cand[:-1], m))
        assert rows(np.cumsum(search_segments(budgets, 1, m)).tolist()) == best


def test_segments_uniform_and_unset():
    assert search_segments([64] * 6, 1, 4) == [64]
    assert search_segments([64] * 6, 4, 4) == [16]
    assert search_segments([7, 7, 0], 1, 4) == [7]
    assert search_segments(None, 1, 4, num_searches=800) == [800]
    assert search_segments(None, 7, 4, num_searches=64) == [10]
    assert search_segments([0, 0], 1, 4) == [] and search_segments(None, 1, 4, num_searches=0) == []
    with pytest.raises(ValueError):
        search_segments([4, -1], 1, 4)
    with pytest.raises(ValueError):
        search_segments([4], 0, 4)
    with pytest.raises(ValueError):
        search_segments([4], 1, -1)


# ------------------------------------------------------------------------------------------------ 2. declared, exported, bound
def test_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "sigmazero.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int sz_set_search_budgets(sz_engine* e, const int32_t* budgets, void* stream);" in flat
    assert "int sz_compact_searching(sz_engine* e, void* planes_dev, int32_t* n_live_out, void* stream);" in flat
    assert N.EXPORTS["sz_set_search_budgets"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p])
    assert N.EXPORTS["sz_compact_searching"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p])
    lib = N.lib()
    for name in ("sz_set_search_budgets", "sz_compact_searching"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == N.EXPORTS[name][1]
    # no engine, no device: the argument check comes first
    assert lib.sz_set_search_budgets(None, None, None) == N.SZ_ERR_INVALID
    assert lib.sz_compact_searching(None, None, None, None) == N.SZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 3. validation before any engine exists
@pytest.mark.parametrize("cap", [{"fast": 1, "p_full": 0.25}, {"fast": 0, "p_full": 0.25}, {"fast": 17, "p_full": 0.25}, {"fast": 4, "p_full": -0.01},
                                 {"fast": 4, "p_full": 1.01}, {"fast": 4, "p_full": float("nan")}, {"fast": 4.5, "p_full": 0.5}, {"fast": 4}, "fast"])
def test_playout_cap_validation(cap, monkeypatch):
    from sigma_zero_amd import sim

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before args['playout_cap'] was checked")

    monkeypatch.setattr(sim, "SelfPlayEngine", no_engine)
    with pytest.raises(ValueError):
        sim.play_games(None, {"C": 2, "num_searches": 16, "playout_cap": cap}, 2)


def test_playout_cap_accepted_values_and_exclusions():
    from sigma_zero_amd import sim
    assert sim.playout_cap_of({"num_searches": 16}) is None
    assert sim.playout_cap_of({"num_searches": 16, "playout_cap": {"fast": 2, "p_full": 0}}) == (2, 0.0)
    assert sim.playout_cap_of({"num_searches": 16, "playout_cap": {"fast": 16, "p_full": 1}}) == (16, 1.0)
    with pytest.raises(ValueError):
        sim.playout_cap_of({"num_searches": 16, "reuse_subtree": True, "playout_cap": {"fast": 4, "p_full": 0.25}})
    with pytest.raises(ValueError):
        sim.play_games(None, {"C": 2, "num_searches": 16}, 2, full_search=lambda g, p: True)       # the callable without the option
