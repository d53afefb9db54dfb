"""arena.match_stats on closed cases: the pair score, its variance over the pairs, the 95 % normal interval, the Elo map and its clip."""
import math

import pytest

from sigma_zero_amd.arena import SCORE_CLIP, Z95, elo_of, match_stats


def test_all_draws():
    s = match_stats([0] * 12)
    assert (s["wins"], s["draws"], s["losses"], s["unfinished"], s["pairs"]) == (0, 12, 0, 0, 6)
    assert s["pentanomial"] == [0, 0, 6, 0, 0]
    assert s["score"] == 0.5 and s["variance"] == 0.0 and s["score_lo"] == s["score_hi"] == 0.5
    assert s["elo"] == s["elo_lo"] == s["elo_hi"] == 0.0


def test_all_wins_are_clipped():
    s = match_stats([1] * 8)
    assert s["pentanomial"] == [0, 0, 0, 0, 4] and s["score"] == 1.0 and s["variance"] == 0.0
    clip = -400.0 * math.log10(1.0 / (1.0 - SCORE_CLIP) - 1.0)
    assert s["elo"] == s["elo_lo"] == s["elo_hi"] == pytest.approx(clip, abs=1e-9) and math.isfinite(s["elo"]) and s["elo"] > 1000
    t = match_stats([-1] * 8)
    assert t["score"] == 0.0 and t["elo"] == pytest.approx(-clip, abs=1e-9) and t["pentanomial"] == [4, 0, 0, 0, 0]
    assert elo_of(0.0) == elo_of(SCORE_CLIP) and elo_of(1.0) == elo_of(1.0 - SCORE_CLIP)


def test_three_pairs_by_hand():
    """pairs (win, draw), (draw, loss), (win, win): pair scores 3/4, 1/4, 1.  s = 2/3; deviations 1/12, -5/12, 1/3: squares 1/144, 25/144,
    16/144, variance 42/144/3 = 7/72; half width Z95 * sqrt(7/216)"""
    s = match_stats([1, 0, 0, -1, 1, 1])
    assert (s["wins"], s["draws"], s["losses"], s["pairs"]) == (3, 2, 1, 3) and s["pentanomial"] == [0, 1, 0, 1, 1]
    assert s["score"] == pytest.approx(2.0 / 3.0, abs=1e-12)
    assert s["variance"] == pytest.approx(7.0 / 72.0, abs=1e-12)
    half = Z95 * math.sqrt(7.0 / 216.0)
    assert s["score_lo"] == pytest.approx(2.0 / 3.0 - half, abs=1e-12) and s["score_hi"] == 1.0          # cut at 1
    assert s["elo"] == pytest.approx(400.0 * math.log10(2.0), abs=1e-12)
    assert s["elo_lo"] == pytest.approx(-400.0 * math.log10(1.0 / (2.0 / 3.0 - half) - 1.0), abs=1e-12)
    assert s["elo_hi"] == pytest.approx(elo_of(1.0), abs=1e-12)


def test_the_interval_shrinks_with_more_identical_pairs():
    block = [1, 0, 0, 0, 0, -1, 1, -1]                    # pair scores 3/4, 1/2, 1/4, 1/2
    widths = []
    for k in (1, 4, 16):
        s = match_stats(block * k)
        assert s["score"] == pytest.approx(0.5, abs=1e-12) and s["variance"] == pytest.approx(1.0 / 32.0, abs=1e-12)
        widths.append(s["score_hi"] - s["score_lo"])
        assert s["elo_lo"] < s["elo"] == 0.0 < s["elo_hi"]
    assert widths[0] == pytest.approx(2 * widths[1], rel=1e-12) and widths[1] == pytest.approx(2 * widths[2], rel=1e-12)


def test_unfinished_games_leave_their_pair_out():
    s = match_stats([1, 2, 0, 0])
    assert s["unfinished"] == 1 and s["pairs"] == 1 and s["pentanomial"] == [0, 0, 1, 0, 0] and s["wins"] == 1
    e = match_stats([2, 2])
    assert e["pairs"] == 0 and e["score"] is None and e["elo"] is None
    with pytest.raises(ValueError):
        match_stats([1, 0, 1])
    with pytest.raises(ValueError):
        match_stats([3, 0])
