"""Guided row SAD and the tracked features' stereo columns on the CPU: the numpy
restatement (tests/stereo_track_reference.py) alone, on a periodic texture and in
the oracle loops. No GPU."""
import numpy as np
import pytest

from stereo_rows_reference import match_rows
from stereo_track_reference import NO_PRIOR, guided_range, match_rows_guided, row_priors, tracked_trace


def periodic_pair(w=160, h=48, period=12, d=30, seed=2):
    """Columns of a sine of `period` px; independent +-2 noise in each image; R[y][x] = L[y][x + d]."""
    rng = np.random.default_rng(seed)
    col = np.rint(128 + 100 * np.sin(2 * np.pi * np.arange(w + d) / period))
    base = np.tile(col, (h, 1))
    L = base[:, :w] + rng.integers(-2, 3, (h, w))
    R = base[:, d:d + w] + rng.integers(-2, 3, (h, w))
    return L.astype(np.uint8), R.astype(np.uint8)


def test_a_prior_picks_the_period_the_full_range_cannot():
    L, R = periodic_pair()
    p = np.array([[100.0, 24.0]], np.float32)
    _, st, disp, _ = match_rows(L, R, p)
    assert st[0] == 0 or disp[0] != 30, "the full range: rejected on uniqueness, or another period"
    for prior in (28, 30, 32):
        nx, st, disp, cost = match_rows_guided(L, R, p, [prior], 4)
        assert st[0] == 1 and disp[0] == 30, prior
        assert abs(float(p[0, 0] - nx[0, 0]) - 30) <= 0.5 and nx[0, 1] == p[0, 1]
    # a wrong prior: at x = 41 the image leaves [36, 41] of 40 +- 4, the period at 42 lies
    # outside, the costs fall towards it and the minimum is the last candidate
    q = np.array([[41.0, 24.0]], np.float32)
    nx, st, disp, cost = match_rows_guided(L, R, q, [40], 4)
    assert st[0] == 0 and disp[0] == 0 and cost[0] == 0 and np.array_equal(nx, q)
    # (without the uniqueness and cost tests only "no bracket" rejects: it is the end)
    assert match_rows_guided(L, R, q, [40], 4, uniq_pct=0)[1][0] == 0
    assert match_rows_guided(L, R, q, [30], 4)[2][0] == 30  # the same point with the right prior


def test_guided_ranges_and_equivalences():
    assert guided_range(-1, 128, NO_PRIOR, 4) == (-1, 128)
    assert guided_range(-1, 128, 30, 4) == (26, 34)
    assert guided_range(-1, 128, 0, 4) == (-1, 4) and guided_range(-1, 128, 127, 4) == (123, 128)
    assert guided_range(-1, 128, 2 ** 31 - 1, 15)[0] > 128 and guided_range(-1, 128, -(2 ** 31) + 1, 15)[1] < -1
    L, R = periodic_pair()
    pts = np.array([[100.0, 24.0], [41.0, 24.0], [70.5, 10.0]], np.float32)
    want = match_rows(L, R, pts)
    for got in (match_rows_guided(L, R, pts, None, 4), match_rows_guided(L, R, pts, [30, 40, 30], 0),
                match_rows_guided(L, R, pts, [NO_PRIOR] * 3, 4)):
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # fewer than 3 candidates: priors at and past the ends of the range
    _, st, _, _ = match_rows_guided(L, R, pts, [133, -6, 2 ** 31 - 1], 4)
    assert not st.any()
    with pytest.raises(ValueError):
        match_rows_guided(L, R, pts, [30, 30, 30], 16)


def test_row_priors_rule():
    prev_mid = np.array([2, 5, 9, 11])
    prev_xy = np.array([[50.5, 1], [40.25, 2], [10, 3], [np.inf, 4]], np.float32)
    prev_ur = np.array([48.0, -1.0, 12.5, 3.0], np.float32)  # 2.5 -> 2 (even); -1: none; -2.5 -> -2; inf
    got = row_priors([1, 2, 3, 5, 9, 11, 12], prev_mid, prev_xy, prev_ur)
    assert list(got) == [NO_PRIOR, 2, NO_PRIOR, NO_PRIOR, -2, NO_PRIOR, NO_PRIOR]
    assert list(row_priors([2], prev_mid[:0], prev_xy[:0], prev_ur[:0])) == [NO_PRIOR]
    assert list(row_priors([2], [2], [[3.5, 0]], [0.0])) == [4] and list(row_priors([2], [2], [[4.5, 0]], [0.0])) == [4]
    assert list(row_priors([2], [2], [[40000.0, 0]], [0.0])) == [NO_PRIOR]


LOOPS = [("wide", 3), ("forward", 3), ("forward", 8)]


@pytest.mark.parametrize("kind,seed", LOOPS)
def test_the_loops_give_nearly_every_tracked_feature_a_column(kind, seed):
    tr = tracked_trace(kind, seed)
    share, differ = [], 0
    for t, s in enumerate(tr[1:], 1):
        assert s.tracked > 100
        got = s.ur[: s.tracked]
        assert s.matched == int(np.sum(got >= 0))
        share.append(s.matched / s.tracked)
        differ += int(np.sum(got.view(np.uint32) != s.full_ur.view(np.uint32)))
        both = (got >= 0) & (s.full_ur >= 0)
        assert np.array_equal(got[both], s.full_ur[both]), "where both succeed they agree"
    print(f"{kind} seed {seed}: tracked {[s.tracked for s in tr[1:]]}, matched {[s.matched for s in tr[1:]]}, "
          f"priors {[s.priors for s in tr[1:]]}, differ from the full range {differ}")
    assert min(share) >= 0.90, share
    if kind == "forward":
        assert differ >= 1, "guide 4 and guide 0 are told apart"
