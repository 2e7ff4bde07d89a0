"""LKBatch::first: a launch over the points [first, n) of a sequence. Through
svo_calc_optical_flow_pyr_lk_split, which tracks [0, k) and [k, n) in two launches,
against the one launch over [0, n): bit for bit, whichever points share a wave or
a block -- for the two product windows and every kernel family behind launch_lk."""
import numpy as np
import pytest

import oracle as O
import svo_amd as S
from svo_amd.scene import Scene

pytestmark = pytest.mark.gpu

W, H, N = 320, 240, 23  # 23 points: six waves of four, the last one short; six blocks of four waves
CALLS = {
    21: dict(win_size=(21, 21), max_level=3, criteria=(3, 50, 1e-3), flags=S.LK_GET_MIN_EIGENVALS),  # trackFrames
    11: dict(win_size=(11, 11), max_level=3, criteria=(3, 30, 1e-3), flags=0, want_err=False),  # findLeftFeaturesInRight
}
# kernel family -> (environment, extra flags)
FAMILIES = {
    "multi": ({}, 0),
    "fast": ({"SVO_LK_QUAD": "0"}, 0),
    "generic": ({"SVO_LK_GENERIC": "1"}, 0),
    "cvq": ({}, S.LK_OPENCV_ORDER),
    "cv": ({"SVO_LK_QUAD": "0"}, S.LK_OPENCV_ORDER),
}


@pytest.fixture(scope="module")
def setup():
    ctx = S.Context(0)
    sc = Scene(W, H, seed=7)
    A, B = sc.frame(0), sc.frame(1)
    pts = O.fast(A, 20, True)[:N, :2]
    assert len(pts) == N
    return ctx, ctx.image(A, 4), ctx.image(B, 4), pts


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("win", [21, 11])
def test_two_launches_equal_one(setup, win, family, monkeypatch):
    ctx, ga, gb, pts = setup
    env, extra = FAMILIES[family]
    for k in ("SVO_LK_QUAD", "SVO_LK_GENERIC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    call = dict(CALLS[win])
    call["flags"] |= extra
    want = ctx.calc_optical_flow_pyr_lk(ga, gb, pts, **call)
    its = ctx.lk_last_iterations()
    assert want[1].sum() > N // 2 and its > 0  # most points track
    for k in (1, 3, 4, 5, N - 1):
        # the device outputs live in the context's scratch, where the last call's results
        # still stand: another call first (the images swapped, the points reversed), so
        # that a point no launch covered would show that call's result, not the wanted one
        other = ctx.calc_optical_flow_pyr_lk(gb, ga, pts[::-1], **call)
        assert not np.array_equal(other[0], want[0])
        got = ctx.calc_optical_flow_pyr_lk(ga, gb, pts, split=k, **call)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (k, "next points")
        assert np.array_equal(got[1], want[1]), (k, "status")
        if want[2] is not None:
            assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (k, "err")
        assert ctx.lk_last_iterations() == its, k
    # the ends: no split
    for k in (0, N):
        got = ctx.calc_optical_flow_pyr_lk(ga, gb, pts, split=k, **call)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


def test_split_outside_the_points_is_refused(setup):
    ctx, ga, gb, pts = setup
    for k in (-1, N + 1):
        with pytest.raises(S.SvoError):
            ctx.calc_optical_flow_pyr_lk(ga, gb, pts, split=k)
