"""The temporal LK kernel's strip map (svo_amd/csrc/lk_strip_map.hpp): a lane's
strips 0, 1, 2 are three neighbouring window columns read by one wide load per
row, its strip 3 a single column. Any strip assignment must reproduce the
oracle's exact integer sums bit for bit -- points, status, err and iteration
counts -- and the wide loads must stay inside the padded levels wherever a
window may lie: on images smaller than the window at the coarse levels, at odd
sizes and pitches, with windows on and over every border, with part-filled and
idle groups, and through the single-group tail, which reads the same map.

Every case is the temporal call (21 x 21, maxLevel 3, (3, 50, 1e-3),
LK_GET_MIN_EIGENVALS) against O.lk(..., acc=O.ACC_EXACT)."""
import numpy as np
import pytest

import oracle as O
import svo_amd as S
from svo_amd.scene import Scene

pytestmark = pytest.mark.gpu

WIN, ML, CRIT = (21, 21), 3, (3, 50, 1e-3)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture(autouse=True)
def four_per_wave(monkeypatch):
    monkeypatch.delenv("SVO_LK_GENERIC", raising=False)
    monkeypatch.delenv("SVO_LK_QUAD", raising=False)


_frames = {}


def frames(w, h):
    """(A, B, FAST corners of A without non-maximum suppression), made once per size."""
    if (w, h) not in _frames:
        sc = Scene(w, h, seed=1)
        A, B = sc.frame(0), sc.frame(1)
        _frames[(w, h)] = (A, B, O.fast(A, 10, False)[:, :2].astype(np.float32))
    return _frames[(w, h)]


def pick(kp, n):
    """n corners spread over the whole list (it is in scan order: over the image)."""
    assert len(kp) >= n
    return kp[(np.arange(n) * len(kp)) // n]


def check(ctx, A, B, pts, guess=None):
    flags = S.LK_GET_MIN_EIGENVALS | (S.LK_USE_INITIAL_FLOW if guess is not None else 0)
    oflags = O.LK_GET_MIN_EIGENVALS | (O.LK_USE_INITIAL_FLOW if guess is not None else 0)
    ga, gb = ctx.image(A, ML + 1), ctx.image(B, ML + 1)
    gn, gs, ge = ctx.calc_optical_flow_pyr_lk(ga, gb, pts, next_pts=guess, win_size=WIN, max_level=ML, criteria=CRIT,
                                              flags=flags)
    rn, rs, re_, it = O.lk(A, B, pts, WIN, ML, CRIT, oflags, acc=O.ACC_EXACT, next_pts=guess)
    assert np.array_equal(gs, rs), f"status differs at {np.nonzero(gs != rs)[0][:10]}"
    assert np.array_equal(gn.view(np.uint32), rn.view(np.uint32)), \
        f"points differ at {np.nonzero((gn.view(np.uint32) != rn.view(np.uint32)).any(1))[0][:10]}"
    assert np.array_equal(ge.view(np.uint32), re_.view(np.uint32)), "err differs"
    assert ctx.lk_last_iterations() == int(it.sum()), "iteration count differs"
    return rs, it


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 300])
def test_small_image_part_filled_waves(ctx, n):
    """160 x 120: level 3 is 20 x 15, smaller than the window -- every coarse window
    reaches into the padding on all sides. 1, 2, 3 features leave idle groups in the
    only wave, 5 and 63 a part-filled last wave."""
    A, B, kp = frames(160, 120)
    st, _ = check(ctx, A, B, pick(kp, n))
    if n >= 63:
        assert st.sum() > 0.8 * n


@pytest.mark.parametrize("wh", [(64, 48), (161, 121)])
def test_odd_sizes_and_pitches(ctx, wh):
    """64 x 48 (level 3: 8 x 6) and 161 x 121 (odd level sizes 81 x 61, 41 x 31,
    21 x 16 and their pitches): the wide loads start at any byte address."""
    A, B, kp = frames(*wh)
    st, _ = check(ctx, A, B, pick(kp, min(len(kp), 300)))
    assert len(st) >= 50 and st.sum() > 0.8 * len(st)


def border_points(w, h):
    xs = [0, 0.5, 10, w - 11, w - 1.5, w - 1]
    ys = [0, 0.5, 10, h - 11, h - 1.5, h - 1]
    return np.array([[x, y] for y in ys for x in xs], np.float32)


@pytest.mark.parametrize("initial_flow", [False, True], ids=["no-guess", "initial-flow"])
@pytest.mark.parametrize("wh", [(64, 48), (161, 121)])
def test_windows_on_every_border(ctx, wh, initial_flow):
    """Features on, half a pixel inside and 10 px inside each border, in x and y: the
    prev window's edges touch or leave every level's border, so the rightmost and the
    bottom wide loads reach as far into the padding as they ever do. With
    USE_INITIAL_FLOW the guesses also start the next window across the borders."""
    A, B, _ = frames(*wh)
    pts = border_points(*wh)
    guess = None
    if initial_flow:
        rng = np.random.default_rng(5)
        guess = (pts + rng.uniform(-4, 4, pts.shape)).astype(np.float32)
    check(ctx, A, B, pts, guess)


def test_single_group_tail(ctx):
    """One wave: three features that do not move (done after their first iteration at
    every level) and one whose surroundings moved: it iterates on while the other
    groups are finished, which hands its iterations to all 64 lanes -- the tail takes
    its strip offsets from the same map."""
    A, _, kp = frames(160, 120)
    inside = kp[(kp[:, 0] > 46) & (kp[:, 0] < 60) & (kp[:, 1] > 44) & (kp[:, 1] < 76)]
    assert len(inside) >= 1
    mover = inside[0]
    x, y = int(mover[0]), int(mover[1])
    B = A.copy()
    B[y - 40:y + 41, x - 40:x + 41] = A[y - 44:y + 37, x - 46:x + 35]  # content moved by (+6, +4)
    still = kp[kp[:, 0] > x + 92]  # windows clear of the moved patch at levels 0 .. 2
    pts = np.concatenate([pick(still, 3), mover[None]]).astype(np.float32)
    _, it = check(ctx, A, B, pts)
    assert it[3] >= it[:3].max() + 4, f"the mover must iterate on alone: {it}"
