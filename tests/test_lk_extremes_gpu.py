"""Every LK kernel at the ends of the pixel range (tests/extreme_images.py): stripes,
checkers, random 0 / 255 blocks against true shifts and against their inverse, and
a binarised scene pair. Gradients are +-4080 and the window sums pass 2^31 and
2^32 (test_extreme_images_cpu.py asserts that of these very cases, from numpy and
the oracle), so the kernels' integer arguments -- a lane's int32 partials, the
STEPS32 count, the 16-bit halves of the wave total, lk_cv's exact shortcut against
its float chains, the SAD's 2048 * 8160 < 2^24 -- are executed at their bounds.

The bar is the project's own: status, points, err and lk_last_iterations() are
bit-identical to O.lk(acc=ACC_EXACT), under LK_OPENCV_ORDER to ACC_SSE. (Not
"within 0.1 px of the SSE order": on checker 2 the two orders legitimately
differ by more than a pixel.)"""
import functools

import numpy as np
import pytest

import extreme_images as X
import oracle as O
import svo_amd as S
from svo_amd.scene import Scene

pytestmark = pytest.mark.gpu

CV = S.LK_OPENCV_ORDER
T_CRIT, S_CRIT = (3, 50, 1e-3), (3, 30, 1e-3)
# the reference's two calls (R:src/tracking.cpp:160-165, :101-105), and the same at
# max_level 0, where the CPU companion's sums are the ones the kernels form
CONFIGS = {
    "temporal21": ((21, 21), 3, T_CRIT, S.LK_GET_MIN_EIGENVALS),
    "stereo11": ((11, 11), 3, S_CRIT, 0),
    "temporal21-level0": ((21, 21), 0, T_CRIT, S.LK_GET_MIN_EIGENVALS),
    "stereo11-level0": ((11, 11), 0, S_CRIT, 0),
}
PAIRS = list(X.LK_PAIRS)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture(scope="module")
def device_pair(ctx):
    """name -> the pair's two device images (six pyramid levels), uploaded once."""
    made = {}

    def get(name):
        if name not in made:
            A, B = X.lk_pair(name)
            made[name] = (ctx.image(A, 6), ctx.image(B, 6))
        return made[name]

    return get


@pytest.fixture(params=["fixed-window", "generic", "one-per-wave"])
def lk_kernel(request, monkeypatch):
    """test_gpu_parity's: the compile-time-window kernels (lk_multi 21 / 11 four
    features per wave, lk_fast), lk_kernel (SVO_LK_GENERIC=1), and one feature per
    wave (SVO_LK_QUAD=0: lk_fast 21 / 11)."""
    monkeypatch.setenv("SVO_LK_GENERIC", "1" if request.param == "generic" else "0")
    monkeypatch.setenv("SVO_LK_QUAD", "0" if request.param == "one-per-wave" else "1")
    return request.param


@pytest.fixture(params=["four-per-wave", "one-per-wave"])
def cv_kernel(request, monkeypatch):
    """test_lk_opencv_order_gpu's: lk_cvq_kernel (21 / 11) and lk_cv_kernel."""
    monkeypatch.setenv("SVO_LK_QUAD", "1" if request.param == "four-per-wave" else "0")
    return request.param


_POINT_SETS = {}


def _register(pts):
    """Point sets by key, so that the oracle's runs can be cached on hashable arguments."""
    pts = np.ascontiguousarray(pts, np.float32)
    key = hash(pts.tobytes())
    _POINT_SETS.setdefault(key, pts)
    return key


@functools.lru_cache(maxsize=None)
def _oracle(name, pkey, win, ml, crit, flags, want_err, acc, gkey=None):
    A, B = X.lk_pair(name) if isinstance(name, str) else name()
    out = O.lk(A, B, _POINT_SETS[pkey], win, ml, crit, flags, acc=acc, want_err=want_err,
               next_pts=None if gkey is None else _POINT_SETS[gkey])
    for a in out:
        a.setflags(write=False)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(ctx, images, name, pts, win, ml, crit, flags, want_err=True, cv=False, guess=None, what=""):
    """One call on the device against the oracle: status, points, err, iterations."""
    ga, gb = images
    gn, gs, ge = ctx.calc_optical_flow_pyr_lk(ga, gb, pts, next_pts=guess, win_size=win, max_level=ml, criteria=crit,
                                              flags=flags | (CV if cv else 0), want_err=want_err)
    git = ctx.lk_last_iterations()
    rn, rs, re_, it = _oracle(name, _register(pts), win, ml, crit, flags, want_err, O.ACC_SSE if cv else O.ACC_EXACT,
                              None if guess is None else _register(guess))
    what = f"{name if isinstance(name, str) else name.__name__} {win} ml {ml} flags {flags} err {want_err} cv {cv} {what}"
    assert np.array_equal(gs, rs), f"{what}: status differs at {np.nonzero(gs != rs)[0][:10]}"
    bad = np.nonzero((_bits(gn) != _bits(rn)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} points differ, first {bad[:8]}: {gn[bad[:3]]} vs {rn[bad[:3]]}"
    if want_err:
        bad = np.nonzero(_bits(ge) != _bits(re_))[0]
        assert len(bad) == 0, f"{what}: err differs at {bad[:8]}: {ge[bad[:3]]} vs {re_[bad[:3]]}"
    else:
        assert ge is None
    assert git == int(it.sum()), f"{what}: iterations {git} vs {int(it.sum())}"
    return rs, it


# ---------------------------------------------------------------- the two product calls
@pytest.mark.parametrize("name", PAIRS)
def test_lk_exact_kernels_on_extreme_pairs(ctx, device_pair, lk_kernel, name):
    """lk_multi 21 and 11 (the latter without err), lk_fast 21 / 11 (with the SAD
    error of flags 0 + err), lk_kernel: the temporal and the stereo call, with and
    without err, on ~800 points (integer, sub-pixel, border and outside; 807 is no
    multiple of 4)."""
    pts = X.lk_points()
    tracked = 0
    for cfg in CONFIGS.values():
        for want_err in (True, False):
            rs, _ = _check(ctx, device_pair(name), name, pts, *cfg, want_err=want_err)
            tracked += int(rs.sum())
    assert tracked > 0 or name == "stripes4-shift1"  # (the plain stripes: every feature rejected)


@pytest.mark.parametrize("name", PAIRS)
def test_lk_opencv_order_kernels_on_extreme_pairs(ctx, device_pair, cv_kernel, name):
    """lk_cvq_kernel and lk_cv_kernel against ACC_SSE: the sums are far above 2^24, so
    the ordered float chains run (not the exact shortcut), and the per-lane cap of
    the bound keeps 64 lanes' |terms| from overflowing."""
    pts = X.lk_points()
    for cfg in CONFIGS.values():
        for want_err in (True, False):
            _check(ctx, device_pair(name), name, pts, *cfg, want_err=want_err, cv=True)


def test_lk_orders_differ_on_checker(ctx, device_pair):
    """Not vacuous: on checker 2 the exact and OpenCV's order stop elsewhere."""
    pts = X.lk_points()
    cfg = CONFIGS["temporal21"]
    ex = _oracle("checker2-shift1", _register(pts), *cfg, True, O.ACC_EXACT)
    sse = _oracle("checker2-shift1", _register(pts), *cfg, True, O.ACC_SSE)
    assert (_bits(ex[0]) != _bits(sse[0])).any()


# ---------------------------------------------------------------- lk_fast's other windows
@pytest.mark.parametrize("win", [(15, 15), (31, 31)], ids=str)
@pytest.mark.parametrize("name", PAIRS)
def test_lk_fast_15_and_31(ctx, device_pair, name, win):
    """lk_fast_kernel's 15 x 15 and 31 x 31 (31 x 31 sums pass 2^32), flags 0 (SAD
    error) and MIN_EIGENVALS, four levels and level 0 alone; and lk_cv_kernel, the
    OpenCV-order kernel of these windows."""
    pts = X.lk_points()
    for ml in (3, 0):
        for flags in (0, S.LK_GET_MIN_EIGENVALS):
            _check(ctx, device_pair(name), name, pts, win, ml, S_CRIT, flags)
            _check(ctx, device_pair(name), name, pts, win, ml, S_CRIT, flags, cv=True)


# ---------------------------------------------------------------- small counts: lk_multi's partial waves
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("name", ["blocks2-shift(1,1)", "stripes4-speckled-shift1", "checker2-shift1"])
def test_lk_small_counts(ctx, device_pair, name, n):
    """n = 1 and counts that are no multiple of 4: a wave of lk_multi / lk_cvq holds
    fewer than four features, and the single-group tail sees saturated sums."""
    allp = X.lk_points()
    for first in (0, 37, X.N_INT + 11):  # integer and sub-pixel features
        pts = allp[first:first + n]
        for cfg in CONFIGS.values():
            for want_err in (True, False):
                for cv in (False, True):
                    _check(ctx, device_pair(name), name, pts, *cfg, want_err=want_err, cv=cv, what=f"n {n} from {first}")


# ---------------------------------------------------------------- initial flow
def test_lk_initial_flow_one_pixel_off(ctx, device_pair, lk_kernel):
    name = "blocks2-shift(1,1)"
    pts = X.lk_points()
    guess = (pts + np.float32([2.0, 1.0])).astype(np.float32)  # the true shift is (1, 1)
    for win, ml, crit, flags in CONFIGS.values():
        for cv in (False, True):
            _check(ctx, device_pair(name), name, pts, win, ml, crit, flags | S.LK_USE_INITIAL_FLOW, guess=guess, cv=cv)


# ---------------------------------------------------------------- windows above 31 x 31
WINDOWS_ABOVE_31 = [(33, 33), (41, 41), (42, 42), (45, 45), (58, 35), (32, 64), (3, 64)]


def _scene_pair():
    sc = Scene(X.LK_W, X.LK_H, seed=4)
    return sc.frame(0), sc.frame(1)


def _window_points(win, seed=0):
    """Inside, and near and beyond all four borders as far as the window reaches
    (OpenCV's bounds test admits a window whose top-left pixel is win px outside:
    wider than the 32-px stored border, so only the REFLECT_101 staging protects
    these reads)."""
    w, h = X.LK_W, X.LK_H
    ww, wh = win
    rng = np.random.default_rng(seed + 100 * ww + wh)
    rx, ry = 1.6 * ww + 3, 1.6 * wh + 3
    k = 40
    pts = np.concatenate([
        np.c_[rng.uniform(0, w, 120), rng.uniform(0, h, 120)],
        X.half_points(w, h, 40, seed + 1),
        np.c_[rng.uniform(-rx, rx / 2, k), rng.uniform(-ry, h + ry, k)],
        np.c_[rng.uniform(w - rx / 2, w + rx, k), rng.uniform(-ry, h + ry, k)],
        np.c_[rng.uniform(-rx, w + rx, k), rng.uniform(-ry, ry / 2, k)],
        np.c_[rng.uniform(-rx, w + rx, k), rng.uniform(h - ry / 2, h + ry, k)],
        np.array([[0, 0], [w - 1, h - 1], [-(ww + 1) / 2, 5], [5, -(wh + 1) / 2], [-(ww + 1) / 2 - 1, 5],
                  [w + (ww - 1) / 2 - 0.1, h / 2], [w / 2, h + (wh - 1) / 2 - 0.5], [w + (ww - 1) / 2, h / 2]]),
    ]).astype(np.float32)
    return pts


def _levels_for_window(w, h, win, max_level):
    return O.pyr_levels(w, h, win, max_level)[0]


@pytest.fixture(scope="module")
def scene_images(ctx):
    A, B = _scene_pair()
    return ctx.image(A, 6), ctx.image(B, 6)


@pytest.mark.parametrize("order", ["exact", "opencv"])
@pytest.mark.parametrize("win", WINDOWS_ABOVE_31, ids=str)
def test_lk_windows_above_31(ctx, device_pair, scene_images, win, order):
    """lk_kernel and lk_cv_kernel (the only kernels of these windows) with strips of
    up to 64 rows, on a scene pair and on blocks 2, flags 0 (SAD) and MIN_EIGENVALS.
    lk_kernel's four waves need 4 * lds_wave bytes of LDS: more than 64 KiB from
    42 x 42 upwards (DESIGN.md says what the runtime made of that launch)."""
    assert S.PYR_PAD == 32 and max(win) > S.PYR_PAD - 1
    assert _levels_for_window(X.LK_W, X.LK_H, win, 3) + 1 <= 7  # the images hold 7 levels
    pts = _window_points(win)
    cv = order == "opencv"
    tracked = 0
    for flags in (0, S.LK_GET_MIN_EIGENVALS):
        rs, it = _check(ctx, scene_images, _scene_pair, pts, win, 3, S_CRIT, flags, cv=cv)
        tracked += int(rs.sum())
        rs, it = _check(ctx, device_pair("blocks2-shift(1,1)"), "blocks2-shift(1,1)", pts, win, 3, S_CRIT, flags, cv=cv)
        tracked += int(rs.sum())
    assert tracked > 400


@pytest.mark.parametrize("order", ["exact", "opencv"])
def test_lk_tall_thin_window(ctx, device_pair, scene_images, order):
    """(3, 682): 21 strips of 33 rows, the tallest strip a window of at most 32
    columns can have (lk_kernel<48> with idle rows; 132 096 B of LDS for four
    waves). Taller than the image: every window hangs over its top and bottom, so
    all of it is REFLECT_101 staging and zero-padded derivatives; level 0 only."""
    win = (3, 682)
    assert _levels_for_window(X.LK_W, X.LK_H, win, 3) == 0
    pts = _window_points(win)
    tracked = 0
    for flags in (0, S.LK_GET_MIN_EIGENVALS):
        rs, _ = _check(ctx, scene_images, _scene_pair, pts, win, 3, S_CRIT, flags, cv=order == "opencv")
        tracked += int(rs.sum())
        rs, _ = _check(ctx, device_pair("blocks2-shift(1,1)"), "blocks2-shift(1,1)", pts, win, 3, S_CRIT, flags,
                       cv=order == "opencv")
        tracked += int(rs.sum())
    assert tracked > 400


@pytest.mark.parametrize("order", ["exact", "opencv"])
def test_lk_sad_bound_32x64_inverse(ctx, device_pair, order):
    """The SAD bound: blocks 2 against its inverse, the (32, 64) window's top-left
    pixel an integer, no iteration (COUNT 0): sum |J - I| = 2048 * 8160 = 16 711 680,
    65 536 below 2^24, err = 255 exactly; and the same pair with iterations."""
    name = "blocks2-inverse"
    pts = X.half_points(X.LK_W, X.LK_H, 100, 3)
    cv = order == "opencv"
    rs, it = _check(ctx, device_pair(name), name, pts, (32, 64), 0, (S.TERM_COUNT, 0, 0.0), 0, cv=cv)
    err = _oracle(name, _register(pts), (32, 64), 0, (S.TERM_COUNT, 0, 0.0), 0, True, O.ACC_SSE if cv else O.ACC_EXACT)[2]
    assert rs.all() and not it.any() and (err == np.float32(255)).all()
    for ml in (0, 3):
        _check(ctx, device_pair(name), name, _window_points((32, 64)), (32, 64), ml, S_CRIT, 0, cv=cv)
