"""svo_stereo_match_rows on the device against the numpy restatement
(tests/stereo_rows_reference.py): next_xy, status, disparity and cost bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import svo_amd as S
from stereo_rows_reference import KITTI_BF, match_rows
from svo_amd.scene import STEREO_BF, Scene

pytestmark = pytest.mark.gpu

_f32p, _u8p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _pair(wide, w, shift, rng):
    """L and R with R[y][x] = L[y][x + shift] (the disparity `shift`, either sign) + noise of +-2."""
    off = max(-shift, 0)
    h = wide.shape[0]
    L = np.ascontiguousarray(wide[:, off: off + w])
    R = wide[:, off + shift: off + shift + w].astype(np.int16) + rng.integers(-2, 3, (h, w))
    return L, np.clip(R, 0, 255).astype(np.uint8)


def random_pair(w, h, seed, shift=9):
    rng = np.random.default_rng(seed)
    return _pair(rng.integers(0, 256, (h, w + abs(shift)), dtype=np.uint8), w, shift, rng)


def blocky_pair(w, h, seed, shift=9, cell=6):
    """cell x cell blocks: costs that fall off over a few disparities, ties and
    near-ties, so uniqueness and the parabola have something to decide."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (h // cell + 2, (w + abs(shift)) // cell + 2), dtype=np.uint8)
    return _pair(np.kron(small, np.ones((cell, cell), np.uint8))[:h, : w + abs(shift)], w, shift, rng)


_SCENES = {}


def scene_pair(bf, size=(320, 240), seed=3):
    key = (bf, size, seed)
    if key not in _SCENES:
        sc = Scene(*size, seed)
        _SCENES[key] = (sc.frame(0), sc.right(0, bf=bf))
    return _SCENES[key]


def point_mix(w, h, seed=0, n_rand=120):
    """A grid, random sub-pixel points, every border and the pixels just inside it,
    points outside the image and half-integer coordinates (both roundings)."""
    rng = np.random.default_rng(seed)
    pts = [(x, y) for y in range(3, h, 9) for x in range(2, w, 7)]
    pts += list(zip(rng.uniform(-0.4, w - 0.6, n_rand), rng.uniform(-0.4, h - 0.6, n_rand)))
    for xi in (0, 1, 2, w - 3, w - 2, w - 1):
        for yi in (0, 1, h - 2, h - 1, h // 2):
            pts.append((xi, yi))
    for x in (w // 2, w - 1, w - 20):
        pts += [(x, 0), (x, h - 1)]
    pts += [(-1, 5), (-0.51, 5), (w, 5), (w - 0.49, 5), (5, -1), (5, h), (40, h - 0.49), (40, -0.51), (-300, -300),
            (1e9, 3), (3, -1e9), (np.nan, 4), (4, np.inf)]
    pts += [(-0.5, 10), (w - 0.5, 10), (30, -0.5), (30, h - 0.5)]  # halves that round inside / outside
    pts += [(10.5, 20.5), (11.5, 21.5), (40.5, 7.5), (41.5, 8.5), (w - 1.5, 12.5), (w - 2.5, 13.5), (0.5, 0.5),
            (1.5, 1.5), (2.5, 2.5)]
    return np.array(pts, np.float32)


def check(ctx, L, R, pts, tag="", **params):
    gl, gr = ctx.image(L, 0), ctx.image(R, 0)
    try:
        got = ctx.stereo_match_rows(gl, gr, pts, S.StereoRowsParams(**params), want_cost=True)
    finally:
        gl.close()
        gr.close()
    ref = match_rows(L, R, pts, **params)
    for name, g, r in zip(("next_xy", "status", "disparity", "cost"), got, ref):
        g, r = np.asarray(g), np.asarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, (tag, name)
        gv, rv = (g.view(np.uint32), r.view(np.uint32)) if g.dtype == np.float32 else (g, r)
        bad = np.flatnonzero((gv != rv).reshape(len(g), -1).any(axis=1)) if len(g) else []
        assert len(bad) == 0, (tag, name, len(bad), pts[bad[:5]], g[bad[:5]], r[bad[:5]])
    return ref


@pytest.mark.parametrize("r", [1, 5, 7])
@pytest.mark.parametrize("image", ["random", "blocky", "scene"])
def test_small_images_every_radius(ctx, image, r):
    if image == "scene":
        L, R = (np.ascontiguousarray(a[100:164, 60:156]) for a in scene_pair(STEREO_BF))
    else:
        L, R = (random_pair if image == "random" else blocky_pair)(96, 64, seed=11)
    pts = point_mix(96, 64)
    for uniq in (80, 0):
        nxt, st, disp, cost = check(ctx, L, R, pts, (image, r, uniq), radius=r, d_min=-1, d_max=40, uniq_pct=uniq)
        assert 0 < st.sum() < len(pts)
    assert st[np.isnan(pts).any(axis=1)].sum() == 0


@pytest.mark.parametrize("d_min", [-16, -1, 0])
@pytest.mark.parametrize("width", [3, 5, 64, 65, 130, 256])
def test_search_widths(ctx, width, d_min):
    """Searched widths at and around the wave size and the lane loop's strides, on an
    image wide enough to hold the widest search, at shifts inside each range."""
    w, h = 300, 40
    d_max = d_min + width - 1
    shift = min(d_min + width // 2, 200)
    L, R = blocky_pair(w, h, seed=width, shift=shift, cell=5)
    pts = point_mix(w, h, seed=width, n_rand=60)
    nxt, st, disp, cost = check(ctx, L, R, pts, (width, d_min), radius=5, d_min=d_min, d_max=d_max, uniq_pct=0)
    if width >= 5:
        assert st.sum() > 20 and np.median(disp[st == 1]) == shift
    check(ctx, L, R, pts[::3], (width, d_min, "r7"), radius=7, d_min=d_min, d_max=d_max, uniq_pct=60)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_point_counts(ctx, n):
    L, R = scene_pair(STEREO_BF)
    kp = O.fast(L, 20, True)[:, :2]
    assert len(kp) >= 300
    nxt, st, disp, cost = check(ctx, L, R, kp[:n], n)
    assert len(st) == n and (n < 63 or st.sum() > n // 2)


def test_constant_image_matches_nothing(ctx):
    Cst = np.full((64, 96), 93, np.uint8)
    pts = point_mix(96, 64)
    for uniq in (80, 0):
        nxt, st, disp, cost = check(ctx, Cst, Cst, pts, uniq_pct=uniq)
        assert st.sum() == 0 and not disp.any() and not cost.any()
        assert np.array_equal(nxt.view(np.uint32), pts.view(np.uint32))


def test_periodic_texture_is_ambiguous(ctx):
    """Columns of period 8: the same cost every 8 disparities. Uniqueness rejects every
    match; with uniq_pct = 0 the lowest disparity of the equals is accepted."""
    h, w, shift = 64, 96, 3
    col = np.array([10, 60, 200, 140, 90, 250, 30, 170], np.uint8)
    wide = np.tile(col, (h, (w + shift) // 8 + 1))
    wide = (wide.astype(np.int16) + (np.arange(h)[:, None] * 37 % 50)).astype(np.uint8)
    L, R = np.ascontiguousarray(wide[:, :w]), np.ascontiguousarray(wide[:, shift: shift + w])
    pts = np.array([(x, y) for y in range(8, h - 8, 6) for x in range(40, w - 8, 5)], np.float32)
    _, st, _, _ = check(ctx, L, R, pts, "uniq", d_min=-1, d_max=30, uniq_pct=80)
    assert st.sum() == 0
    _, st, disp, cost = check(ctx, L, R, pts, "off", d_min=-1, d_max=30, uniq_pct=0)
    assert st.all() and np.all(disp == shift) and not cost.any()


def test_max_cost(ctx):
    L, R = scene_pair(STEREO_BF)
    kp = O.fast(L, 20, True)[:, :2]
    _, st0, _, c0 = check(ctx, L, R, kp, "off", max_cost=0)
    cut = int(np.median(c0[st0 == 1]))
    _, st1, _, c1 = check(ctx, L, R, kp, "on", max_cost=cut)
    assert 0 < st1.sum() < st0.sum() and c1.max() <= cut
    assert np.array_equal(st1 == 1, (st0 == 1) & (c0 <= cut))


@pytest.mark.parametrize("bf", [KITTI_BF, STEREO_BF])
def test_scene_pair(ctx, bf):
    L, R = scene_pair(bf)
    sc = Scene(320, 240, 3)
    kp = np.ascontiguousarray(O.fast(L, 20, True)[:, :2], np.float32)
    nxt, st, disp, cost = check(ctx, L, R, kp, bf)
    truth = bf / sc.map_points(kp, 0)[:, 2]
    good = (st == 1) & (np.abs(kp[:, 0] - nxt[:, 0] - truth) <= 1)
    assert good.sum() > 0.75 * len(kp)


BAD_PARAMS = [dict(radius=0), dict(radius=8), dict(d_min=-17), dict(d_max=256), dict(d_min=0, d_max=1),
              dict(d_min=5, d_max=4), dict(d_min=-16, d_max=240), dict(uniq_pct=-1), dict(uniq_pct=101),
              dict(max_cost=-1)]


def test_bad_arguments_write_nothing(ctx):
    L, R = random_pair(96, 64, seed=2)
    gl, gr, gs = ctx.image(L, 0), ctx.image(R, 0), ctx.image(L[:, :90], 0)
    pts = point_mix(96, 64)[:40]
    n = len(pts)
    fn = S.lib().svo_stereo_match_rows

    def call(left, right, p, n_, par, want=(True, True, True, True)):
        nxt = np.full((n, 2), 7.25, np.float32)
        st = np.full(n, 9, np.uint8)
        disp = np.full(n, -5, np.int32)
        cost = np.full(n, -6, np.int32)
        rc = fn(ctx.handle, left, right, None if p is None else p.ctypes.data_as(_f32p), n_,
                None if par is None else C.byref(par), nxt.ctypes.data_as(_f32p) if want[0] else None,
                st.ctypes.data_as(_u8p) if want[1] else None, disp.ctypes.data_as(_i32p) if want[2] else None,
                cost.ctypes.data_as(_i32p) if want[3] else None)
        untouched = np.all(nxt == 7.25) and np.all(st == 9) and np.all(disp == -5) and np.all(cost == -6)
        return rc, untouched, (nxt, st, disp, cost)

    ok = S.StereoRowsParams()
    for bad in BAD_PARAMS:
        rc, untouched, _ = call(gl.handle, gr.handle, pts, n, S.StereoRowsParams(**bad))
        assert rc == -1 and untouched, bad
        with pytest.raises(S.SvoError):
            ctx.stereo_match_rows(gl, gr, pts, S.StereoRowsParams(**bad))
    for args in ((None, gr.handle, pts, n, ok), (gl.handle, None, pts, n, ok), (gl.handle, gr.handle, None, n, ok),
                 (gl.handle, gr.handle, pts, n, None), (gl.handle, gr.handle, pts, -1, ok),
                 (gl.handle, gs.handle, pts, n, ok)):
        rc, untouched, _ = call(*args)
        assert rc == -1 and untouched, args[3:]
    for want in ((False, True, True, True), (True, False, True, True)):
        rc, untouched, _ = call(gl.handle, gr.handle, pts, n, ok, want)
        assert rc == -1 and untouched, want
    assert fn(None, gl.handle, gr.handle, pts.ctypes.data_as(_f32p), n, C.byref(ok), None, None, None, None) == -1
    # the boundary values are accepted; n = 0 is valid and writes nothing; disparity / cost are optional
    for good in (dict(radius=1), dict(radius=7), dict(d_min=-16, d_max=239), dict(d_min=0, d_max=255),
                 dict(d_min=0, d_max=2), dict(uniq_pct=100), dict(uniq_pct=0)):
        rc, untouched, _ = call(gl.handle, gr.handle, pts, n, S.StereoRowsParams(**good))
        assert rc == 0 and not untouched, good
    rc, untouched, _ = call(gl.handle, gr.handle, None, 0, ok)
    assert rc == 0 and untouched
    rc, _, (nxt, st, disp, cost) = call(gl.handle, gr.handle, pts, n, ok, (True, True, False, False))
    ref = match_rows(L, R, pts)
    assert rc == 0 and np.array_equal(st, ref[1]) and np.array_equal(nxt.view(np.uint32), ref[0].view(np.uint32))
    assert np.all(disp == -5) and np.all(cost == -6)
    for g in (gl, gr, gs):
        g.close()


def test_two_runs_give_the_same_bits(ctx):
    L, R = scene_pair(KITTI_BF)
    kp = O.fast(L, 20, True)[:, :2]
    gl, gr = ctx.image(L, 0), ctx.image(R, 0)
    a = ctx.stereo_match_rows(gl, gr, kp, want_cost=True)
    b = ctx.stereo_match_rows(gl, gr, kp, want_cost=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    gl.close()
    gr.close()
