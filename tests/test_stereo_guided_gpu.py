"""svo_stereo_match_rows_guided and svo_stereo_row_priors on the device against the
numpy restatement (tests/stereo_track_reference.py): every output bit for bit.
160 x 96 images: partial groups of four points, partial waves, points with and
without a prior inside one wave."""
import ctypes as C

import numpy as np
import pytest

import svo_amd as S
from stereo_rows_reference import match_rows
from stereo_track_reference import NO_PRIOR, match_rows_guided, row_priors
from test_stereo_rows_gpu import BAD_PARAMS, blocky_pair, point_mix, random_pair

pytestmark = pytest.mark.gpu

_f32p, _u8p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
W, H, SHIFT = 160, 96, 9
I32_MAX, I32_MIN1 = 2 ** 31 - 1, -(2 ** 31) + 1


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def same(got, ref, tag, pts):
    for name, g, r in zip(("next_xy", "status", "disparity", "cost"), got, ref):
        g, r = np.asarray(g), np.asarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, (tag, name)
        gv, rv = (g.view(np.uint32), r.view(np.uint32)) if g.dtype == np.float32 else (g, r)
        bad = np.flatnonzero((gv != rv).reshape(len(g), -1).any(axis=1)) if len(g) else []
        assert len(bad) == 0, (tag, name, len(bad), pts[bad[:5]], g[bad[:5]], r[bad[:5]])


def check(ctx, L, R, pts, prior, guide, tag="", **params):
    gl, gr = ctx.image(L, 0), ctx.image(R, 0)
    try:
        got = ctx.stereo_match_rows_guided(gl, gr, pts, prior, guide, S.StereoRowsParams(**params), want_cost=True)
    finally:
        gl.close()
        gr.close()
    ref = match_rows_guided(L, R, pts, prior, guide, **params)
    same(got, ref, tag, pts)
    return ref


def mixed_priors(n, seed, centre=SHIFT, spread=3, none_every=4):
    """Priors around the true shift; every none_every-th point (and a run of five) has none."""
    rng = np.random.default_rng(seed)
    p = centre + rng.integers(-spread, spread + 1, n)
    p[::none_every] = NO_PRIOR
    p[10:15] = NO_PRIOR
    return p.astype(np.int32)


@pytest.mark.parametrize("guide", [1, 4, 15])
@pytest.mark.parametrize("r", [1, 5, 7])
def test_every_radius_and_guide(ctx, r, guide):
    pts = point_mix(W, H)
    for image, pair in (("blocky", blocky_pair), ("random", random_pair)):
        L, R = pair(W, H, seed=11)
        for uniq in (80, 0):
            prior = mixed_priors(len(pts), seed=r * 16 + guide)
            _, st, disp, _ = check(ctx, L, R, pts, prior, guide, (image, r, guide, uniq), radius=r, d_min=-1,
                                   d_max=40, uniq_pct=uniq)
            has = prior != NO_PRIOR
            assert 0 < st[has].sum() < has.sum() and 0 < st[~has].sum() < (~has).sum()
            assert np.all(np.abs(disp[has & (st == 1)] - prior[has & (st == 1)]) < guide)  # interior of the guide
    assert st[np.isnan(pts).any(axis=1)].sum() == 0


@pytest.mark.parametrize("n", [0, 1, 5, 67])
def test_point_counts(ctx, n):
    L, R = blocky_pair(W, H, seed=5)
    pts = np.array([(x, y) for y in range(10, H - 8, 11) for x in range(30, W - 10, 13)], np.float32)[:n]
    assert len(pts) == n
    for none_every in (4, 3, 10 ** 6):  # the last: every point (but the run of five) has a prior
        prior = mixed_priors(max(n, 15), 3, none_every=none_every)[:n]
        _, st, _, _ = check(ctx, L, R, pts, prior, 4, (n, none_every))
        assert len(st) == n and (n < 5 or st.sum() > n // 2)


def test_edge_priors(ctx):
    L, R = blocky_pair(W, H, seed=7, shift=3)
    par = dict(radius=5, d_min=-2, d_max=40, uniq_pct=0)
    edge = [-2, -1, 0, 1, 3, 5, -5, -6, -7, -17, 36, 38, 40, 41, 43, 44, 45, 55, 56, 300, 321, -64, -65, I32_MAX,
            I32_MAX - 1, I32_MIN1, I32_MIN1 + 1, NO_PRIOR]
    # interior columns; columns where xi - d < 0 clips the range; columns at w - 1 where d < 0 is clipped
    cols = [80.0, 0.0, 1.0, 2.0, 3.0, 4.4, 6.5, 12.0, W - 1.0, W - 2.0, W - 3.0, W - 1.5]
    pts = np.array([(x, 40.0) for x in cols for _ in edge], np.float32)
    prior = np.array(edge * len(cols), np.int64).astype(np.int32)
    for guide in (1, 4, 15):
        _, st, disp, _ = check(ctx, L, R, pts, prior, guide, ("edge", guide), **par)
        g = st.reshape(len(cols), len(edge))
        assert g[0].any() and not g[0][[edge.index(v) for v in (I32_MAX, I32_MIN1, 300, -65)]].any()
    # fewer than 3 candidates: two at the top of the range, two at the bottom, none at all
    _, st, _, _ = check(ctx, L, R, pts[:4], [44, -6, 45, I32_MAX], 4, "short", **par)
    assert not st.any()
    # the image leaves two candidates of a guided range of nine: x = 1, d in [-2, 1] cut to prior 4 - 4 = 0
    _, st, _, _ = check(ctx, L, R, np.array([[1.0, 40.0]], np.float32), [4], 4, "clipped", **par)
    assert st[0] == 0


def test_edge_points_take_the_inputs_bits(ctx):
    L, R = random_pair(W, H, seed=2)
    pts = np.array([(np.nan, 4), (4, np.inf), (-1, 5), (W, 5), (5, -1), (5, H), (1e9, 3), (-0.51, 5), (W - 0.49, 5),
                    (-0.5, 10), (W - 0.5, 10), (30, -0.5), (30, H - 0.5)], np.float32)
    ref = check(ctx, L, R, pts, np.full(len(pts), SHIFT, np.int32), 4, "outside", d_min=-1, d_max=40)
    assert not ref[1][:9].any() and np.array_equal(ref[0][:9].view(np.uint32), pts[:9].view(np.uint32))


def test_edge_images(ctx):
    pts = point_mix(W, H)
    Cst = np.full((H, W), 93, np.uint8)
    for uniq in (80, 0):  # all costs equal: the first candidate wins, no bracket
        nxt, st, disp, cost = check(ctx, Cst, Cst, pts, mixed_priors(len(pts), 1), 4, "constant", uniq_pct=uniq)
        assert st.sum() == 0 and not disp.any() and not cost.any()
        assert np.array_equal(nxt.view(np.uint32), pts.view(np.uint32))
    # period-4 columns: equal costs at 4 and 8, both inside 6 +- 4: the smaller one
    col = np.array([10, 200, 90, 40], np.uint8)
    Lp = np.tile(col, (H, W // 4))
    p = np.array([(x, y) for y in (16.0, 40.0) for x in (48.0, 61.0, 90.5)], np.float32)
    _, st, disp, cost = check(ctx, Lp, Lp, p, np.full(len(p), 6, np.int32), 4, "tie", uniq_pct=0)
    assert st.all() and np.all(disp == 4) and not cost.any()
    _, st, _, _ = check(ctx, Lp, Lp, p, np.full(len(p), 6, np.int32), 4, "tie-uniq", uniq_pct=80)
    assert not st.any()  # the runner-up at 8 costs 0 as well
    # den == 0 needs c- == c0 == c+, which the tie rule rules out (d* - 1 would win); the
    # nearest case, a flat minimum that starts inside (c- > c0 == c+): delta = 1/2 exactly
    ramp = np.minimum(np.arange(W), 60).astype(np.uint8) * 4
    Lr = np.tile(ramp, (H, 1))
    Rr = np.full((H, W), 240, np.uint8)
    Rr[:, 86] = 0
    q = np.array([[80.0, 16.0]], np.float32)
    nx, s2, d2, c2 = check(ctx, Lr, Rr, q, [1], 2, "flat", d_min=-3, d_max=30, uniq_pct=0)
    assert s2[0] == 1 and d2[0] == 0 and c2[0] == 0 and nx[0, 0] == np.float32(79.5)


def test_no_prior_and_guide_zero_are_stereo_match_rows(ctx):
    L, R = blocky_pair(W, H, seed=11)
    pts = point_mix(W, H)
    gl, gr = ctx.image(L, 0), ctx.image(R, 0)
    par = S.StereoRowsParams(d_min=-1, d_max=40)
    want = ctx.stereo_match_rows(gl, gr, pts, par, want_cost=True)
    same(want, match_rows(L, R, pts, d_min=-1, d_max=40), "plain", pts)
    prior = mixed_priors(len(pts), 9)
    for tag, got in (("none", ctx.stereo_match_rows_guided(gl, gr, pts, None, 4, par, want_cost=True)),
                     ("guide 0", ctx.stereo_match_rows_guided(gl, gr, pts, prior, 0, par, want_cost=True)),
                     ("all without", ctx.stereo_match_rows_guided(gl, gr, pts, np.full(len(pts), NO_PRIOR), 4, par,
                                                                  want_cost=True))):
        same(got, want, tag, pts)
    # the same points in another order: the same outputs per point
    a = ctx.stereo_match_rows_guided(gl, gr, pts, prior, 4, par, want_cost=True)
    perm = np.random.default_rng(4).permutation(len(pts))
    b = ctx.stereo_match_rows_guided(gl, gr, pts[perm], prior[perm], 4, par, want_cost=True)
    same(b, [x[perm] for x in a], "order", pts[perm])
    gl.close()
    gr.close()


def test_bad_arguments_write_nothing(ctx):
    L, R = random_pair(W, H, seed=2)
    gl, gr, gs = ctx.image(L, 0), ctx.image(R, 0), ctx.image(L[:, :90], 0)
    pts = point_mix(W, H)[:40]
    n = len(pts)
    prior = mixed_priors(n, 2)
    fn = S.lib().svo_stereo_match_rows_guided

    def call(left, right, p, n_, par, guide=4, pr=prior, want=(True, True)):
        nxt = np.full((n, 2), 7.25, np.float32)
        st = np.full(n, 9, np.uint8)
        disp = np.full(n, -5, np.int32)
        cost = np.full(n, -6, np.int32)
        rc = fn(ctx.handle, left, right, None if p is None else p.ctypes.data_as(_f32p), n_,
                None if par is None else C.byref(par), None if pr is None else pr.ctypes.data_as(_i32p), guide,
                nxt.ctypes.data_as(_f32p) if want[0] else None, st.ctypes.data_as(_u8p) if want[1] else None,
                disp.ctypes.data_as(_i32p), cost.ctypes.data_as(_i32p))
        untouched = np.all(nxt == 7.25) and np.all(st == 9) and np.all(disp == -5) and np.all(cost == -6)
        return rc, untouched

    ok = S.StereoRowsParams()
    for bad in BAD_PARAMS:
        assert call(gl.handle, gr.handle, pts, n, S.StereoRowsParams(**bad)) == (-1, True), bad
    for guide in (-1, 16, 1 << 20):
        for pr in (prior, None):
            assert call(gl.handle, gr.handle, pts, n, ok, guide, pr) == (-1, True), guide
        with pytest.raises(S.SvoError):
            ctx.stereo_match_rows_guided(gl, gr, pts, prior, guide)
    for args in ((None, gr.handle, pts, n, ok), (gl.handle, None, pts, n, ok), (gl.handle, gr.handle, None, n, ok),
                 (gl.handle, gr.handle, pts, n, None), (gl.handle, gr.handle, pts, -1, ok),
                 (gl.handle, gs.handle, pts, n, ok)):
        assert call(*args) == (-1, True), args[3:]
    for want in ((False, True), (True, False)):
        assert call(gl.handle, gr.handle, pts, n, ok, want=want) == (-1, True)
    for guide in (0, 1, 15):
        assert call(gl.handle, gr.handle, pts, n, ok, guide) == (0, False), guide
    assert call(gl.handle, gr.handle, None, 0, ok) == (0, True)
    for g in (gl, gr, gs):
        g.close()


def test_row_priors(ctx):
    prev_mid = np.array([3, 4, 9, 20, 21, 40], np.int32)
    prev_xy = np.array([[50.5, 1], [40.25, 2], [10, 3], [np.inf, 4], [12.5, 5], [90.75, 6]], np.float32)
    prev_ur = np.array([48.0, -1.0, 12.5, 3.0, 10.0, 60.5], np.float32)
    mid = np.array([40, 3, 0, 2, 5, 8, 9, 10, 20, 21, 22, 41, 2 ** 31 - 1, 4], np.int32)
    got = ctx.stereo_row_priors(mid, prev_mid, prev_xy, prev_ur)
    want = row_priors(mid, prev_mid, prev_xy, prev_ur)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # first and last places, absent below / between / above, ur -1, inf, ties to even (2.5 -> 2, -2.5 -> -2)
    assert list(got) == [30, 2, NO_PRIOR, NO_PRIOR, NO_PRIOR, NO_PRIOR, -2, NO_PRIOR, NO_PRIOR, 2, NO_PRIOR, NO_PRIOR,
                         NO_PRIOR, NO_PRIOR]
    for pm, pxy, pur in ((prev_mid[:0], prev_xy[:0], prev_ur[:0]), (prev_mid[:1], prev_xy[:1], prev_ur[:1]),
                         (prev_mid[2:3], prev_xy[2:3], prev_ur[2:3])):
        assert np.array_equal(ctx.stereo_row_priors(mid, pm, pxy, pur), row_priors(mid, pm, pxy, pur)), len(pm)
    assert len(ctx.stereo_row_priors(mid[:0], prev_mid, prev_xy, prev_ur)) == 0
    # halves, NaN, values past +-32767, a long list (several blocks)
    rng = np.random.default_rng(6)
    pm = np.cumsum(rng.integers(1, 4, 3000)).astype(np.int32)
    pxy = np.stack([rng.integers(0, 2400, 3000) / 2, rng.uniform(0, 100, 3000)], 1).astype(np.float32)
    pur = np.where(rng.random(3000) < 0.2, -1, rng.integers(0, 2400, 3000) / 2).astype(np.float32)
    pxy[5, 0], pxy[6, 0], pxy[7, 0], pur[8] = np.nan, 40000.0, -40000.0, np.nan
    pur[5:8] = 1.0
    m = np.arange(pm[-1] + 3, dtype=np.int32)
    got, want = ctx.stereo_row_priors(m, pm, pxy, pur), row_priors(m, pm, pxy, pur)
    assert np.array_equal(got, want) and np.sum(want != NO_PRIOR) > 2000
    assert all(want[pm[k]] == NO_PRIOR for k in (5, 6, 7, 8))
    fn = S.lib().svo_stereo_row_priors
    out = np.full(4, 77, np.int32)
    i32 = lambda a: a.ctypes.data_as(_i32p)  # noqa: E731
    f32 = lambda a: a.ctypes.data_as(_f32p)  # noqa: E731
    assert fn(None, i32(mid), 4, i32(prev_mid), f32(prev_xy), f32(prev_ur), 6, i32(out)) == -1
    assert fn(ctx.handle, i32(mid), -1, i32(prev_mid), f32(prev_xy), f32(prev_ur), 6, i32(out)) == -1
    assert fn(ctx.handle, i32(mid), 4, i32(prev_mid), f32(prev_xy), f32(prev_ur), -1, i32(out)) == -1
    assert fn(ctx.handle, i32(mid), 4, None, f32(prev_xy), f32(prev_ur), 6, i32(out)) == -1
    assert fn(ctx.handle, None, 4, i32(prev_mid), f32(prev_xy), f32(prev_ur), 6, i32(out)) == -1
    assert np.all(out == 77)
