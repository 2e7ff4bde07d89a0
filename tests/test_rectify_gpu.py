"""The rectifying kernel (svo_remap: host in, host out, the launcher the front end
uses with one sequence) against the numpy restatement of cv::remap's fixed-point
rule: exact equality, grey and BGR, over quads and tails, unaligned rows, every
fraction, every edge combination, saturated map entries and random maps; then
svo_image_upload_raw through the pyramid, and svo_rect_maps_create's rejections."""
import ctypes as C

import numpy as np
import pytest

import rectify_reference as RR
import svo_amd as S

pytestmark = pytest.mark.gpu

_u8p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def ctx():
    c = S.Context(0)
    yield c
    c.close()


def _source(rng, raw_w, raw_h, stride, bgr):
    """-> (host buffer (raw_h, stride * bpp) with 255 in the row padding, grey (raw_h, raw_w)):
    non-zero everywhere, so a tap taken from the wrong side of an edge shows."""
    bpp = 3 if bgr else 1
    buf = np.full((raw_h, stride * bpp), 255, np.uint8)
    if bgr:
        px = RR.bgr_of(rng.integers(60, 200, (raw_h, raw_w), dtype=np.uint8), int(rng.integers(1 << 30)))
        buf[:, :raw_w * 3] = px.reshape(raw_h, raw_w * 3)
        grey = RR.gray_of(px)
    else:
        grey = rng.integers(1, 256, (raw_h, raw_w), dtype=np.uint8)
        buf[:, :raw_w] = grey
    assert grey.min() > 0
    return buf, grey


def _remap(ctx, buf, bgr, maps):
    out = np.full((maps.h, maps.w + 3), 7, np.uint8)  # dst_stride > w: the columns beyond stay
    ctx._check(S.lib().svo_remap(ctx.handle, buf.ctypes.data_as(_u8p), buf.shape[1], int(bgr), maps.handle,
                                 out.ctypes.data_as(_u8p), out.shape[1]))
    assert (out[:, maps.w:] == 7).all()
    return out[:, :maps.w].copy()


def _check(ctx, rng, raw_w, raw_h, stride, bgr, map1, map2):
    buf, grey = _source(rng, raw_w, raw_h, stride, bgr)
    maps = S.RectMaps(ctx, raw_w, raw_h, map1, map2)
    got = _remap(ctx, buf, bgr, maps)
    maps.close()
    ref = RR.remap(grey, map1, map2)
    assert np.array_equal(got, ref), f"differs at (y, x) {np.argwhere(got != ref)[:6].tolist()}"
    return got


def _random_maps(rng, w, h, raw_w, raw_h):
    m1 = np.stack([rng.integers(-8, raw_w + 8, (h, w)), rng.integers(-8, raw_h + 8, (h, w))], -1).astype(np.int16)
    return m1, rng.integers(0, 1024, (h, w)).astype(np.uint16)


RAWS = [(2, 2, 2), (61, 7, 61), (61, 7, 64)]  # (raw_w, raw_h, stride in pixels)
OUTS = [(1, 1), (3, 2), (4, 1), (5, 3), (67, 5)]


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("raw", RAWS)
def test_quads_tails_and_unaligned_rows(ctx, raw, bgr):
    raw_w, raw_h, stride = raw
    rng = np.random.default_rng(raw_w * 100 + stride + bgr)
    for w, h in OUTS:
        _check(ctx, rng, raw_w, raw_h, stride, bgr, *_random_maps(rng, w, h, raw_w, raw_h))


@pytest.mark.parametrize("bgr", [False, True])
def test_every_fraction(ctx, bgr):
    rng = np.random.default_rng(11 + bgr)
    raw_w, raw_h = 41, 37
    m1 = np.stack([rng.integers(0, raw_w - 1, (32, 32)), rng.integers(0, raw_h - 1, (32, 32))], -1).astype(np.int16)
    m2 = np.arange(1024, dtype=np.uint16).reshape(32, 32)
    got = _check(ctx, rng, raw_w, raw_h, raw_w, bgr, m1, m2)
    assert len(np.unique(got)) > 30


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("raw", [(2, 2, 2), (9, 6, 9), (61, 7, 64)])
def test_every_edge_combination(ctx, raw, bgr):
    raw_w, raw_h, stride = raw
    rng = np.random.default_rng(5 + bgr)
    xs = [-2, -1, 0, raw_w - 2, raw_w - 1, raw_w]
    ys = [-2, -1, 0, raw_h - 2, raw_h - 1, raw_h]
    cells = [(sx, sy, a, b) for sy in ys for sx in xs for a in (0, 13, 31) for b in (0, 13, 31)]
    assert len(cells) == 324
    c = np.array(cells).reshape(12, 27, 4)  # 27 columns: six quads and a tail of three
    m1 = c[..., :2].astype(np.int16)
    m2 = (c[..., 3] * 32 + c[..., 2]).astype(np.uint16)
    _check(ctx, rng, raw_w, raw_h, stride, bgr, m1, m2)


@pytest.mark.parametrize("bgr", [False, True])
def test_saturated_map_entries(ctx, bgr):
    rng = np.random.default_rng(17)
    ext = [32767, -32767, -32768, 0, 3]
    cells = [(sx, sy) for sy in ext for sx in ext]
    m1 = np.array(cells, np.int16).reshape(5, 5, 2)
    m2 = rng.integers(0, 1024, (5, 5)).astype(np.uint16)
    got = _check(ctx, rng, 9, 6, 9, bgr, m1, m2)
    assert got[3:, 3:].all() and not got[:3].any() and not got[:, :3].any()


@pytest.mark.parametrize("bgr", [False, True])
def test_random_map_over_a_larger_image(ctx, bgr):
    rng = np.random.default_rng(23 + bgr)
    raw_w, raw_h, w, h = 353, 67, 1029, 9  # more than one block of quads per row, a tail of one
    _check(ctx, rng, raw_w, raw_h, raw_w, bgr, *_random_maps(rng, w, h, raw_w, raw_h))


@pytest.mark.parametrize("bgr", [False, True])
def test_image_upload_raw_through_the_pyramid(ctx, bgr):
    rng = np.random.default_rng(29 + bgr)
    raw_w, raw_h, w, h = 90, 70, 67, 45
    buf, grey = _source(rng, raw_w, raw_h, raw_w, bgr)
    K = np.array([[80.0, 0, 44.2], [0, 81, 35.1], [0, 0, 1]])
    newK = np.array([[78.0, 0, 33.0], [0, 78, 22.5], [0, 0, 1]])
    m1, m2 = RR.init_maps(K, [-0.2, 0.05, 1e-3, -1e-3], RR.rodrigues(0.01, -0.02, 0.015), newK, w, h)
    maps = S.RectMaps(ctx, raw_w, raw_h, m1, m2)
    rectified = RR.remap(grey, m1, m2)  # (held: the upload reads it after ctx.image returns)
    blank = np.zeros((h, w), np.uint8)
    ref = ctx.image(rectified, 2)
    img = ctx.image(blank, 2)
    ctx._check(S.lib().svo_ctx_synchronize(ctx.handle))
    img.upload_raw(buf.reshape((raw_h, raw_w, 3) if bgr else (raw_h, raw_w)), maps)
    for lvl in range(3):
        assert np.array_equal(img.level(lvl), ref.level(lvl)), f"level {lvl}"
    assert ref.level(0).std() > 10
    other = ctx.image(np.zeros((h, w + 1), np.uint8), 2)
    with pytest.raises(S.SvoError):  # not the maps' size
        other.upload_raw(buf.reshape((raw_h, raw_w, 3) if bgr else (raw_h, raw_w)), maps)
    for o in (ref, img, other, maps):
        o.close()


def test_create_rejections(ctx):
    m1 = np.zeros((3, 5, 2), np.int16)
    m2 = np.zeros((3, 5), np.uint16)
    S.RectMaps(ctx, 2, 2, m1, m2).close()  # the smallest raw image
    bad = m2.copy()
    bad[2, 4] = 1024
    with pytest.raises(S.SvoError):
        S.RectMaps(ctx, 8, 8, m1, bad)
    with pytest.raises(S.SvoError):
        S.RectMaps(ctx, 1, 8, m1, m2)
    with pytest.raises(S.SvoError):
        S.RectMaps(ctx, 8, 1, m1, m2)
    L = S.lib()
    out = C.c_void_p()
    p1, p2 = m1.ctypes.data_as(C.POINTER(C.c_int16)), m2.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.svo_rect_maps_create(ctx.handle, 8, 8, 5, 3, None, p2, C.byref(out)) == -1
    assert L.svo_rect_maps_create(ctx.handle, 8, 8, 5, 3, p1, None, C.byref(out)) == -1
    assert L.svo_rect_maps_create(ctx.handle, 8, 8, 5, 3, p1, p2, None) == -1
    assert L.svo_rect_maps_create(None, 8, 8, 5, 3, p1, p2, C.byref(out)) == -1
    assert L.svo_rect_maps_create(ctx.handle, 8, 8, 0, 3, p1, p2, C.byref(out)) == -1
    assert not out.value
