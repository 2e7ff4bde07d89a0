"""Rectification maps on the host (svo_init_undistort_rectify_map) against the numpy
restatement of the same rule, bit for bit, and the numpy remap's known answers
(no GPU: host code of the library)."""
import ctypes

import numpy as np
import pytest

import rectify_reference as RR
import svo_amd as S

SIZES = [(1, 1), (5, 3), (97, 61), (320, 240)]


def _K(w, h, f=0.9):
    return np.array([[f * w, 0, 0.5 * w - 0.3], [0, f * w * 1.01, 0.5 * h + 0.2], [0, 0, 1]], np.float64)


RIGS = {
    "five": dict(dist=[-0.28, 0.09, 1e-3, -7e-4, -0.012], rvec=(0.02, -0.03, 0.01)),
    "eight": dict(dist=[0.4, -0.2, 6e-4, 4e-4, 0.05, 0.7, -0.15, 0.02], rvec=(-0.03, 0.015, 0.025)),
    "zero": dict(dist=[0, 0, 0, 0, 0, 0, 0, 0], rvec=(0.01, 0.02, -0.03)),
}


def _both(K, dist, R, newK, w, h):
    got = S.init_undistort_rectify_map(K, dist, R, newK, w, h)
    ref = RR.init_maps(K, dist, R, newK, w, h)
    return got, ref


def _equal(got, ref):
    assert got[0].dtype == np.int16 and got[1].dtype == np.uint16
    assert np.array_equal(got[0], ref[0]), f"map1 differs at {np.argwhere(got[0] != ref[0])[:4].tolist()}"
    assert np.array_equal(got[1], ref[1]), f"map2 differs at {np.argwhere(got[1] != ref[1])[:4].tolist()}"
    assert int(got[1].max()) < 1024


@pytest.mark.parametrize("rig", sorted(RIGS))
@pytest.mark.parametrize("size", SIZES)
def test_init_maps_equal_the_numpy_restatement(size, rig):
    w, h = size
    K = _K(max(w, 40), max(h, 30))
    newK = K.copy()
    newK[0, 2] -= 1.75
    newK[1, 2] += 0.6
    newK[0, 0] *= 0.97
    got, ref = _both(K, RIGS[rig]["dist"], RR.rodrigues(*RIGS[rig]["rvec"]), newK, w, h)
    _equal(got, ref)
    if rig != "zero" and w > 5:
        assert len(np.unique(got[1])) > 50  # the fractions are exercised


def test_corners_far_outside_saturate():
    """A wide-angle newK with strong positive distortion sends the corners tens of
    thousands of pixels out: the int16 cast saturates (at +-32767 / -32768)."""
    w, h = 97, 61
    K = _K(w, h, f=40.0)
    newK = _K(w, h, f=0.05)
    got, ref = _both(K, [3.0, 8.0, 0, 0, 20.0], np.eye(3), newK, w, h)
    _equal(got, ref)
    assert got[0].max() == 32767 and got[0].min() == -32768


def test_w_crossing_zero_gives_nan_and_infinity():
    """A rotation of ~90 degrees puts the plane w = 0 inside the image: 1 / _w is
    infinite there and the pixel's coordinates NaN or infinite (INT_MIN / saturation)."""
    w, h = 97, 61
    K = _K(w, h)
    R = RR.rodrigues(0.0, 1.2, 0.0)
    got, ref = _both(K, RIGS["five"]["dist"], R, K, w, h)
    _equal(got, ref)
    # and exactly zero: newK R chosen so that _w starts at -2 and steps by 1
    M = np.array([[1.0, 0, 0], [0, 1, 0], [1, 0, -2]])
    newK = np.linalg.inv(M)
    assert np.array_equal(RR.inverse_by_cofactors(newK)[0].reshape(3, 3), M)
    got, ref = _both(K, RIGS["eight"]["dist"], np.eye(3), newK, 5, 3)
    _equal(got, ref)
    assert got[0][0, 2, 0] == -32768  # _w = 0 at column 2: x = inf or NaN


def test_identity_rig_gives_the_pixel_grid():
    w, h = 97, 61
    K = np.array([[64.0, 0, 32], [0, 64, 16], [0, 0, 1]])  # powers of two: every step exact
    m1, m2 = S.init_undistort_rectify_map(K, np.zeros(8), np.eye(3), K, w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    assert np.array_equal(m1[..., 0], xx) and np.array_equal(m1[..., 1], yy)
    assert not m2.any()
    _equal((m1, m2), RR.init_maps(K, np.zeros(8), np.eye(3), K, w, h))


def test_singular_rig_is_refused_with_the_outputs_untouched():
    K = _K(40, 30)
    newK = K.copy()
    newK[2] = 0  # a zero row: every product of the determinant is zero, det = 0 exactly
    assert RR.init_maps(K, np.zeros(8), np.eye(3), newK, 5, 3) is None
    m1 = np.full((3, 5, 2), 77, np.int16)
    m2 = np.full((3, 5), 99, np.uint16)
    f64 = ctypes.POINTER(ctypes.c_double)
    args = [np.ascontiguousarray(a, np.float64).ravel() for a in (K, np.zeros(8), np.eye(3), newK)]
    rc = S.lib().svo_init_undistort_rectify_map(*[a.ctypes.data_as(f64) for a in args], 5, 3,
                                                m1.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                                                m2.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
    assert rc == -1  # SVO_ERR_ARG
    assert (m1 == 77).all() and (m2 == 99).all()
    with pytest.raises(S.SvoError):
        S.init_undistort_rectify_map(K, np.zeros(8), np.eye(3), newK, 5, 3)
    with pytest.raises(S.SvoError):
        S.init_undistort_rectify_map(K, np.zeros(8), np.eye(3), K, 0, 3)


def _one(taps, a, b):
    src = np.array(taps, np.uint8).reshape(2, 2)
    return int(RR.remap(src, np.zeros((1, 1, 2), np.int16), np.array([[b * 32 + a]], np.uint16))[0, 0])


def test_numpy_remap_known_answers():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    yy, xx = np.mgrid[0:7, 0:9]
    ident = np.stack([xx, yy], -1).astype(np.int16)
    assert np.array_equal(RR.remap(img, ident, np.zeros((7, 9), np.uint16)), img)
    assert _one([1, 2, 3, 4], 16, 16) == 3   # 2.5 + 512 / 1024 -> 3
    assert _one([0, 0, 0, 2], 16, 16) == 1   # exactly one half rounds up
    assert _one([0, 0, 0, 1], 16, 16) == 0
    assert _one([200, 0, 0, 0], 0, 0) == 200
    # outside taps are zero: the pixel one left of the image at a = 16 sees half of column 0
    m1 = np.array([[[-1, 0]]], np.int16)
    assert int(RR.remap(img, m1, np.array([[16]], np.uint16))[0, 0]) == (16 * 32 * int(img[0, 0]) + 512) >> 10


def test_symbols_are_present():
    lib = ctypes.CDLL(S.lib_path())
    for name in ("svo_rect_maps_create", "svo_rect_maps_destroy", "svo_init_undistort_rectify_map", "svo_remap",
                 "svo_image_upload_raw", "svo_frontend_set_rectification", "svo_frontend_time_ingest"):
        assert hasattr(lib, name), name
