"""numpy restatement of the rectifying ingest's two rules (TEST INFRASTRUCTURE).

init_maps: cv::initUndistortRectifyMap(K, dist, R, newK, (w, h), CV_16SC2) as
svo_init_undistort_rectify_map states it (include/svo_gpu.h): f64, operation by
operation in the order of OpenCV's scalar loop, the running sums along a row kept
with np.cumsum (a sequential sum), coordinates rounded half to even at 1/32
pixel, int32 and int16 casts saturating.

remap: cv::remap(src, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) of 8-bit grey
with the fixed-point maps, pure integer:
  out = ((32-a)(32-b) t00 + a(32-b) t01 + (32-a)b t10 + ab t11 + 512) >> 10
"""
import numpy as np

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1


def rodrigues(rx, ry, rz):
    """Rotation matrix of the rotation vector (rx, ry, rz)."""
    v = np.array([rx, ry, rz], np.float64)
    th = float(np.linalg.norm(v))
    if th == 0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _round_sat(v):
    """round half to even, saturated to int32, NaN -> INT_MIN"""
    with np.errstate(invalid="ignore"):
        r = np.rint(v)
        out = np.where(np.isnan(r), float(INT_MIN), np.clip(r, float(INT_MIN), float(INT_MAX)))
    return out.astype(np.int64)


def inverse_by_cofactors(m):
    """(m^-1, det) of a 3x3 by cofactors, each entry (cofactor) * (1 / det)."""
    m = np.asarray(m, np.float64).reshape(9)
    det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    with np.errstate(all="ignore"):
        d = np.float64(1.0) / det
        ir = np.array([(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d,
                       (m[1] * m[5] - m[2] * m[4]) * d, (m[5] * m[6] - m[3] * m[8]) * d,
                       (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
                       (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d,
                       (m[0] * m[4] - m[1] * m[3]) * d])
    return ir, det


def init_maps(K, dist, R, newK, w, h):
    """-> (map1 (h, w, 2) int16, map2 (h, w) uint16), or None where newK R is singular."""
    K, R, newK = (np.asarray(a, np.float64).reshape(3, 3) for a in (K, R, newK))
    d = np.zeros(8)
    d[:len(dist)] = dist
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(c) for c in d)
    M = np.array([[(newK[i, 0] * R[0, j] + newK[i, 1] * R[1, j]) + newK[i, 2] * R[2, j] for j in range(3)]
                  for i in range(3)])
    ir, det = inverse_by_cofactors(M)
    if det == 0 or not np.isfinite(det):
        return None
    i = np.arange(h, dtype=np.float64)[:, None]

    def running(first, step):  # first, first + step, (first + step) + step, ...
        a = np.empty((h, w))
        a[:, :1] = first
        a[:, 1:] = step
        return np.cumsum(a, axis=1)

    with np.errstate(all="ignore"):
        _x = running(i * ir[1] + ir[2], ir[0])
        _y = running(i * ir[4] + ir[5], ir[3])
        _w = running(i * ir[7] + ir[8], ir[6])
        ww = 1.0 / _w
        x, y = _x * ww, _y * ww
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        _2xy = 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
        u = K[0, 0] * xd + K[0, 2]
        v = K[1, 1] * yd + K[1, 2]
        iu, iv = _round_sat(u * 32), _round_sat(v * 32)
    map1 = np.stack([np.clip(iu >> 5, -32768, 32767), np.clip(iv >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    map2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return map1, map2


def remap(src, map1, map2):
    """src (raw_h, raw_w) uint8 -> (h, w) uint8."""
    src = np.asarray(src)
    assert src.ndim == 2 and src.dtype == np.uint8
    rh, rw = src.shape
    sx = map1[..., 0].astype(np.int64)
    sy = map1[..., 1].astype(np.int64)
    m2 = map2.astype(np.int64)
    a, b = m2 & 31, m2 >> 5

    def tap(i, j):
        yy, xx = sy + i, sx + j
        ok = (yy >= 0) & (yy < rh) & (xx >= 0) & (xx < rw)
        return np.where(ok, src[np.clip(yy, 0, rh - 1), np.clip(xx, 0, rw - 1)].astype(np.int64), 0)

    out = ((32 - a) * (32 - b) * tap(0, 0) + a * (32 - b) * tap(0, 1) + (32 - a) * b * tap(1, 0) +
           a * b * tap(1, 1) + 512) >> 10
    return out.astype(np.uint8)


def gray_of(bgr):
    """cv::cvtColor(BGR2GRAY) of 8UC3: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    c = np.asarray(bgr).astype(np.int64)
    return ((1868 * c[..., 0] + 9617 * c[..., 1] + 4899 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def bgr_of(gray, seed):
    """A BGR frame whose channels differ (the conversion's weights matter)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-40, 41, gray.shape + (2,))
    b = np.clip(gray.astype(np.int32) + d[..., 0], 0, 255)
    r = np.clip(gray.astype(np.int32) - d[..., 1], 0, 255)
    return np.ascontiguousarray(np.stack([b, gray, r], axis=-1).astype(np.uint8))
