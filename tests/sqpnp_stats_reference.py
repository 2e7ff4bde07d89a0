"""References for the batched front end's SQPnP statistics and final fits.

stats_f64: suffstats_block (svo_amd/csrc/suffstats.hpp) restated in numpy float64,
operation by operation (the library is built with -ffp-contract=off, numpy's
element-wise float64 arithmetic is the same IEEE operation each): the per-point
terms, thread tid of 256 accumulating the inlier points tid, tid + 256, ... in
order, per wave the butterfly v = v + v[lane ^ off] for off = 32 .. 1, then
((p0 + p1) + p2) + p3 over the four waves.

stats_longdouble: the same terms from the same float inputs summed in np.longdouble,
with the sum of their magnitudes (the scale of the summation bound).

problem: PnP problems whose object-point mean lies behind the camera when nb
points of the nf + nb do, so that SQPnP's choice between a pose and its mirror
falls to the majority of positive depths.
"""
import numpy as np

import oracle as O

KITTI_K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])
THREADS = 256  # suffstats.hpp kSuffThreads


def problem(nf, nb, seed, zb=40.0):
    """nf points with depth uniform in [6, 30] and nb with depth -uniform(zb, 2 zb),
    (the nf first), lateral coordinates uniform in [-8, 8] x [-3, 3]; a pose of
    rotation vector ~ N(0, 0.05), t ~ N(0, 0.3); object points rounded through
    float32; pixels = pinhole projection + N(0, 0.2) as float32 (KITTI_K).
    -> X (n, 3) f32, uv (n, 2) f32, R_true (3, 3), t_true (3,)."""
    rng = np.random.default_rng(seed)
    n = nf + nb
    z = np.r_[rng.uniform(6, 30, nf), -rng.uniform(zb, 2 * zb, nb)]
    X = np.c_[rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), z]
    R = O.rodrigues(rng.normal(0, 0.05, 3))
    t = rng.normal(0, 0.3, 3)
    X = X.astype(np.float32)
    Y = X.astype(np.float64) @ R.T + t
    K = KITTI_K
    uv = (Y[:, :2] / Y[:, 2:]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]] + rng.normal(0, 0.2, (n, 2))
    return X, uv.astype(np.float32), R, t


def pack_bits(mask, words):
    """mask (n,) bool -> `words` uint32 words, bit i & 31 of word i // 32 = mask[i]."""
    mask = np.asarray(mask, bool)
    out = np.zeros(words, np.uint32)
    i = np.nonzero(mask)[0]
    np.bitwise_or.at(out, i >> 5, (np.uint32(1) << (i & 31).astype(np.uint32)))
    return out


def unpack_bits(words, n):
    """`words` uint32 -> (n,) uint8, the bits of points 0 .. n - 1."""
    i = np.arange(n)
    return ((np.asarray(words, np.uint32)[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(np.uint8)


def _terms(obj, img, K, dt):
    """The 40 terms of every point, (n, 40), in arithmetic of type dt. 1 / fx and
    1 / fy are float64 quotients in either case: the launcher computes them on the
    host and hands them to the kernel."""
    K = np.asarray(K, np.float64).reshape(9)
    ifx, ify = dt(np.float64(1.0) / K[0]), dt(np.float64(1.0) / K[4])
    cx, cy = dt(K[2]), dt(K[5])
    u = img[:, 0].astype(dt)
    v = img[:, 1].astype(dt)
    x = (u - cx) * ifx
    y = (v - cy) * ify
    sq = x * x + y * y
    p = obj.astype(dt)
    pp = np.stack([p[:, 0] * p[:, 0], p[:, 0] * p[:, 1], p[:, 0] * p[:, 2], p[:, 1] * p[:, 1], p[:, 1] * p[:, 2],
                   p[:, 2] * p[:, 2]], axis=1)
    c = np.stack([np.ones(len(x), dt), x, y, sq], axis=1)
    T = np.empty((len(x), 40), dt)
    T[:, 0:4] = c
    for k in range(4):
        T[:, 4 + 3 * k: 7 + 3 * k] = c[:, k: k + 1] * p
        T[:, 16 + 6 * k: 22 + 6 * k] = c[:, k: k + 1] * pp
    return T


def _inliers(n, bits):
    return np.nonzero(unpack_bits(bits, n))[0] if n > 0 else np.zeros(0, np.int64)


def stats_f64(obj, img, n, bits, K):
    """suffstats_block's 40 sums of the points i < n whose bit is set, bit for bit."""
    obj = np.asarray(obj, np.float32).reshape(-1, 3)
    img = np.asarray(img, np.float32).reshape(-1, 2)
    inl = _inliers(n, bits)
    rounds = max(1, -(-n // THREADS))
    T = np.zeros((rounds * THREADS, 40), np.float64)
    with np.errstate(all="ignore"):
        T[inl] = _terms(obj[inl], img[inl], K, np.float64)
    T = T.reshape(rounds, THREADS, 40)
    acc = np.zeros((THREADS, 40), np.float64)
    for r in range(rounds):  # thread tid: points tid, tid + 256, ... in order
        acc = acc + T[r]
    v = acc.reshape(THREADS // 64, 64, 40)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def stats_longdouble(obj, img, n, bits, K):
    """-> (the 40 sums, the 40 sums of |term|, the number of points summed), longdouble."""
    obj = np.asarray(obj, np.float32).reshape(-1, 3)
    img = np.asarray(img, np.float32).reshape(-1, 2)
    inl = _inliers(n, bits)
    T = _terms(obj[inl], img[inl], K, np.longdouble)
    s = np.zeros(40, np.longdouble)
    a = np.zeros(40, np.longdouble)
    for row in T:
        s = s + row
        a = a + np.abs(row)
    return s, a, len(inl)
