"""The two-view DLT (svo_amd/csrc/dlt.hpp, behind svo_triangulate_points and the
front end's keyframe append) where the loop tests never reach: sub-pixel and
negative disparity at KITTI's real fx * b, vertical mismatch up to the keep
rule's 40 px, pixels on the principal point (exact zeros in A), a non-rectified
right camera, the tail of a 256-thread block and null outputs.

Reference: a float64 restatement in this file (A from the float32 P and points,
numpy's SVD, unit length, w >= 0, rounded to float32, float32 divide by w) --
independent of the kernel (Jacobi on A^T A) and of oracle/triangulate.c (OpenCV's
Jacobi SVD restated). The CPU tests hold the oracle to it at 0 ulp, so whatever
the GPU tests find beyond that is the kernel's.

Bars: the project's (xyzw atol 2e-7, xyz rtol 1e-5 / atol 1e-5, against both
references), the keep decision z > 0 equal on every point, and ULP_BAR float32
ulp on every xyz component that is not small against its point's largest one.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import svo_amd as S
from svo_amd.scene import STEREO_BF, intrinsics, rot, stereo_projections

W, H = 1241, 376
KITTI_BF = 386.1448
N_BAND = 2000
MIN_DISP = 0.01          # below ~1e-4 px the sign of w is rounding noise in any SVD
# xyz = h_k * (1 / h_3) in float32, h = the unit vector rounded to float32: h_k and
# h_3 may each round across a boundary against the reference (1 + 1 ulp), the
# reciprocal and the product are correctly rounded (1/2 + 1/2), 1 ulp of slack
# (-ffp-contract=off, no fast-math).
ULP_BAR = 4
SMALL = 1e-3             # components below SMALL * max|xyz| of their point are left out ...
MAX_EXCLUDED = 0.01      # ... and may be at most this share of a band's components


# ------------------------------------------------------------------ reference
def ref_triangulate(P1, P2, p1, p2):
    """cv::triangulatePoints + convertPointsFromHomogeneous in float64 numpy."""
    P1, P2 = (np.asarray(P, np.float32).reshape(3, 4).astype(np.float64) for P in (P1, P2))
    p1, p2 = (np.asarray(p, np.float32).reshape(-1, 2).astype(np.float64) for p in (p1, p2))
    if len(p1) == 0:
        return np.zeros((0, 4), np.float32), np.zeros((0, 3), np.float32)
    A = np.stack([p1[:, :1] * P1[2] - P1[0], p1[:, 1:] * P1[2] - P1[1],
                  p2[:, :1] * P2[2] - P2[0], p2[:, 1:] * P2[2] - P2[1]], axis=1)
    v = np.linalg.svd(A)[2][:, 3]
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    v = v * np.where(v[:, 3:] < 0, -1.0, 1.0)
    h = v.astype(np.float32)
    with np.errstate(divide="ignore"):
        sc = np.where(h[:, 3] != 0, np.float32(1) / h[:, 3], np.float32(1)).astype(np.float32)
    return h, h[:, :3] * sc[:, None]


def ulp_distance(a, b):
    """Distance in float32 ulp: the number of representable values between a and b."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def significant(xyz):
    """The components the ulp bar applies to: |component| >= SMALL * max|xyz| of its point."""
    a = np.abs(xyz.astype(np.float64))
    return a >= SMALL * a.max(axis=1, keepdims=True)


# ------------------------------------------------------------------ inputs
K = intrinsics(W, H)


def _left(rng, n):
    return np.c_[rng.uniform(0, W, n), rng.uniform(0, H, n)].astype(np.float32)


def _right(p1, disp, dy):
    """x2 = x1 - disp, y2 = y1 + dy as float32, |x1 - x2| kept >= MIN_DISP after rounding."""
    x1 = p1[:, 0].astype(np.float64)
    x2 = (x1 - disp).astype(np.float32)
    away = np.where(disp > 0, -np.inf, np.inf).astype(np.float32)
    short = np.abs(x1 - x2.astype(np.float64)) < MIN_DISP
    x2 = np.where(short, np.nextafter(x2, away), x2).astype(np.float32)
    assert (np.abs(x1 - x2.astype(np.float64)) >= MIN_DISP).all()
    return np.c_[x2, (p1[:, 1].astype(np.float64) + dy).astype(np.float32)].astype(np.float32)


def _rectified(seed, bf, d_lo, d_hi, dy=0.0, n=N_BAND):
    rng = np.random.default_rng(seed)
    p1 = _left(rng, n)
    disp = rng.uniform(d_lo, d_hi, n)
    dyv = rng.uniform(-dy, dy, n) if dy else np.zeros(n)
    P1, P2 = stereo_projections(K, bf)
    return dict(P1=P1, P2=P2, p1=p1, p2=_right(p1, disp, dyv))


def _general(seed, n=N_BAND):
    """P2 = K [R | t], R = 2 deg yaw . 1 deg pitch, t = (-0.54, 0.01, 0.02), float32;
    points at Z in [3, 1200] m (log-uniform) through both cameras in float64."""
    rng = np.random.default_rng(seed)
    R = rot("y", np.radians(2.0)) @ rot("x", np.radians(1.0))
    t = np.array([-0.54, 0.01, 0.02])
    P1 = np.c_[K, np.zeros(3)].astype(np.float32)
    P2 = (K @ np.c_[R, t]).astype(np.float32)
    Z = np.exp(rng.uniform(np.log(3.0), np.log(1200.0), n))
    px = np.c_[rng.uniform(0, W, n), rng.uniform(0, H, n)]
    X = (np.linalg.inv(K) @ np.c_[px, np.ones(n)].T).T * Z[:, None]
    Xh = np.c_[X, np.ones(n)]
    u1, u2 = Xh @ P1.astype(np.float64).T, Xh @ P2.astype(np.float64).T
    return dict(P1=P1, P2=P2, p1=(u1[:, :2] / u1[:, 2:]).astype(np.float32),
                p2=(u2[:, :2] / u2[:, 2:]).astype(np.float32), Z=X[:, 2])


def _structured():
    """Hand-written points on the rectified KITTI rig: the principal point (exact
    zeros in A: the skipped rotations of dlt_jrot), the image corners, integer
    pixels, and x2 one float32 ulp below x1 - 0.01."""
    f = np.float32
    cx, cy = f(K[0, 2]), f(K[1, 2])
    rows = []
    for d in (0.5, 3.0, 20.0, -0.5):                      # x1 = cx, y1 = cy exactly
        rows.append((cx, cy, f(cx - f(d)), cy))
    for d in (0.25, 7.0):                                 # one of the two on the principal point
        rows.append((cx, f(100.5), f(cx - f(d)), f(100.5)))
        rows.append((f(300.25), cy, f(f(300.25) - f(d)), cy))
        rows.append((f(cx + f(d)), cy, cx, cy))           # x2 = cx: the zero in the right view's row
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):   # the four corners
        rows.append((f(x), f(y), f(x - 1), f(y)))
        rows.append((f(x), f(y), f(x - 0.0625), f(y)))
    for x, y, d in ((100, 50, 1), (100, 50, 2), (620, 185, 16), (1000, 300, 32), (7, 370, 5), (640, 1, -2)):
        rows.append((f(x), f(y), f(x - d), f(y)))         # integer pixels
    for x in (3.0, 100.37, 607.1928, 999.9, 1240.0, 0.0):  # x2 one ulp below x1 - 0.01
        x1 = f(x)
        rows.append((x1, f(77.7), np.nextafter(f(x1 - f(0.01)), f(-np.inf)), f(77.7)))
    a = np.array(rows, np.float32)
    assert (np.abs(a[:, 0].astype(np.float64) - a[:, 2]) >= MIN_DISP).all()
    P1, P2 = stereo_projections(K, KITTI_BF)
    return dict(P1=P1, P2=P2, p1=np.ascontiguousarray(a[:, :2]), p2=np.ascontiguousarray(a[:, 2:]))


BANDS = {
    "near": lambda: _rectified(101, KITTI_BF, 5.0, 32.0),
    "far": lambda: _rectified(102, KITTI_BF, 0.3, 3.0),
    "very_far": lambda: _rectified(103, KITTI_BF, 0.01, 0.3),
    "vertical": lambda: _rectified(104, KITTI_BF, 0.3, 3.0, dy=39.9),
    "behind_clear": lambda: _rectified(105, KITTI_BF, -3.0, -0.3),
    "behind_marginal": lambda: _rectified(106, KITTI_BF, -0.3, -0.01),
    "quarter": lambda: _rectified(107, STEREO_BF, 0.01, 3.0, dy=2.0),
    "general": lambda: _general(108),
    "structured": _structured,
}
_CACHE = {}


def band(name):
    """A band's inputs with the float64 reference and the oracle's result, computed
    once and shared (nothing writes to them)."""
    if name not in _CACHE:
        b = BANDS[name]()
        b["ref_h"], b["ref_x"] = ref_triangulate(b["P1"], b["P2"], b["p1"], b["p2"])
        b["ora_h"], b["ora_x"] = O.triangulate(b["P1"], b["P2"], b["p1"], b["p2"])
        for v in b.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = b
    return _CACHE[name]


def _zero_disparity():
    rng = np.random.default_rng(109)
    p1 = _left(rng, 64)
    P1, P2 = stereo_projections(K, KITTI_BF)
    return P1, P2, p1, p1.copy()


# ------------------------------------------------------------------ CPU: generator, reference, oracle
@pytest.mark.parametrize("name", list(BANDS))
def test_oracle_equals_float64_reference(name):
    """oracle/triangulate.c (OpenCV's SVD restated) against the float64 reference:
    0 ulp on every output, and the share of components the ulp bar leaves out.
    The structured set has components that are exactly 0 (a pixel on the principal
    point): rounding noise of 1e-17 there in either SVD, so its 0 ulp holds on the
    significant components, the project's bars on all, and no share is taken of
    hand-written points."""
    b = band(name)
    assert np.isfinite(b["ref_x"]).all() and np.isfinite(b["ora_x"]).all()
    excluded = 1.0 - significant(b["ref_x"]).mean()
    print(f"{name}: {len(b['p1'])} points, {100 * excluded:.2f} % of the components left out of the ulp bar")
    if name == "structured":
        assert int(ulp_distance(b["ora_h"], b["ref_h"])[significant(b["ref_h"])].max()) == 0
        assert int(ulp_distance(b["ora_x"], b["ref_x"])[significant(b["ref_x"])].max()) == 0
        assert np.allclose(b["ora_h"], b["ref_h"], rtol=0, atol=2e-7)
        assert np.allclose(b["ora_x"], b["ref_x"], rtol=1e-5, atol=1e-5)
        assert excluded > MAX_EXCLUDED   # it does hold exact zeros
    else:
        assert int(ulp_distance(b["ora_h"], b["ref_h"]).max()) == 0
        assert int(ulp_distance(b["ora_x"], b["ref_x"]).max()) == 0
        assert excluded <= MAX_EXCLUDED


def test_bands_exercise_the_keep_decision():
    """z > 0 in the reference: every point of the positive-disparity bands but a
    non-zero share of the vertical-mismatch one, no point of the behind bands."""
    for name in ("near", "far", "very_far", "quarter"):
        assert (band(name)["ref_x"][:, 2] > 0).all(), name
    behind = (band("vertical")["ref_x"][:, 2] <= 0).mean()
    print(f"vertical mismatch: {100 * behind:.2f} % of the points at z <= 0")
    assert 0 < behind < 0.02
    for name in ("behind_clear", "behind_marginal"):
        assert (band(name)["ref_x"][:, 2] <= 0).all(), name
    z = band("structured")["ref_x"][:, 2]
    assert 0 < (z <= 0).sum() < len(z)
    d = band("very_far")
    assert np.abs(d["p1"][:, 0].astype(np.float64) - d["p2"][:, 0]).min() >= MIN_DISP
    assert d["ref_x"][:, 2].max() > 10000    # beyond 10 km at KITTI's fx * b


def test_general_rig_reference_recovers_depth():
    """The reference on the float32-rounded pixels of the general rig against the
    true depth: what pixel rounding alone allows (the GPU test's bound)."""
    b = band("general")
    rel = np.abs(b["ref_x"][:, 2].astype(np.float64) - b["Z"]) / b["Z"]
    print(f"general rig, reference vs truth: median {np.median(rel):.3g}, max {rel.max():.3g}")
    assert np.median(rel) < 1e-4 and rel.max() < 2e-3


def test_ulp_distance_helper():
    f = np.float32
    a = np.array([1.0, -1.0, 0.0, 1e-45, 3.0], f)
    b = np.array([np.nextafter(f(1), f(2)), np.nextafter(f(-1), f(-2)), -0.0, -1e-45, 3.0], f)
    assert ulp_distance(a, b).tolist() == [1, 1, 0, 2, 0]
    assert ulp_distance(np.array([1.0], f), np.array([2.0], f)).tolist() == [1 << 23]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BANDS))
def test_triangulate_band(ctx, name):
    """svo_triangulate_points on one band against the float64 reference and the oracle.

    Measured on an MI355X: 0 ulp on every significant xyz component of every band
    (near, far, very far, vertical mismatch, both behind bands, quarter baseline,
    general rig, structured), and xyzw bit-equal to the reference on the eight
    random bands; only the structured set's exact-zero components differ (1e-16
    of rounding noise against 0, inside the 2e-7 bar)."""
    b = band(name)
    gh, gx = ctx.triangulate_points(b["P1"], b["P2"], b["p1"], b["p2"])
    sig = significant(b["ref_x"])
    ulp = ulp_distance(gx, b["ref_x"])
    print(f"{name}: worst ulp {int(ulp[sig].max())} on significant components ({int(ulp.max())} on all), "
          f"max |xyzw - ref| {np.abs(gh.astype(np.float64) - b['ref_h']).max():.3g}")
    assert np.isfinite(gh).all() and np.isfinite(gx).all()
    for rh, rx in ((b["ref_h"], b["ref_x"]), (b["ora_h"], b["ora_x"])):
        assert np.allclose(gh, rh, rtol=0, atol=2e-7)
        assert np.allclose(gx, rx, rtol=1e-5, atol=1e-5)
    assert np.array_equal(gx[:, 2] > 0, b["ref_x"][:, 2] > 0)
    assert int(ulp[sig].max()) <= ULP_BAR


@pytest.mark.gpu
def test_triangulate_general_rig_recovers_depth(ctx):
    """An arbitrary P2 is honoured (not only P2[0, 3]): the depth against the true
    Z is as good as the float32 rounding of the pixels allows -- the float64
    reference's own error on the same rounded pixels, with 1 % on top."""
    b = band("general")
    _, gx = ctx.triangulate_points(b["P1"], b["P2"], b["p1"], b["p2"])
    got = np.abs(gx[:, 2].astype(np.float64) - b["Z"]) / b["Z"]
    ref = np.abs(b["ref_x"][:, 2].astype(np.float64) - b["Z"]) / b["Z"]
    print(f"general rig vs truth: kernel median {np.median(got):.3g} max {got.max():.3g}; "
          f"reference median {np.median(ref):.3g} max {ref.max():.3g}")
    assert got.max() <= 1.01 * ref.max()
    assert np.median(got) <= 1.01 * np.median(ref)


@pytest.mark.gpu
def test_triangulate_zero_disparity_is_finite(ctx):
    """x2 == x1, y2 == y1 bitwise: the point at infinity. w is rounding noise around
    0, sign and size (1e-16 in the float64 reference, 1e-18 in the oracle on these
    points), so of xyz = h / w only the ray is defined: every output finite, |xyzw|
    within the project's 2e-7 of the reference's (w: of 0), and |xyz| scaled to unit
    length within its 1e-5."""
    P1, P2, p1, p2 = _zero_disparity()
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    gh, gx = ctx.triangulate_points(P1, P2, p1, p2)
    rh, rx = ref_triangulate(P1, P2, p1, p2)
    assert np.isfinite(gh).all() and np.isfinite(gx).all()
    assert np.allclose(np.abs(gh), np.abs(rh), rtol=0, atol=2e-7)

    def ray(x):
        x = np.abs(x.astype(np.float64))
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    assert np.allclose(ray(gx), ray(rx), rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_triangulate_prefix_sizes_bitwise(ctx):
    """The tail of a 256-thread block: every prefix of a band gives the bits of the
    full call (n = 1, around one wave, around one and two blocks)."""
    b = band("far")
    fh, fx = ctx.triangulate_points(b["P1"], b["P2"], b["p1"], b["p2"])
    for n in (1, 63, 64, 255, 256, 257, 513):
        h, x = ctx.triangulate_points(b["P1"], b["P2"], b["p1"][:n], b["p2"][:n])
        assert h.shape == (n, 4) and x.shape == (n, 3)
        assert np.array_equal(h.view(np.uint32), fh[:n].view(np.uint32)), n
        assert np.array_equal(x.view(np.uint32), fx[:n].view(np.uint32)), n


@pytest.mark.gpu
def test_triangulate_null_outputs_and_empty(ctx):
    """svo_triangulate_points called directly: xyzw = NULL, xyz = NULL, both NULL,
    and n = 0; the output that is asked for has the bits of the full call, and
    nothing is written behind it."""
    b = band("far")
    n = 513
    p1, p2 = np.ascontiguousarray(b["p1"][:n]), np.ascontiguousarray(b["p2"][:n])
    P1, P2 = (np.ascontiguousarray(P, np.float32).reshape(12) for P in (b["P1"], b["P2"]))
    fh, fx = ctx.triangulate_points(P1, P2, p1, p2)
    fp = C.POINTER(C.c_float)

    def call(cnt, want_h, want_x):
        h = np.full((n + 16, 4), -7.0, np.float32)
        x = np.full((n + 16, 3), -7.0, np.float32)
        rc = S.lib().svo_triangulate_points(ctx.handle, P1.ctypes.data_as(fp), P2.ctypes.data_as(fp),
                                            p1.ctypes.data_as(fp), p2.ctypes.data_as(fp), cnt,
                                            h.ctypes.data_as(fp) if want_h else None,
                                            x.ctypes.data_as(fp) if want_x else None)
        assert rc == 0
        return h, x

    for want_h, want_x in ((True, True), (False, True), (True, False), (False, False)):
        h, x = call(n, want_h, want_x)
        assert np.array_equal(h[:n].view(np.uint32), fh.view(np.uint32)) if want_h else (h == -7.0).all()
        assert np.array_equal(x[:n].view(np.uint32), fx.view(np.uint32)) if want_x else (x == -7.0).all()
        assert (h[n:] == -7.0).all() and (x[n:] == -7.0).all()
    h, x = call(0, True, True)
    assert (h == -7.0).all() and (x == -7.0).all()
    h0, x0 = ctx.triangulate_points(P1, P2, np.zeros((0, 2)), np.zeros((0, 2)))
    assert h0.shape == (0, 4) and x0.shape == (0, 3)
