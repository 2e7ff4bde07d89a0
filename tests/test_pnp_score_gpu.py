"""The batched front end's RANSAC scoring kernel by itself (svo_pnp_score ->
pnp_score_kernel: one block per hypothesis and sequence, a strided loop over the
points, per-wave ballots into bit words, one count per row, rows at a fixed
stride) against the oracle's projectPoints + findInliers (O.pnp_residuals): the
inlier bits and counts of every scored row are the oracle's, and every row and
word the kernel must leave alone keeps the caller's fill."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import svo_amd as S
from sqpnp_stats_reference import KITTI_K as K, problem, unpack_bits

pytestmark = pytest.mark.gpu

FILL_BITS, FILL_CNT = 0xDEADBEEF, -77
CAP, WORDS_CAP, STRIDE = 640, 22, 16  # above every count / (600 + 31) // 32 = 19 / the front end's chunk
# every count around a word, a wave's two words and the block, an empty sequence between live ones
RAGGED = {"a": [1, 0, 31, 32, 33, 600], "b": [63, 64, 65, 255, 256, 257]}


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _fills(nseq, stride=STRIDE, words_cap=WORDS_CAP):
    return (np.full((nseq, stride, words_cap), FILL_BITS, np.uint32), np.full((nseq, stride), FILL_CNT, np.int32))


def _batch(counts, seed):
    """Sequences of counts[s] points (some behind the camera, a fifth moved off their
    pixel), NaN beyond the count, and STRIDE hypotheses each around the true pose."""
    rng = np.random.default_rng(seed)
    nseq = len(counts)
    obj = np.full((nseq, CAP, 3), np.nan, np.float32)
    img = np.full((nseq, CAP, 2), np.nan, np.float32)
    hyps = np.zeros((nseq, STRIDE, 12))
    for s, n in enumerate(counts):
        nb = n // 7
        X, uv, R, t = problem(max(n - nb, 1), nb, seed * 100 + s)
        X, uv = X[:n], uv[:n].copy()
        off = rng.random(n) < 0.2
        uv[off] += rng.uniform(5, 40, (int(off.sum()), 2)).astype(np.float32)
        order = rng.permutation(n)
        obj[s, :n], img[s, :n] = X[order], uv[order]
        rv = O.rodrigues_inv(R)
        for j in range(STRIDE):
            hyps[s, j, :9] = O.rodrigues(rv + rng.normal(0, 0.0015 * (j % 5), 3)).ravel()
            hyps[s, j, 9:] = t + rng.normal(0, 0.01 * (j % 4), 3)
    return obj, img, np.array(counts, np.int32), hyps


def _check(counts, obj, img, hyps, m, bits, cnt, thresh2=64.0):
    for s, n in enumerate(counts):
        words = (n + 31) // 32
        assert (bits[s, m:] == FILL_BITS).all() and (cnt[s, m:] == FILL_CNT).all(), f"seq {s}: rows >= m written"
        assert (bits[s, :, words:] == FILL_BITS).all(), f"seq {s}: words past the count written"
        if n == 0:
            assert (cnt[s, :m] == 0).all() and (bits[s] == FILL_BITS).all()
            continue
        _, mask, rc = O.pnp_residuals(obj[s, :n], img[s, :n], hyps[s, :m], K, thresh2)
        for j in range(m):
            assert np.array_equal(unpack_bits(bits[s, j], n), mask[j]), f"seq {s} row {j}: inlier bits differ"
            # (the bits of the last word above the count are clear: ballots of lanes past n)
            assert np.array_equal(unpack_bits(bits[s, j], 32 * words)[n:], np.zeros(32 * words - n, np.uint8))
        assert np.array_equal(cnt[s, :m], rc), f"seq {s}: counts {cnt[s, :m]} != {rc}"


@pytest.mark.parametrize("m", [1, 3, 16])
@pytest.mark.parametrize("half", ["a", "b"])
def test_ragged_batch_matches_oracle(ctx, half, m):
    counts = RAGGED[half]
    obj, img, n, hyps = _batch(counts, seed=11 if half == "a" else 12)
    bits, cnt = _fills(len(counts))
    ctx.pnp_score(obj, img, n, hyps, m, K, 64.0, bits, cnt)
    _check(counts, obj, img, hyps, m, bits, cnt)
    # the scene is not trivial: among the scored rows some points are in and some out
    live = [s for s, c in enumerate(counts) if c >= 31]
    assert all(0 < cnt[s, 0] < counts[s] for s in live)
    bits2, cnt2 = _fills(len(counts))
    ctx.pnp_score(obj, img, n, hyps, m, K, 64.0, bits2, cnt2)
    assert np.array_equal(bits, bits2) and np.array_equal(cnt, cnt2)


def test_hand_made_rows(ctx):
    """err exactly at thresh2 and one float above it, a depth of exactly 0 (the z ?
    1 / z : 1 rule), a point behind the camera, a NaN pixel; the identity, a NaN
    translation and the all-zero hypothesis the front end pads rounds with."""
    fx, fy = K[0, 0], K[1, 1]
    cx, cy = np.float32(K[0, 2]), np.float32(K[1, 2])
    at = np.float32(cx + np.float32(8))
    assert float(at) - float(cx) == 8.0
    above = np.nextafter(at, np.float32(np.inf))
    X = np.array([[0, 0, 1], [0, 0, 1], [1, 2, 0], [1, 2, 0], [0.5, 0.2, -5], [0.3, 0.1, 9], [3, 4, 5]], np.float32)
    uv = np.array([[at, cy], [above, cy], [cx, cy],
                   [np.float32(1 * fx + K[0, 2]), np.float32(2 * fy + K[1, 2])],  # where the depth-0 rule puts it
                   [np.float32(0.5 / -5 * fx + K[0, 2]), np.float32(0.2 / -5 * fy + K[1, 2])],
                   [np.nan, cy], [cx, cy]], np.float32)
    n = len(X)
    eye = np.r_[np.eye(3).ravel(), 0, 0, 0]
    hyps = np.zeros((1, STRIDE, 12))
    hyps[0, 0] = eye
    hyps[0, 1] = np.r_[np.eye(3).ravel(), np.nan, 0, 0]
    hyps[0, 2] = 0
    obj = np.full((1, 40, 3), np.nan, np.float32)
    img = np.full((1, 40, 2), np.nan, np.float32)
    obj[0, :n], img[0, :n] = X, uv
    bits, cnt = _fills(1, words_cap=3)
    ctx.pnp_score(obj, img, [n], hyps, 3, K, 64.0, bits, cnt)
    err, mask, rc = O.pnp_residuals(X, uv, hyps[0, :3], K, 64.0)
    assert err[0, 0] == 64.0 and abs(err[0, 1] - 64.00098) < 1e-5 and err[0, 2] > 2.5e6  # the oracle on these rows
    got = np.array([unpack_bits(bits[0, j], n) for j in range(3)])
    print("hand-made rows: oracle err", err[0], "mask", mask.tolist(), "device", got.tolist())
    assert np.array_equal(got, mask) and np.array_equal(cnt[0, :3], rc)
    assert got[0].tolist() == [1, 0, 0, 1, 1, 0, 0]  # identity: at the threshold in, one float above out, ...
    assert cnt[0, 1] == 0                              # NaN translation: nothing
    assert got[2].tolist() == [1, 0, 1, 0, 0, 0, 1]    # zero hypothesis: every point lands on (cx, cy)
    assert (bits[0, 3:] == FILL_BITS).all() and (bits[0, :, 1:] == FILL_BITS).all() and (cnt[0, 3:] == FILL_CNT).all()


def test_matches_the_standalone_kernel(ctx):
    """One ordinary 600-point problem: the same mask and counts as svo_pnp_residuals
    (pnp_residual_kernel, the standalone solvePnPRansac's scoring)."""
    from test_gpu_parity import _pnp_problem
    sc, X, uv, _ = _pnp_problem(n=600, seed=4)
    rng = np.random.default_rng(5)
    hyps = np.zeros((1, STRIDE, 12))
    rv = O.rodrigues_inv(sc.R(3))  # the problem's pose (t = 0), more and more disturbed
    for j in range(STRIDE):
        hyps[0, j] = np.r_[O.rodrigues(rv + rng.normal(0, 0.0008 * j, 3)).ravel(), rng.normal(0, 0.004 * j, 3)]
    obj = np.full((1, CAP, 3), np.nan, np.float32)
    img = np.full((1, CAP, 2), np.nan, np.float32)
    obj[0, :600], img[0, :600] = X, uv
    bits, cnt = _fills(1)
    ctx.pnp_score(obj, img, [600], hyps, STRIDE, sc.K, 64.0, bits, cnt)
    _, mask, rc = ctx.pnp_residuals(X, uv, hyps[0], sc.K, 64.0, want_err=False)
    assert np.array_equal(np.array([unpack_bits(bits[0, j], 600) for j in range(STRIDE)]), mask)
    assert np.array_equal(cnt[0], rc) and 0 < rc.min() and rc.max() < 600 and len(set(rc.tolist())) > 4


def test_refused_arguments_write_nothing(ctx):
    obj, img, n, hyps = _batch([40, 50], seed=13)
    Kf = np.ascontiguousarray(K.ravel())
    f32p, f64p, i32p, u32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int, C.c_uint32))

    def call(**kw):
        bits, cnt = _fills(2)
        a = dict(ctx=ctx.handle, obj=obj.ctypes.data_as(f32p), img=img.ctypes.data_as(f32p), counts=n, S=2, cap=CAP,
                 hyps=hyps.ctypes.data_as(f64p), m=3, m_stride=STRIDE, K=Kf.ctypes.data_as(f64p),
                 bits=bits.ctypes.data_as(u32p), words_cap=WORDS_CAP, cnt=cnt.ctypes.data_as(i32p))
        a.update(kw)
        cn = None if a["counts"] is None else np.ascontiguousarray(a["counts"], np.int32)
        rc = S.lib().svo_pnp_score(a["ctx"], a["obj"], a["img"], None if cn is None else cn.ctypes.data_as(i32p),
                                   a["S"], a["cap"], a["hyps"], a["m"], a["m_stride"], a["K"], 64.0, a["bits"],
                                   a["words_cap"], a["cnt"])
        if rc != 0 or a["S"] == 0:
            assert (bits == FILL_BITS).all() and (cnt == FILL_CNT).all()
        return rc

    assert call() == 0
    assert call(counts=[40, -1]) == -1
    assert call(counts=[CAP + 1, 50]) == -1
    assert call(m=STRIDE + 1) == -1
    assert call(m=-1) == -1
    assert call(words_cap=1) == -1  # 50 points need 2 words
    assert call(S=-1) == -1
    for name in ("ctx", "obj", "img", "counts", "hyps", "K", "bits", "cnt"):
        assert call(**{name: None}) == -1, name
    assert call(S=0) == 0  # nothing to score: valid, nothing written
