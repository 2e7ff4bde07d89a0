"""SQPnP's sufficient statistics on the device (svo_sqpnp_stats -> suffstats_kernel
-> suffstats_block, the block the keyframe's compaction runs too): bit for bit
against the float64 restatement of its arithmetic and reduction order
(sqpnp_stats_reference.stats_f64), and against longdouble sums of the same terms
within the summation bound."""
import numpy as np
import pytest

import svo_amd as S
from sqpnp_stats_reference import KITTI_K as K, pack_bits, problem, stats_f64, stats_longdouble

pytestmark = pytest.mark.gpu

CAP, WORDS_CAP = 1024, 33
# around a wave, the block (one point per thread, then two) and several rounds; two launches
LAUNCHES = [[0, 1, 63, 64, 65], [255, 256, 257, 1000]]
PATTERNS = {"all": lambda n: np.ones(n, bool), "none": lambda n: np.zeros(n, bool),
            "every third": lambda n: np.arange(n) % 3 == 0, "last only": lambda n: np.arange(n) == n - 1}
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _sequence(n, inl, seed):
    """n points (a seventh of them behind the camera) of which `inl` are the fitted
    set; NaN at every other slot and beyond the count; every bit at or above n set
    at random (the last word's among them)."""
    rng = np.random.default_rng(seed)
    nb = n // 7
    X, uv, _, _ = problem(max(n - nb, 1), nb, seed)
    order = rng.permutation(n)
    obj = np.full((CAP, 3), np.nan, np.float32)
    img = np.full((CAP, 2), np.nan, np.float32)
    obj[:n][inl], img[:n][inl] = X[:n][order][inl], uv[:n][order][inl]
    garbage = rng.random(32 * WORDS_CAP) < 0.5
    garbage[:n] = inl
    if n % 32:
        garbage[n: 32 * (n // 32 + 1)] = True  # the word the count ends in: every bit above it
    return obj, img, pack_bits(garbage, WORDS_CAP)


def _launch(ctx, counts, pattern, seed):
    seqs = [_sequence(n, PATTERNS[pattern](n), seed + s) for s, n in enumerate(counts)]
    obj, img, bits = (np.stack([q[k] for q in seqs]) for k in range(3))
    return obj, img, bits, ctx.sqpnp_stats(obj, img, counts, bits, K)


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_stats_bit_for_bit_and_within_the_summation_bound(ctx, pattern):
    worst = 0.0
    for li, counts in enumerate(LAUNCHES):
        obj, img, bits, got = _launch(ctx, counts, pattern, 100 * li + 7)
        assert got.shape == (len(counts), 40)
        for s, n in enumerate(counts):
            ref = stats_f64(obj[s], img[s], n, bits[s], K)
            assert np.array_equal(got[s].view(np.uint64), ref.view(np.uint64)), \
                f"{pattern} n={n}: stats {np.nonzero(got[s] != ref)[0]} differ from the float64 restatement"
            ld, mag, n_in = stats_longdouble(obj[s], img[s], n, bits[s], K)
            assert n_in == int(PATTERNS[pattern](n).sum()) and got[s, 0] == n_in
            if n_in == 0:
                assert np.array_equal(got[s].view(np.uint64), np.zeros(40, np.uint64))
                continue
            bound = (n_in + 8) * np.longdouble(U) * mag
            ratio = float((np.abs(got[s].astype(np.longdouble) - ld) / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{pattern} n={n}: {ratio} of the summation bound"
        again = ctx.sqpnp_stats(obj, img, counts, bits, K)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    print(f"{pattern}: largest |stat - longdouble| / ((n_in + 8) 2^-53 sum|term|) = {worst:.3g}")


def test_a_sequence_does_not_depend_on_its_neighbours(ctx):
    """The same sequence alone and in the last slot of a launch: the same bits."""
    obj, img, bits, got = _launch(ctx, LAUNCHES[1], "every third", 107)
    alone = ctx.sqpnp_stats(obj[3:], img[3:], [1000], bits[3:], K)
    assert np.array_equal(alone.view(np.uint64), got[3:].view(np.uint64))


def test_refused_arguments_write_nothing(ctx):
    import ctypes as C
    obj, img, bits, _ = _launch(ctx, [40, 50], "all", 3)
    Kf = np.ascontiguousarray(K.ravel())
    f32p, f64p, i32p, u32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int, C.c_uint32))

    def call(**kw):
        out = np.full((2, 40), -7.0)
        a = dict(ctx=ctx.handle, obj=obj.ctypes.data_as(f32p), img=img.ctypes.data_as(f32p), counts=[40, 50], S=2,
                 cap=CAP, bits=bits.ctypes.data_as(u32p), words_cap=WORDS_CAP, K=Kf.ctypes.data_as(f64p),
                 stats=out.ctypes.data_as(f64p))
        a.update(kw)
        cn = None if a["counts"] is None else np.ascontiguousarray(a["counts"], np.int32)
        rc = S.lib().svo_sqpnp_stats(a["ctx"], a["obj"], a["img"], None if cn is None else cn.ctypes.data_as(i32p),
                                     a["S"], a["cap"], a["bits"], a["words_cap"], a["K"], a["stats"])
        if rc != 0 or a["S"] == 0:
            assert (out == -7.0).all()
        return rc

    assert call() == 0
    assert call(counts=[40, -1]) == -1
    assert call(counts=[CAP + 1, 50]) == -1
    assert call(words_cap=1) == -1
    assert call(S=-1) == -1
    for name in ("ctx", "obj", "img", "counts", "bits", "K", "stats"):
        assert call(**{name: None}) == -1, name
    assert call(S=0) == 0
