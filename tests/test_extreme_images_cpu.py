"""CPU side of the extreme-image tests (tests/extreme_images.py): (1) the range each
case of test_lk_extremes_gpu.py / test_fast_extremes_gpu.py claims, from numpy's
int64 sums and the oracle -- never from the GPU -- so that an edit of a generator
that quietly leaves the extreme range fails here; (2) the oracle's EXACT sums
pinned at saturation against numpy, independently of the oracle; (3) the oracle's
FAST list against its own score map on content it has never been given."""
import numpy as np
import pytest

import extreme_images as X
import oracle as O
import starved_cases as C

TEMPORAL = dict(win=(21, 21), max_level=3, criteria=(3, 50, 1e-3), flags=O.LK_GET_MIN_EIGENVALS)
BOUND_21 = 441 * X.IX_MAX ** 2          # 7 341 062 400: sum Ix^2 of a 21 x 21 window, every |Ix| = 4080
SAD_BOUND = 2048 * X.IVAL_MAX           # 16 711 680 < 2^24 = 16 777 216
INT = slice(0, X.N_INT)                 # lk_points' features at integer positions


def _bmax(s):
    return np.maximum(np.abs(s.b1), np.abs(s.b2))


def _sums(name, win, pts=None):
    A, B = X.lk_pair(name)
    return X.lk_sums(A, B, X.lk_points()[INT] if pts is None else pts, win)


# ---------------------------------------------------------------- 1. the cases reach their range
def test_generators_are_what_they_say():
    s = X.stripes4(9, 13)
    assert s[0].tolist() == [0, 0, 255, 255, 0, 0, 255, 255, 0, 0, 255, 255, 0] and (s == s[0]).all()
    d = O.scharr(X.stripes4(40, 40)).astype(int)[:, 1:-1]
    assert (np.abs(d[..., 0]) == X.IX_MAX).all() and not d[..., 1].any()
    c = X.checker(8, 8, 2)
    assert c[0].tolist() == [0, 0, 255, 255, 0, 0, 255, 255] and c[2].tolist() == [255, 255, 0, 0, 255, 255, 0, 0]
    b = X.blocks(31, 45, 4, 3)
    assert set(np.unique(b)) == {0, 255} and b.shape == (31, 45)
    assert all((b[y:y + 4, x:x + 4] == b[y, x]).all() for y in range(0, 28, 4) for x in range(0, 44, 4))
    assert np.array_equal(X.blocks(31, 45, 4, 3), b) and not np.array_equal(X.blocks(31, 45, 4, 4), b)
    assert np.array_equal(X.inverse(b).astype(int) + b, np.full(b.shape, 255))
    n = X.noise(64, 64, 1)
    assert n.min() == 0 and n.max() == 255 and len(np.unique(n)) == 256
    assert set(np.unique(X.binary_noise(64, 64, 1))) == {0, 255}
    assert X.binarise(np.array([[0, 127, 128, 255]], np.uint8)).tolist() == [[0, 0, 255, 255]]
    A, B = X.pair(X.canvas(X.noise, 30, 40, 5), 3, -2)
    assert A.shape == B.shape == (30, 40) and np.array_equal(B[:-2, 3:], A[2:, :-3])  # next(x + 3, y - 2) = prev(x, y)
    sp = X.speckled(X.stripes4(60, 60), 1)
    assert 0 < (sp != X.stripes4(60, 60)).sum() < 200 and set(np.unique(sp)) <= {0, 12, 243, 255}


def test_stripes_reach_the_21x21_bound_exactly():
    """Every |Ix| = 4080: sum Ix^2 = 441 * 4080^2, the figure lk_multi's STEPS32 and
    tail asserts are written for; sum Iy^2 = 0, so the oracle rejects the feature at
    every level (status 0, no iteration)."""
    s = _sums("stripes4-shift1", (21, 21))
    assert s.a11.max() == BOUND_21 == 7341062400
    assert not s.a22.any() and not s.a12.any()
    assert _bmax(s).max() >= 2 ** 32  # 7.69e9 would be summed, were an iteration run
    A, B = X.lk_pair("stripes4-shift1")
    pts = X.lk_points()[INT]
    _, st, _, it = O.lk(A, B, pts, **TEMPORAL)
    assert not st.any() and not it.any()


@pytest.mark.parametrize("win,bit", [((11, 11), 31), ((15, 15), 31), ((21, 21), 32), ((31, 31), 32)])
def test_speckled_stripes_iterate_past_int32(win, bit):
    """The speckled stripes pass the minimum-eigenvalue test, so the right-hand side
    of the first iteration is really summed: features at integer positions whose
    |b| >= 2^31 (11 x 11, where sum Ix^2 <= 121 * 4080^2 < 2^31 cannot get there, and
    15 x 15) or >= 2^32 (21, 31) iterate at level 0 of a max_level 0 call."""
    A, B = X.lk_pair("stripes4-speckled-shift1")
    pts = X.lk_points()[INT]
    s = X.lk_sums(A, B, pts, win)
    _, _, _, it = O.lk(A, B, pts, win, 0, (3, 30, 1e-3), 0, level_iters=True)
    big = (_bmax(s) >= 2 ** bit) & (it[0] > 0)
    print(win, "features past 2^%d that iterate:" % bit, int(big.sum()), "max |b|", int(_bmax(s).max()))
    assert big.sum() >= 20
    if win != (11, 11):
        assert (s.a11[it[0] > 0] >= 2 ** bit).any()


def test_blocks_21x21_pass_2_31_in_one_feature():
    s = _sums("blocks2-shift(1,1)", (21, 21))
    both = (s.a11 >= 2 ** 31) & (_bmax(s) >= 2 ** 31)
    assert both.sum() >= 10, int(both.sum())


@pytest.mark.parametrize("win", [(31, 31), (32, 64)])
def test_blocks_31_and_larger_pass_2_32(win):
    """(32, 64) at k + 0.5, where an even window's samples are the pixels themselves."""
    pts = X.lk_points()[INT] + np.float32(0.5 if win[0] % 2 == 0 else 0.0)
    s = _sums("blocks2-shift(1,1)", win, pts)
    assert (s.a11 >= 2 ** 32).any() and (s.a22 >= 2 ** 32).any() and (_bmax(s) >= 2 ** 32).any()
    assert ((s.a11 >= 2 ** 32) & (_bmax(s) >= 2 ** 32)).sum() >= 10


def test_inverse_32x64_is_the_sad_bound():
    """prev 0 / 255, next its inverse, the window's top-left pixel an integer: every
    |J - I| x32 is 8160 and the 2048 of them sum to 16 711 680, 65 536 short of 2^24;
    the oracle's mean (no iteration: a COUNT 0 criterion, so the error is taken where
    the helper sums it) is 255 exactly."""
    A, B = X.lk_pair("blocks2-inverse")
    pts = X.half_points(X.LK_W, X.LK_H, 100, 3)
    s = X.lk_sums(A, B, pts, (32, 64))
    assert s.inside.all() and (s.sad == SAD_BOUND).all() and SAD_BOUND == 16711680 < 2 ** 24
    _, st, err, it = O.lk(A, B, pts, (32, 64), 0, (O.TERM_COUNT, 0, 0.0), 0)
    assert st.all() and not it.any() and (err == np.float32(255)).all()


@pytest.mark.parametrize("name", [n for n in X.LK_PAIRS if n.startswith("blocks") and "shift" in n])
def test_blocks_pairs_iterate_and_split(name):
    """In each shifted blocks pair at least half of the features (the border and
    outside set included) iterate at level 0 and both statuses occur (temporal call,
    exact and OpenCV's order)."""
    A, B = X.lk_pair(name)
    pts = X.lk_points()
    for acc in (O.ACC_EXACT, O.ACC_SSE):
        _, st, _, it = O.lk(A, B, pts, **TEMPORAL, acc=acc, level_iters=True)
        print(name, acc, "level-0 iterating", float((it[0] > 0).mean()), "status 1", float(st.mean()),
              "levels iterating", (it > 0).any(1).tolist())
        assert (it[0] > 0).mean() >= 0.5
        assert 0 < st.sum() < len(st)
    if name == "blocks2-shift(1,1)":
        assert (it > 0).any(1).all()  # all four levels iterate


@pytest.mark.parametrize("key", X.NOISE_IMAGES)
def test_noise_tiles_overflow_a_queue_pass(key):
    """More than 256 corners in one 64 x 32 tile (each wave's private queue then
    holds more than 64 of them: several compaction passes) and more than 1000
    adjacent corner pairs (NMS decisions between neighbours) at threshold 20."""
    _, c = O.fast_score(X.IMAGES[key](), 20)
    fullest, pairs = X.tile_stats(c)
    print(key, "fullest tile", fullest, "adjacent pairs", pairs, "corners", int(c.sum()))
    assert fullest > 256 and pairs > 1000


def test_binary_images_score_254_at_every_threshold():
    for key in ("binary-noise-320x240", "blocks3-320x240", "scene-binary-320x240"):
        img = X.IMAGES[key]()
        ref = O.fast_score(img, 1)
        assert ref[1].sum() > 1000 and (ref[0][ref[1] > 0] == 254).all()
        for t in (20, 100, 254):
            s, c = O.fast_score(img, t)
            assert np.array_equal(s, ref[0]) and np.array_equal(c, ref[1])
        assert not O.fast_score(img, 255)[1].any()
    for key in ("stripes4-161x121", "checker2-161x121"):
        assert not O.fast_score(X.IMAGES[key](), 1)[1].any()


@pytest.mark.parametrize("forward", [False, True], ids=["scene", "forward"])
@pytest.mark.parametrize("n", [64, 300])
def test_saturated_frontend_cases_track(n, forward):
    """test_frontend_saturated_gpu.py's cases, all three settings."""
    C.assert_saturated_conditions(C.saturated(n, forward))
    C.assert_saturated_conditions(C.saturated(n, forward, bucket=(50, 4)))
    if n == 300 and not forward:
        C.assert_saturated_conditions(C.saturated(n, acc=O.ACC_SSE))


# ---------------------------------------------------------------- 2. the oracle pinned at saturation
PIN_IMAGES = {"stripes4": lambda: X.stripes4(X.LK_H, X.LK_W), "checker2": lambda: X.checker(X.LK_H, X.LK_W, 2),
              "blocks2": lambda: X.blocks(X.LK_H, X.LK_W, 2, 12)}


@pytest.mark.parametrize("win", [(11, 11), (21, 21), (31, 31), (32, 64)], ids=str)
@pytest.mark.parametrize("image", list(PIN_IMAGES))
def test_oracle_exact_sums_pinned_against_numpy(image, win):
    """O.lk(acc=ACC_EXACT) at max_level 0 with MIN_EIGENVALS on an image against
    itself: err is, bit for bit, numpy's float32 evaluation of (A22 + A11 -
    sqrt((A11 - A22)^2 + 4 A12^2)) / (2 w h) from A = float32(int64 sum) * 2^-20 in
    oracle/lk.c's operation order, and the status is 0 exactly where that is below
    1e-4, the determinant below FLT_EPSILON, or the window outside the image. The
    features: integer positions, k + 0.5 (the even window's integer samples) and
    the border / outside set."""
    A = PIN_IMAGES[image]()
    pts = np.concatenate([X.lk_points()[INT], X.half_points(X.LK_W, X.LK_H, 100, 5), X.lk_points()[-407:]])
    s = X.lk_sums(A, A, pts, win)
    assert not s.b1.any() and not s.sad.any()
    me, D = X.min_eig_f32(s.a11, s.a12, s.a22, win)
    reject = (me < np.float32(1e-4)) | (D < X.FLT_EPSILON)
    _, st, err, it = O.lk(A, A, pts, win, 0, (3, 30, 0.01), O.LK_GET_MIN_EIGENVALS, acc=O.ACC_EXACT)
    want_err = np.where(s.inside, me, np.float32(0)).astype(np.float32)
    assert np.array_equal(err.view(np.uint32), want_err.view(np.uint32))
    assert np.array_equal(st, (s.inside & ~reject).astype(np.uint8))
    assert np.array_equal(it, st.astype(np.int32))  # b = 0: one iteration, then converged
    assert s.inside.sum() > 400 and not s.inside.all()
    if win == (21, 21) and image == "stripes4":
        assert s.a11.max() == BOUND_21 and reject[s.inside].all()
    if image != "stripes4":
        assert (st == 1).sum() > 300
        # (121 * 4080^2 < 2^31: an 11 x 11 window cannot get there)
        assert s.a11.max() >= {11: 0, 21: 2 ** 31, 31: 2 ** 32, 32: 2 ** 32}[win[0]]


# ---------------------------------------------------------------- 3. O.fast against O.fast_score
@pytest.mark.parametrize("t", [1, 20, 100, 254, 255])
@pytest.mark.parametrize("key", list(X.NOISE_IMAGES) + ["binary-noise-320x240", "blocks3-320x240"])
def test_oracle_fast_list_is_its_score_map(key, t):
    img = X.IMAGES[key]()
    s, c = O.fast_score(img, t)
    ys, xs = np.nonzero(c)  # raster order
    allk = O.fast(img, t, False)
    assert np.array_equal(allk, np.c_[xs, ys, np.zeros(len(xs))].astype(np.float32))
    p = np.pad(s.astype(np.int16), 1)
    h, w = s.shape
    nb = np.max([p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy], axis=0)
    keep = (c > 0) & (s > nb)
    ys, xs = np.nonzero(keep)
    assert np.array_equal(O.fast(img, t, True), np.c_[xs, ys, s[ys, xs]].astype(np.float32))
