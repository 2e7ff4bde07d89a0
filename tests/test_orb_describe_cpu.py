"""ORB descriptors and the Hamming matcher on a CPU-only host: the library's host
entry points (svo_orb_umax, svo_orb_default_pattern, svo_match_filter) against the
numpy restatement (tests/orb_describe_reference.py), and self-checks of the
restatement that need no library: a quarter turn of the image turns the
descriptor's sampling exactly, and a ramp has the direction (1, 0).
"""
import ctypes as C

import numpy as np
import pytest

import orb_describe_reference as R

UMAX_31 = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def test_symbols_declared_and_bound():
    import svo_amd as S
    new = ["svo_orb_default_pattern", "svo_orb_umax", "svo_orb_compute", "svo_orb_detect_and_compute",
           "svo_orb_blur_level", "svo_match_hamming", "svo_match_filter"]
    assert set(new) <= set(S.SYMBOLS)
    lib = C.CDLL(S.lib_path())
    for name in new:
        assert hasattr(lib, name), name


def test_umax_known_answer_and_restatement():
    import svo_amd as S
    assert S.orb_umax(31).tolist() == UMAX_31
    assert R.umax(31).tolist() == UMAX_31
    assert np.array_equal(S.orb_umax(15), R.umax(15))
    assert len(S.orb_umax(15)) == 8
    # the raw entry: cap below the table writes cap entries and reports the full length
    out = np.full(8, -7, np.int32)
    n = C.c_int(-1)
    assert S.lib().svo_orb_umax(31, out.ctypes.data_as(C.POINTER(C.c_int)), 4, C.byref(n)) == 0
    assert n.value == 16 and out[:4].tolist() == UMAX_31[:4] and (out[4:] == -7).all()


@pytest.mark.parametrize("patch", [31, 15])
def test_default_pattern_matches_mwc_restatement(patch):
    import svo_amd as S
    got = S.orb_default_pattern(patch)
    assert got.shape == (512, 2) and got.dtype == np.int8
    assert np.array_equal(got, R.default_pattern(patch))
    hp = patch // 2
    assert got.min() >= -hp and got.max() <= hp
    assert got.min() == -hp and got.max() == hp  # the range is reached at both ends


@pytest.mark.parametrize("patch", [30, 16, 4, 3, 33, 0, -31])
def test_default_pattern_and_umax_reject_bad_sizes(patch):
    import svo_amd as S
    buf = np.full(1024, 99, np.int8)
    assert S.lib().svo_orb_default_pattern(patch, buf.ctypes.data_as(C.POINTER(C.c_int8))) == -1
    assert (buf == 99).all()
    u = np.full(16, 99, np.int32)
    n = C.c_int(-5)
    assert S.lib().svo_orb_umax(patch, u.ctypes.data_as(C.POINTER(C.c_int)), 16, C.byref(n)) == -1
    assert (u == 99).all() and n.value == -5
    with pytest.raises(S.SvoError):
        S.orb_default_pattern(patch)


# ------------------------------------------------------------------ match filter
def _filter_both(idx, dist, tq, ratio):
    import svo_amd as S
    got = S.match_filter(idx, dist, tq, ratio)
    exp = R.match_filter(np.asarray(idx).reshape(-1, 2), np.asarray(dist).reshape(-1, 2),
                         None if tq is None else np.asarray(tq).reshape(-1, 2), ratio)
    assert np.array_equal(got, exp)
    return got.tolist()


def test_match_filter_ratio_boundary_is_rejected():
    # 40 * 100 == 80 * 50: rejected; 39 * 100 < 80 * 50: kept; 41: rejected
    idx = [[0, 1], [1, 0], [2, 0]]
    dist = [[40, 50], [39, 50], [41, 50]]
    assert _filter_both(idx, dist, None, 80) == [[1, 1]]
    # distance 0 against 0: 0 < 0 is false
    assert _filter_both([[0, 1]], [[0, 0]], None, 80) == []
    assert _filter_both([[0, 1]], [[0, 1]], None, 80) == [[0, 0]]
    # ratio 100: strictly better than the second only
    assert _filter_both([[0, 1], [1, 0]], [[7, 7], [6, 7]], None, 100) == [[1, 1]]


def test_match_filter_missing_neighbours():
    idx = [[3, -1], [-1, -1], [0, 2]]
    dist = [[10, 257], [257, 257], [10, 200]]
    # with the ratio test a missing second neighbour rejects; without it only a missing first does
    assert _filter_both(idx, dist, None, 80) == [[2, 0]]
    assert _filter_both(idx, dist, None, 0) == [[0, 3], [2, 0]]


def test_match_filter_cross_check_drops_non_mutual_pairs():
    idx = [[0, 1], [0, 1], [1, 0]]          # queries 0 and 1 both choose train 0
    dist = [[5, 90], [9, 90], [4, 90]]
    tq = [[0, 1], [2, 0]]                   # train 0 chooses query 0, train 1 chooses query 2
    assert _filter_both(idx, dist, None, 80) == [[0, 0], [1, 0], [2, 1]]
    assert _filter_both(idx, dist, tq, 80) == [[0, 0], [2, 1]]
    assert _filter_both(idx, dist, tq, 0) == [[0, 0], [2, 1]]


def test_match_filter_cap_and_errors():
    import svo_amd as S
    i32p = C.POINTER(C.c_int)
    idx = np.array([[0, 1], [1, 0], [2, 0], [1, 2]], np.int32)
    dist = np.array([[1, 90], [2, 90], [3, 90], [4, 90]], np.int32)
    pairs = np.full((4, 2), -9, np.int32)
    n = C.c_int(-1)
    f = S.lib().svo_match_filter
    assert f(idx.ctypes.data_as(i32p), dist.ctypes.data_as(i32p), 4, None, 3, 80, pairs.ctypes.data_as(i32p), 2,
             C.byref(n)) == 0
    assert n.value == 4  # the full count
    assert pairs.tolist() == [[0, 0], [1, 1], [-9, -9], [-9, -9]]
    assert S.match_filter(idx, dist, None, 80, cap=3).tolist() == [[0, 0], [1, 1], [2, 2]]
    # nq = 0
    assert f(None, None, 0, None, 0, 80, pairs.ctypes.data_as(i32p), 2, C.byref(n)) == 0 and n.value == 0
    # nothing written on errors: a negative count, a negative ratio, an index past nt
    pairs[:] = -9
    n = C.c_int(-1)
    for nq, nt, ratio in ((-1, 3, 80), (4, -1, 80), (4, 3, -1), (4, 2, 80)):
        assert f(idx.ctypes.data_as(i32p), dist.ctypes.data_as(i32p), nq, None, nt, ratio,
                 pairs.ctypes.data_as(i32p), 4, C.byref(n)) == -1
    assert (pairs == -9).all() and n.value == -1


def test_knn2_argmin_form_is_the_upward_scan():
    rng = np.random.default_rng(3)
    t = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    t[7] = t[2]
    t[30] = t[2]
    t[31] = t[5]
    q = np.concatenate([t[[2, 5, 31]], rng.integers(0, 256, (20, 32), dtype=np.uint8)])
    q[4] = t[2] ^ np.eye(1, 32, 3, dtype=np.uint8)[0]  # one bit from three equal rows
    for nt in (0, 1, 2, 40):
        idx, dist = R.knn2(q, t[:nt])
        d = R.hamming(q, t[:nt]) if nt else np.zeros((len(q), 0), np.int32)
        for i in range(len(q)):
            i1, i2, d1, d2 = R.knn2_scan(d[i])
            assert (idx[i].tolist(), dist[i].tolist()) == ([i1, i2], [d1, d2]), (nt, i)
    idx, dist = R.knn2(q, t)
    assert idx[0].tolist() == [2, 7] and dist[0].tolist() == [0, 0]  # ties: the lowest indices, in order
    assert idx[4].tolist() == [2, 7] and dist[4].tolist() == [1, 1]


# ------------------------------------------------------------------ restatement self-checks
def _texture(w, h, seed):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4), dtype=np.uint8)
    return np.kron(b, np.ones((4, 4), np.uint8))[:h, :w].copy()


def test_blur_weights_and_border():
    assert R.BLUR_W.sum() == 256 and R.BLUR_W.tolist() == R.BLUR_W[::-1].tolist()
    flat = np.full((9, 13), 201, np.uint8)
    assert (R.blur(flat) == 201).all()  # the weights sum to 256 on both passes, border included
    img = _texture(23, 11, 1)
    b = R.blur(img)
    # REFLECT_101 by hand at a corner pixel
    taps = [3, 2, 1, 0, 1, 2, 3]
    hor = [sum(int(w) * int(img[r, c]) for w, c in zip(R.BLUR_W, taps)) for r in taps]
    assert b[0, 0] == (sum(int(w) * v for w, v in zip(R.BLUR_W, hor)) + 32768) >> 16
    assert R.reflect101(np.array([-3, -1, 0, 4, 5, 7]), 5).tolist() == [3, 1, 0, 4, 3, 1]
    assert R.reflect101(np.array([-9, -4, 5, 8]), 3).tolist() == [1, 0, 1, 0]   # narrower than the kernel
    assert R.reflect101(np.array([-2, 0, 3]), 1).tolist() == [0, 0, 0]
    assert R.blur(img[:1, :1])[0, 0] == img[0, 0]


@pytest.mark.parametrize("patch", [31, 15])
def test_descriptor_turns_with_the_image(patch):
    """np.rot90 (counterclockwise): pixel (x, y) of a w-wide image goes to (y, w - 1 - x).
    The moments swap exactly (m10' = m01, m01' = -m10), so c' = s and s' = -c; for
    an axis-aligned direction (0 or +-1) the steered offsets are the pattern's own
    points turned, and the symmetric blur commutes with the turn: same samples,
    same bits. A general direction turns exactly too (the products are the same
    numbers in the other coordinate)."""
    img = _texture(96, 80, 5)
    h, w = img.shape
    rot = np.rot90(img).copy()
    bl, blr = R.blur(img), R.blur(rot)
    assert np.array_equal(np.rot90(bl), blr)
    pat = R.default_pattern(patch)
    rch = R.reach(patch)
    rng = np.random.default_rng(0)
    for _ in range(12):
        x = int(rng.integers(rch, w - rch))
        y = int(rng.integers(rch, h - rch))
        m10, m01 = R.moments(img, x, y, patch)
        r10, r01 = R.moments(rot, y, w - 1 - x, patch)
        assert (r10, r01) == (m01, -m10)
        d0, a0 = R.describe_at(img, bl, x, y, pat, patch)
        d1, a1 = R.describe_at(rot, blr, y, w - 1 - x, pat, patch)
        assert np.array_equal(d0, d1)
        assert abs(((float(a0) - float(a1)) % 360.0) - 90.0) < 1e-3
        assert d0.any()


def test_ramp_has_direction_one_zero():
    x = np.arange(80, dtype=np.int64)
    img = np.broadcast_to((20 + 2 * x).astype(np.uint8), (64, 80)).copy()  # flat plus a ramp along x
    m10, m01 = R.moments(img, 40, 32, 31)
    assert m01 == 0 and m10 > 0
    c, s, a = R.direction(m10, m01)
    assert (c, s) == (1.0, 0.0) and a == 0
    # a constant patch: no gradient at all
    flat = np.full((64, 80), 77, np.uint8)
    assert R.moments(flat, 40, 32, 31) == (0, 0)
    assert R.direction(0, 0) == (1.0, 0.0, np.float32(0))
    d, _ = R.describe_at(flat, R.blur(flat), 40, 32, R.default_pattern(31), 31)
    assert not d.any()
    # the ramp turned: straight down is (0, 1), 90 degrees
    c, s, a = R.direction(*R.moments(img.T.copy(), 32, 40, 31))
    assert (c, s) == (0.0, 1.0) and a == 90


def test_validity_and_level_pixel():
    lv = [np.zeros((60, 70), np.uint8)]
    ls = np.array([1.0], np.float32)
    kp = np.array([[21, 21], [48, 38], [20, 30], [49, 30], [30, 39], [20.5, 21.5], [21.5, 22.5]], np.float32)
    _, ang, valid = R.compute(lv, lv, ls, kp, np.zeros(len(kp), int), 31)
    # 20.5 rounds to 20 (outside), 21.5 to 22 and 22.5 to 22 (inside): half to even
    assert valid.tolist() == [1, 1, 0, 0, 0, 0, 1]
    assert (ang[valid == 0] == -1).all()
    assert R.level_pixel(np.float32(100.0), np.float32(1.2)) == 83


def test_relocalisation_case_reaches_its_recorded_figures():
    """The restatement's chain alone (the oracle's solvePnPRansac for the pose) on the
    scene tests/test_orb_describe_gpu.py relocalises in: the figures recorded in
    orb_describe_cases.RELOC_MEASURED and DESIGN.md section 3d, from which the GPU
    test's bars are derived, and at least 30 pairs."""
    import oracle as O
    import orb_describe_cases as K
    d = K.reloc_inputs()
    sc, t = d["scene"], K.RELOC["t"]
    pairs = K.reloc_pairs()
    m = K.RELOC_MEASURED
    assert len(pairs) == m["pairs"] >= 30
    assert abs(np.degrees(sc.roll_rate * sc.phase(t)) - 15.0) < 1e-9  # a visible turn in the image plane
    share = K.match_share(sc, t, d["xyz"], d["cur"]["kp"][:, :2], pairs)
    res = O.solve_pnp_ransac(d["xyz"][pairs[:, 1]], d["cur"]["kp"][pairs[:, 0], :2], sc.K)
    assert res[0]
    rot, trans = K.pose_error(sc, t, res[1], res[2])
    assert abs(share - m["share"]) < 1e-3 and abs(rot - m["rot_deg"]) < 1e-3 and abs(trans - m["trans_m"]) < 1e-4
