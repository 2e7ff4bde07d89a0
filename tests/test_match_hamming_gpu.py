"""svo_match_hamming on the GPU against the numpy restatement
(tests/orb_describe_reference.py knn2): best and second-best train index and
distance, exact in all four outputs. Counts around the kernel's 256-query blocks
and 256-descriptor train tiles, empty and single-row sets, ties (lowest index),
the largest distance, and a batch with strides above the counts whose padding
must stay untouched.
"""
import ctypes as C

import numpy as np
import pytest

import orb_describe_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import svo_amd as S
    return S.Context(0)


def _rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _check(ctx, q, t):
    idx, dist = ctx.match_hamming(q, t)
    ei, ed = R.knn2(q, t)
    assert idx.shape == ei.shape and idx.dtype == np.int32 and dist.dtype == np.int32
    assert np.array_equal(idx, ei), np.argwhere(idx != ei)[:4]
    assert np.array_equal(dist, ed), np.argwhere(dist != ed)[:4]
    return idx, dist


@pytest.mark.parametrize("nq,nt", [(0, 5), (5, 0), (1, 1), (3, 1), (64, 64), (65, 257), (300, 1000),
                                   (256, 256), (257, 512), (2, 513)])
def test_gpu_match_random(ctx, nq, nt):
    rng = np.random.default_rng(1000 * nq + nt)
    idx, dist = _check(ctx, _rand(rng, nq), _rand(rng, nt))
    if nt == 0:
        assert (idx == -1).all() and (dist == 257).all()
    if nt == 1 and nq:
        assert (idx[:, 0] == 0).all() and (idx[:, 1] == -1).all() and (dist[:, 1] == 257).all()


def test_gpu_match_close_descriptors(ctx):
    """Queries a few bits from train rows: distances small and full of ties, unlike
    random descriptors (which sit near 128)."""
    rng = np.random.default_rng(5)
    t = _rand(rng, 700)
    q = t[rng.integers(0, 700, 300)].copy()
    flips = rng.integers(0, 256, (300, 3))
    for i in range(300):
        for b in flips[i][: i % 4]:
            q[i, b // 8] ^= np.uint8(1 << (b % 8))
    idx, dist = _check(ctx, q, t)
    assert (dist[:, 0] <= 3).all() and (dist[:, 0] == 0).any()


def test_gpu_match_ties_go_to_the_lowest_index(ctx):
    rng = np.random.default_rng(9)
    t = _rand(rng, 600)
    t[300] = t[10]      # across a train tile
    t[599] = t[10]
    t[11] = t[10]
    t[500] = t[258]
    near = t[10].copy()
    near[31] ^= 0x80    # one bit from rows 10, 11, 300 and 599
    q = np.stack([t[10], t[258], near, t[599]])
    idx, dist = _check(ctx, q, t)
    assert idx.tolist() == [[10, 11], [258, 500], [10, 11], [10, 11]]
    assert dist.tolist() == [[0, 0], [0, 0], [1, 1], [0, 0]]
    # every row equal: best 0, second 1
    same = np.repeat(t[:1], 300, axis=0)
    idx, dist = _check(ctx, q[:2], same)
    assert (idx == [0, 1]).all()


def test_gpu_match_distance_256(ctx):
    q = np.zeros((1, 32), np.uint8)
    t = np.full((1, 32), 255, np.uint8)
    idx, dist = _check(ctx, q, t)
    assert idx.tolist() == [[0, -1]] and dist.tolist() == [[256, 257]]
    idx, dist = _check(ctx, q, np.concatenate([t, t, q]))
    assert idx.tolist() == [[2, 0]] and dist.tolist() == [[0, 256]]


def test_gpu_match_batch_leaves_padding_untouched(ctx):
    rng = np.random.default_rng(21)
    nq = np.array([5, 0, 300, 257], np.int32)
    nt = np.array([700, 9, 1, 260], np.int32)
    qs, ts = 320, 720
    q = rng.integers(0, 256, (4, qs, 32), dtype=np.uint8)  # the padding holds descriptors too:
    t = rng.integers(0, 256, (4, ts, 32), dtype=np.uint8)  # reading past a count would change a result
    idx = np.full((4, qs, 2), -77, np.int32)
    dist = np.full((4, qs, 2), -88, np.int32)
    gi, gd = ctx.match_hamming(q, t, nq, nt, idx=idx, dist=dist)
    assert gi is idx and gd is dist
    for p in range(4):
        ei, ed = R.knn2(q[p, : nq[p]], t[p, : nt[p]])
        assert np.array_equal(idx[p, : nq[p]], ei), p
        assert np.array_equal(dist[p, : nq[p]], ed), p
        assert (idx[p, nq[p]:] == -77).all() and (dist[p, nq[p]:] == -88).all(), p
    # without the caller's arrays the padding reads as "no neighbour"
    gi, gd = ctx.match_hamming(q, t, nq, nt)
    assert (gi[1] == -1).all() and (gd[1] == 257).all() and np.array_equal(gi[0, :5], idx[0, :5])


def test_gpu_match_argument_errors(ctx):
    import svo_amd as S
    i32p, u8p = C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    q = np.zeros((4, 32), np.uint8)
    idx = np.full((4, 2), -77, np.int32)
    dist = np.full((4, 2), -88, np.int32)

    def call(P, nq, nt, qs, ts):
        nq, nt = np.array([nq], np.int32), np.array([nt], np.int32)
        return S.lib().svo_match_hamming(ctx.handle, P, nq.ctypes.data_as(i32p), nt.ctypes.data_as(i32p), qs, ts,
                                         q.ctypes.data_as(u8p), q.ctypes.data_as(u8p), idx.ctypes.data_as(i32p),
                                         dist.ctypes.data_as(i32p))

    assert call(0, 4, 4, 4, 4) == 0        # no problems: valid, nothing written
    assert call(1, 0, 4, 4, 4) == 0
    assert (idx == -77).all() and (dist == -88).all()
    for args in ((-1, 4, 4, 4, 4), (1, -1, 4, 4, 4), (1, 4, -1, 4, 4), (1, 5, 4, 4, 4), (1, 4, 5, 4, 4),
                 (1, 4, 4, -4, 4)):
        assert call(*args) == -1, args
    assert (idx == -77).all() and (dist == -88).all()
    assert call(1, 4, 4, 4, 4) == 0 and idx.tolist() == [[0, 1]] * 4 and (dist == 0).all()
