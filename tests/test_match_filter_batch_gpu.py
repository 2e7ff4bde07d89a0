"""svo_match_filter_batch (the match filter on the device, many problems at once)
against the restatement's match_filter per problem: the ratio test, the
cross-check, and the stable compaction across wave and chunk boundaries (counts
0, 1, 63, 64, 65, 255, 256, 257: one block takes 256 queries per round, a wave 64)."""
import numpy as np
import pytest

import orb_describe_reference as R
import svo_amd as S

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _problem(rng, nq, nt, mode="random"):
    """(idx_qt (nq, 2), dist_qt (nq, 2), idx_tq (nt, 2)) as svo_match_hamming would
    lay one problem out. random: about half the queries pass each test."""
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), 257, np.int32)
    tq = np.full((nt, 2), -1, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist, tq
    if mode == "all":  # query q matches train q % nt ... one to one needs nt >= nq
        assert nt >= nq
        idx[:, 0] = np.arange(nq)
        idx[:, 1] = (np.arange(nq) + 1) % nt if nt > 1 else -1
        dist[:, 0] = 10
        dist[:, 1] = 100 if nt > 1 else 257
        tq[:nq, 0] = np.arange(nq)
        return idx, dist, tq
    idx[:, 0] = rng.integers(0, nt, nq)
    if nt > 1:
        idx[:, 1] = (idx[:, 0] + 1 + rng.integers(0, nt - 1, nq)) % nt
        dist[:, 1] = rng.integers(40, 120, nq)
    dist[:, 0] = rng.integers(20, 100, nq) if mode == "random" else dist[:, 1]  # none: d1 == d2 fails every ratio
    tq[:, 0] = rng.integers(0, nq, nt)
    half = rng.random(nq) < 0.6  # make the cross-check hold for many
    tq[idx[half, 0], 0] = np.flatnonzero(half)
    return idx, dist, tq


def _pack(probs, qs, ts, fill=-7):
    """The problems in one batch at strides qs / ts, the padding rows filled with `fill`."""
    P = len(probs)
    idx = np.full((P, qs, 2), fill, np.int32)
    dist = np.full((P, qs, 2), fill, np.int32)
    tq = np.full((P, max(ts, 1), 2), fill, np.int32)[:, :ts]
    tq = np.ascontiguousarray(tq)
    nq, nt = np.zeros(P, np.int32), np.zeros(P, np.int32)
    for p, (i, d, t) in enumerate(probs):
        nq[p], nt[p] = len(i), len(t)
        idx[p, : len(i)], dist[p, : len(i)], tq[p, : len(t)] = i, d, t
    return idx, dist, tq, nq, nt


def _check(ctx, probs, qs, ts, ratio_pct=80, cross=True):
    idx, dist, tq, nq, nt = _pack(probs, qs, ts)
    pairs = np.full((len(probs), qs, 2), -9, np.int32)
    got, n = ctx.match_filter_batch(idx, dist, nq, nt, tq if cross else None, ratio_pct, pairs=pairs)
    assert got is pairs
    for p, (i, d, t) in enumerate(probs):
        want = R.match_filter(i, d, t if cross else None, ratio_pct)
        assert n[p] == len(want), (p, n[p], len(want))
        assert np.array_equal(pairs[p, : n[p]], want), p
        assert np.all(pairs[p, n[p]:] == -9), f"problem {p}: rows behind its pairs were written"
    return n


@pytest.mark.parametrize("nq", COUNTS)
def test_one_problem_per_count(ctx, nq):
    rng = np.random.default_rng(nq)
    for nt in (max(nq, 1), 257, 3):
        n = _check(ctx, [_problem(rng, nq, nt)], nq, nt)
        assert nq < 63 or 0 < n[0] < nq  # some kept, some dropped
        _check(ctx, [_problem(rng, nq, nt)], nq, nt, cross=False)
        _check(ctx, [_problem(rng, nq, nt)], nq, nt, ratio_pct=0)


@pytest.mark.parametrize("nq", COUNTS)
def test_all_kept_and_none_kept(ctx, nq):
    rng = np.random.default_rng(100 + nq)
    n = _check(ctx, [_problem(rng, nq, nq + 2, "all")], nq, nq + 2)
    assert n[0] == nq
    n = _check(ctx, [_problem(rng, nq, 300, "none")], nq, 300)
    assert n[0] == 0


def test_ratio_zero_keeps_a_single_neighbour(ctx):
    """nt = 1: idx2 = -1, dist2 = 257. The ratio test drops every query; ratio_pct 0
    switches it off and the cross-check alone decides."""
    nq = 65
    idx = np.zeros((nq, 2), np.int32)
    idx[:, 1] = -1
    dist = np.full((nq, 2), 257, np.int32)
    dist[:, 0] = 5
    tq = np.array([[64, -1]], np.int32)
    assert _check(ctx, [(idx, dist, tq)], nq, 1, ratio_pct=80)[0] == 0
    assert _check(ctx, [(idx, dist, tq)], nq, 1, ratio_pct=0)[0] == 1
    assert _check(ctx, [(idx, dist, tq)], nq, 1, ratio_pct=0, cross=False)[0] == nq
    # no neighbour at all (an empty train set): nothing kept, cross-check or not
    none = (np.full((nq, 2), -1, np.int32), np.full((nq, 2), 257, np.int32), np.zeros((0, 2), np.int32))
    assert _check(ctx, [none], nq, 0, ratio_pct=0)[0] == 0
    assert _check(ctx, [none], nq, 4, ratio_pct=0, cross=False)[0] == 0


def test_many_problems_of_different_sizes_at_wide_strides(ctx):
    """Every count at once, strides above every count: the padding rows of the inputs
    hold garbage that is never read as a match, the padding of the output stays."""
    rng = np.random.default_rng(7)
    probs = [_problem(rng, nq, nt) for nq in COUNTS for nt in (0, 1, 200, 257)]
    n = _check(ctx, probs, 300, 260)
    assert n.max() > 64 and n.min() == 0
    _check(ctx, probs, 300, 260, cross=False)
    _check(ctx, probs[::-1], 257, 257, ratio_pct=60)


def test_filter_of_the_matchers_own_output(ctx):
    """Descriptors through match_hamming both ways, then the batch filter: the chain the
    place memory's query runs, against the restatement's chain."""
    rng = np.random.default_rng(11)
    P, qs, ts = 3, 130, 140
    nq, nt = np.array([130, 65, 0], np.int32), np.array([140, 64, 9], np.int32)
    base = rng.integers(0, 256, (P, ts, 32), dtype=np.uint8)
    t = base.copy()
    q = np.zeros((P, qs, 32), np.uint8)
    for p in range(P):
        for i in range(nq[p]):  # a noisy copy of a train descriptor (a few bits flipped), or noise
            src = base[p, i % max(nt[p], 1)].copy()
            src[rng.integers(0, 32, 3)] ^= np.uint8(1 << int(rng.integers(0, 8)))
            q[p, i] = src if i % 3 else rng.integers(0, 256, 32, dtype=np.uint8)
    iqt, dqt = ctx.match_hamming(q, t, nq, nt)
    itq, _ = ctx.match_hamming(t, q, nt, nq)
    pairs, n = ctx.match_filter_batch(iqt, dqt, nq, nt, itq, 80)
    for p in range(P):
        a, b = R.knn2(q[p, : nq[p]], t[p, : nt[p]])
        c, _ = R.knn2(t[p, : nt[p]], q[p, : nq[p]])
        want = R.match_filter(a, b, c, 80)
        assert n[p] == len(want) and np.array_equal(pairs[p, : n[p]], want)
    assert n[0] > 40 and n[2] == 0


def test_errors(ctx):
    idx, dist, tq = _problem(np.random.default_rng(1), 10, 12)
    i3, d3, t3, nq, nt = _pack([(idx, dist, tq)], 10, 12)
    with pytest.raises(S.SvoError):
        ctx.match_filter_batch(i3, d3, nq, nt, t3, -1)
    with pytest.raises(S.SvoError):
        ctx.match_filter_batch(i3, d3, np.array([11], np.int32), nt, t3)  # a count above its stride
    bad = i3.copy()
    bad[0, 4, 0] = 12  # an index not below the train count
    pairs = np.full((1, 10, 2), -9, np.int32)
    with pytest.raises(S.SvoError):
        ctx.match_filter_batch(bad, d3, nq, nt, t3, pairs=pairs)
    assert np.all(pairs == -9)
    p, n = ctx.match_filter_batch(np.zeros((0, 4, 2), np.int32), np.zeros((0, 4, 2), np.int32), [], [])
    assert p.shape == (0, 4, 2) and len(n) == 0
