"""bucket_kernel (svo_amd/csrc/bucket.hip) at the table sizes and inputs the
FAST-corner tests never reach: tables of 56-135 KiB (dynamic LDS up to the
96 KiB switch, then bucket_kernel<false> with its tables in global scratch behind
the n bucket ids), dense points so that buckets overflow (slot 0 replaced by the
last point), points on cell edges, in the aliased last column, out of range and
duplicated, and an output capacity that truncates. Bar: np.array_equal on points
and ages against the oracle's restatement of FeatureSet::bucketingFeatures.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import svo_amd as S

pytestmark = pytest.mark.gpu

LDS_MAX = 96 * 1024   # kBucketLdsMax

# (w, h, B, k, n, table bytes, tables in LDS)
CONFIGS = [
    (640, 376, 11, 4, 20000, 57824, True),     # just under 64 KiB
    (640, 376, 10, 4, 20000, 69164, True),     # inside the 64-96 KiB window
    (160, 120, 4, 16, 30000, 96600, True),     # the last size below the switch
    (160, 120, 4, 17, 30000, 101684, False),   # the first size above it
    (640, 376, 8, 4, 20000, 108868, False),
    (160, 120, 2, 4, 30000, 138352, False),    # small image
]
IDS = [f"{w}x{h}-B{B}-k{k}" for w, h, B, k, *_ in CONFIGS]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def table_bytes(w, h, B, k):
    """launch_bucket's expression: cnt[nb] | last[nb] | first[k][nb] | off[nb + 1]."""
    nb = (h // B + 1) * (w // B + 1)
    return 4 * ((k + 3) * nb + 1)


def dense_points(w, h, n, seed):
    """n random points over the image; every 7th floored to integers (on a cell edge
    for every B), every 50th an exact duplicate of its neighbour, every 97th at
    x = w - 0.25 (the last column, which aliases the next row's first bucket), and
    five extras: two the oracle drops as out of range ((5, -40), (3, h + 50)), three
    that fall into in-range cells or aliases."""
    rng = np.random.default_rng(seed)
    p = np.c_[rng.uniform(0, w, n), rng.uniform(0, h, n)].astype(np.float32)
    p[::7] = np.floor(p[::7])
    p[50::50] = p[49::50][:len(p[50::50])]
    p[::97, 0] = np.float32(w - 0.25)
    extra = np.array([(-0.5, 3), (w + 24, 5), (5, -40), (3, h + 50), (w - 0.001, h - 0.001)], np.float32)
    at = (n // 5) * np.arange(5) + 3
    p = np.insert(p, at, extra, axis=0)
    return np.ascontiguousarray(p, np.float32)


_CACHE = {}


def case(w, h, B, k, n):
    """Points, ages and the oracle's selections (with and without ages), computed once."""
    key = (w, h, B, k, n)
    if key not in _CACHE:
        pts = dense_points(w, h, n, seed=w + 31 * B + k)
        ages = (np.arange(len(pts)) % 5).astype(np.int32)
        c = dict(pts=pts, ages=ages, ref=O.bucket(pts, w, h, B, k, ages), ref0=O.bucket(pts, w, h, B, k, None))
        for v in (pts, ages, *c["ref"], *c["ref0"]):
            v.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]


@pytest.mark.parametrize("w,h,B,k,n,nbytes,in_lds", CONFIGS, ids=IDS)
def test_bucket_dense_identical(ctx, w, h, B, k, n, nbytes, in_lds):
    assert table_bytes(w, h, B, k) == nbytes and (nbytes <= LDS_MAX) == in_lds
    c = case(w, h, B, k, n)
    pts = c["pts"]
    # the inputs do what they are for: buckets overflow, others are part full,
    # points sit on cell edges, two of the extras are out of range
    nw, nb = w // B, (h // B + 1) * (w // B + 1)
    idx = (pts[:, 1] / np.float32(B)).astype(np.int32) * nw + (pts[:, 0] / np.float32(B)).astype(np.int32)
    inside = (idx >= 0) & (idx < nb)
    m = np.bincount(idx[inside], minlength=nb)
    assert (~inside).sum() == 2
    assert (m > k).mean() > 0.5 and ((m > 0) & (m <= k)).mean() > 0.02
    assert ((pts[:, 0] % B == 0) & (pts[:, 1] % B == 0)).sum() > 5
    for ages, (rx, ra) in ((c["ages"], c["ref"]), (None, c["ref0"])):
        gx, ga = ctx.bucket_features(pts, w, h, B, k, ages)
        assert len(gx) == len(rx) > 0
        assert np.array_equal(gx.view(np.uint32), rx.view(np.uint32))
        assert np.array_equal(ga, ra)
    assert c["ref"][1].any() and not c["ref0"][1].any()


@pytest.mark.parametrize("cfg", [4, 0], ids=[IDS[4], IDS[0]])
def test_bucket_cap_truncates(ctx, cfg):
    """svo_bucket_features called directly with a capacity below the selection (the
    Python wrapper's cannot truncate): n_out is the full count, the first
    min(cap, total) entries are the oracle's, and nothing is written behind cap."""
    w, h, B, k, n, _, _ = CONFIGS[cfg]
    c = case(w, h, B, k, n)
    pts, ages = c["pts"], c["ages"]
    rx, ra = c["ref"]
    total = len(rx)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    CANARY = 64
    for cap in (0, 1, 37, total - 1):
        xy_out = np.full(2 * cap + CANARY, -7.0, np.float32)
        ages_out = np.full(cap + CANARY, -7, np.int32)
        nout = C.c_int(-1)
        rc = S.lib().svo_bucket_features(ctx.handle, pts.ctypes.data_as(fp), ages.ctypes.data_as(ip), len(pts), w, h,
                                         B, k, xy_out.ctypes.data_as(fp), ages_out.ctypes.data_as(ip), cap,
                                         C.byref(nout))
        assert rc == 0
        assert nout.value == total, cap
        keep = min(cap, total)
        assert np.array_equal(xy_out[:2 * keep].reshape(-1, 2).view(np.uint32), rx[:keep].view(np.uint32)), cap
        assert np.array_equal(ages_out[:keep], ra[:keep]), cap
        assert (xy_out[2 * cap:] == -7.0).all() and (ages_out[cap:] == -7).all(), cap
    # the oracle truncates alike
    ox, oa = np.empty((37, 2), np.float32), np.empty(37, np.int32)
    tot = C.c_int()
    kept = O.load().svo_oracle_bucket(pts.ctypes.data_as(fp), ages.ctypes.data_as(ip), len(pts), w, h, B, k,
                                      ox.ctypes.data_as(fp), oa.ctypes.data_as(ip), 37, C.byref(tot))
    assert kept == 37 and tot.value == total and np.array_equal(ox, rx[:37])
