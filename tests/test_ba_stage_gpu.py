"""The bundle adjustment's staging on the device (svo_ba_stage_lists, ba_stage.hip)
against the host's stable sort (svo_ba_sort_observations, host code) on the same
observations listed camera by camera with the points numbered by ascending id:
exact equality of every array. The device path gets W sorted lists per problem
and places every observation by binary searches; the shapes are the ones where
that can go wrong -- one camera, two, sixteen; lists of 0, 1 and around the wave
(64) and workgroup (256) sizes up to the capacity; an empty list between full
ones; identical lists; disjoint lists; ids with gaps; an id in the first and the
last camera only; more observations than one scan chunk (1024) beside a tiny
problem."""
import ctypes as C

import numpy as np
import pytest

import svo_amd as S

pytestmark = pytest.mark.gpu

KEYS = ("ocam", "oxy", "pt_off", "cam_off", "cam_idx", "cam_pt", "pt_id", "n_points", "n_obs")


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def pack(problems, W, cap):
    """problems: per problem a list of W (ids, xy) lists -> counts, ids, xy arrays."""
    P = len(problems)
    counts = np.zeros((P, W), np.int32)
    ids = np.full((P, W, cap), -7, np.int32)  # (behind a list's end: never read)
    xy = np.full((P, W, cap, 2), np.nan, np.float32)
    for p, lists in enumerate(problems):
        assert len(lists) == W
        for j, (a, b) in enumerate(lists):
            counts[p, j] = len(a)
            ids[p, j, : len(a)] = a
            xy[p, j, : len(a)] = b
    return counts, ids, xy


def host_stage(lists, W, cap):
    """What bundle.cpp's stage() builds for one problem from the observations listed
    camera by camera, points numbered by ascending id, at strides W * cap."""
    O = W * cap
    cam = np.concatenate([np.full(len(a), j, np.int32) for j, (a, _) in enumerate(lists)]).astype(np.int32)
    mid = np.concatenate([np.asarray(a, np.int32) for a, _ in lists]).astype(np.int32)
    xy = np.concatenate([np.asarray(b, np.float32).reshape(-1, 2) for _, b in lists]).astype(np.float32)
    pid = np.unique(mid).astype(np.int32)
    pt = np.searchsorted(pid, mid).astype(np.int32)
    n, M = len(cam), len(pid)
    order, cam_idx = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    pt_off, cam_off = np.zeros(M + 1, np.int32), np.zeros(W + 1, np.int32)
    ip = C.POINTER(C.c_int)
    cam_c, pt_c = np.ascontiguousarray(cam), np.ascontiguousarray(pt)
    rc = S.lib().svo_ba_sort_observations(cam_c.ctypes.data_as(ip), pt_c.ctypes.data_as(ip), n, W, M,
                                          order.ctypes.data_as(ip), pt_off.ctypes.data_as(ip),
                                          cam_off.ctypes.data_as(ip), cam_idx.ctypes.data_as(ip))
    assert rc == 0
    order, cam_idx = order[:n], cam_idx[:n]
    out = {"ocam": np.zeros(O, np.int32), "oxy": np.zeros((O, 2), np.float32), "pt_off": np.full(O + 1, n, np.int32),
           "cam_off": cam_off, "cam_idx": np.zeros(O, np.int32), "cam_pt": np.zeros(O, np.int32),
           "pt_id": np.zeros(O, np.int32), "n_points": np.int32(M), "n_obs": np.int32(n)}
    out["ocam"][:n] = cam[order]
    out["oxy"][:n] = xy[order]
    out["pt_off"][: M + 1] = pt_off
    out["cam_idx"][:n] = cam_idx
    out["cam_pt"][:n] = pt[order[cam_idx]]
    out["pt_id"][:M] = pid
    return out


def check(ctx, problems, W, cap):
    got = ctx.ba_stage_lists(*pack(problems, W, cap))
    for p, lists in enumerate(problems):
        want = host_stage(lists, W, cap)
        for k in KEYS:
            g = got[k][p]
            if k == "oxy":
                assert np.array_equal(g.view(np.uint32), want[k].view(np.uint32)), (p, k)
            else:
                assert np.array_equal(g, want[k]), (p, k, g, want[k])
    return got


def make_list(rng, n, universe):
    """n distinct ids out of range(universe), ascending, with their pixels."""
    a = np.sort(rng.choice(universe, size=n, replace=False)).astype(np.int32)
    return a, rng.uniform(0, 1000, (n, 2)).astype(np.float32)


@pytest.mark.parametrize("W", [1, 2, 16])
def test_list_lengths_around_wave_and_block(ctx, W):
    """Every list length of the issue in one batch of W-camera problems: problem q has
    its first list of length LENGTHS[q], the others of the lengths that follow; ids
    drawn from 1.5 x cap with gaps, so lists overlap in part."""
    cap = 320
    lengths = [0, 1, 63, 64, 65, 255, 256, 257, cap]
    rng = np.random.default_rng(W)
    problems = [[make_list(rng, lengths[(q + j) % len(lengths)], cap * 3 // 2) for j in range(W)]
                for q in range(len(lengths))]
    got = check(ctx, problems, W, cap)
    assert got["n_obs"].max() > 1024 or W < 16  # W = 16: more than one scan chunk


def test_empty_identical_disjoint(ctx):
    rng = np.random.default_rng(3)
    cap, W = 128, 3
    full = make_list(rng, cap, cap)  # ids 0 .. cap - 1, every slot used
    empty = (np.zeros(0, np.int32), np.zeros((0, 2), np.float32))
    other = lambda: (full[0].copy(), rng.uniform(0, 1000, (cap, 2)).astype(np.float32))
    problems = [
        [full, empty, other()],  # an empty list between two full ones
        [full, other(), other()],  # all lists identical
        [(np.arange(j * 1000, j * 1000 + 100, dtype=np.int32), rng.uniform(0, 9, (100, 2)).astype(np.float32))
         for j in range(W)],  # all lists disjoint
        [empty, empty, empty],
    ]
    got = check(ctx, problems, W, cap)
    assert list(got["n_points"]) == [cap, cap, 300, 0] and list(got["n_obs"]) == [2 * cap, 3 * cap, 300, 0]


def test_gaps_and_first_last_only(ctx):
    """Ids with gaps; id 500 is seen by cameras 0 and 15 only, id 7 by camera 15 only."""
    rng = np.random.default_rng(5)
    W, cap = 16, 64
    base = np.array([3, 10, 11, 40, 90, 91, 300, 301, 900, 2000], np.int32)
    lists = []
    for j in range(W):
        a = base[rng.random(len(base)) < 0.7]
        if j in (0, 15):
            a = np.sort(np.r_[a, 500]).astype(np.int32)
        if j == 15:
            a = np.sort(np.r_[a, 7]).astype(np.int32)
        lists.append((a, rng.uniform(0, 99, (len(a), 2)).astype(np.float32)))
    got = check(ctx, [lists], W, cap)
    M = int(got["n_points"][0])
    ids = list(got["pt_id"][0, :M])
    i = ids.index(500)
    seen = got["ocam"][0, got["pt_off"][0, i]: got["pt_off"][0, i + 1]]
    assert list(seen) == [0, 15]
    i = ids.index(7)
    assert list(got["ocam"][0, got["pt_off"][0, i]: got["pt_off"][0, i + 1]]) == [15]


def test_batch_independence(ctx):
    """16 x 300 observations beside a problem of 3: each gives the bits it gives alone."""
    rng = np.random.default_rng(9)
    W, cap = 16, 300
    big = [make_list(rng, cap, 450) for _ in range(W)]
    empty = (np.zeros(0, np.int32), np.zeros((0, 2), np.float32))
    small = [make_list(rng, 2, 5), make_list(rng, 1, 5)] + [empty] * (W - 2)
    both = check(ctx, [big, small], W, cap)
    assert both["n_obs"][0] == 4800 and both["n_obs"][1] == 3
    for p, lists in enumerate((big, small)):
        alone = check(ctx, [lists], W, cap)
        for k in KEYS:
            assert np.array_equal(alone[k][0].view(np.uint32), both[k][p].view(np.uint32)), (p, k)


@pytest.mark.parametrize("bad", ["equal", "descending", "negative", "count"])
def test_unsorted_list_is_refused(ctx, bad):
    """A list that is not strictly increasing (or a count beyond cap): SVO_ERR_ARG with
    nothing written."""
    W, cap = 2, 8
    counts = np.array([[4, 3]], np.int32)
    ids = np.zeros((1, W, cap), np.int32)
    ids[0, 0, :4] = [1, 2, 3, 4]
    ids[0, 1, :3] = {"equal": [5, 5, 6], "descending": [5, 4, 6], "negative": [-1, 0, 1], "count": [1, 2, 3]}[bad]
    if bad == "count":
        counts[0, 1] = cap + 1
    xy = np.zeros((1, W, cap, 2), np.float32)
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    out = np.full(W * cap + 1, -5, np.int32)
    oxy = np.full(2 * W * cap, -5, np.float32)
    n = np.full(1, -5, np.int32)
    args = [out.copy() for _ in range(6)]
    rc = S.lib().svo_ba_stage_lists(ctx.handle, 1, W, cap, counts.ctypes.data_as(ip), ids.ctypes.data_as(ip),
                                    xy.ctypes.data_as(fp), args[0].ctypes.data_as(ip), oxy.ctypes.data_as(fp),
                                    *[a.ctypes.data_as(ip) for a in args[1:]], n.ctypes.data_as(ip),
                                    n.ctypes.data_as(ip))
    assert rc == -1  # SVO_ERR_ARG
    assert all(np.all(a == -5) for a in args) and np.all(oxy == -5) and n[0] == -5
