"""ORB detection off its defaults: the cases tests/test_orb_params_gpu.py runs on
the GPU, their inputs, and the oracle's side of each (computed once and shared;
treat as read-only). tests/test_orb.py uses the level sizes for its resize pins
and checks on the CPU that every case reaches what it is there for.

The input is blocky noise (3x3 blocks of uniform random bytes): FAST corners on
every level and right up to the edge filter on every side, which the scenes of
the other ORB tests (edge 31) never have.
"""
from functools import lru_cache

import numpy as np

import oracle as O

KEEP_ALL = 100000  # no level's quota binds: every FAST corner inside the edge comes back

# id: w, h, seed, then ORB parameters (defaults below) and the mask kind
_DEF = dict(nfeatures=KEEP_ALL, scale=1.2, nlevels=8, edge=4, patch=None, thr=10, harris=True, mask=None, fill=None)
CASES = {
    "base": dict(w=129, h=67, seed=1, patch=4),
    "s2": dict(w=129, h=67, seed=1, scale=2.0, nlevels=3),
    "s3": dict(w=200, h=131, seed=2, thr=5, scale=3.0, nlevels=3),
    "s15": dict(w=200, h=131, seed=2, thr=5, scale=1.5, nlevels=5),
    "s105": dict(w=200, h=131, seed=2, nfeatures=60, edge=8, thr=5, scale=1.05, harris=False),
    "fast60": dict(w=129, h=67, seed=1, nfeatures=60, harris=False),
    "h40": dict(w=129, h=67, seed=1, nfeatures=40),
    "h300": dict(w=200, h=131, seed=2, nfeatures=300, thr=5, scale=1.5, nlevels=5),
    "nf7": dict(w=129, h=67, seed=1, nfeatures=7),
    "nf0": dict(w=129, h=67, seed=1, nfeatures=0),
    "nl1": dict(w=129, h=67, seed=1, nfeatures=40, nlevels=1),
    "e16": dict(w=129, h=67, seed=1, edge=16),
    "e5": dict(w=129, h=67, seed=1, edge=5, patch=5),
    "w64": dict(w=64, h=64, seed=4),
    "w257": dict(w=257, h=33, seed=5),
    "w65x9": dict(w=65, h=9, seed=4, nlevels=2),
    "tiny": dict(w=24, h=20, seed=3),
    "thr0": dict(w=129, h=67, seed=1, thr=0),
    "thr255": dict(w=129, h=67, seed=1, thr=255),
    "thr300": dict(w=129, h=67, seed=1, thr=300),
    "thr-5": dict(w=129, h=67, seed=1, thr=-5),
    "mask": dict(w=129, h=67, seed=1, mask="mixed"),
    "mask0": dict(w=129, h=67, seed=1, mask="zero"),
    "const": dict(w=129, h=67, seed=1, nfeatures=1000, fill=90),
    # The clamped taps of the resize. Shrinking never leaves the source (the last
    # sample position is sw - 1 - (scale - 1) / 2 < sw - 1), so the cases above do not
    # reach them: consecutive levels that round to the same size do (the last tap is
    # then the last source pixel at full weight, its neighbour one past the edge at
    # weight 0), and so does a source level one pixel high.
    "same": dict(w=40, h=24, seed=6, scale=1.02),
    "h1": dict(w=40, h=2, seed=6, scale=1.5, nlevels=3),
}
EDGE_LINE_CASES = ("base", "s2", "s3", "s15", "e5", "e16", "w64", "w257")


def blocky(w, h, seed):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, ((h + 2) // 3, (w + 2) // 3), dtype=np.uint8)
    return np.kron(b, np.ones((3, 3), np.uint8))[:h, :w].copy()


def params(cid):
    p = dict(_DEF, **CASES[cid])
    if p["patch"] is None:
        p["patch"] = p["edge"]
    return p


def inputs(cid):
    """(image, mask or None) of a case."""
    p = params(cid)
    w, h = p["w"], p["h"]
    img = np.full((h, w), p["fill"], np.uint8) if p["fill"] is not None else blocky(w, h, p["seed"])
    m = None
    if p["mask"] == "mixed":
        m = np.full((h, w), 255, np.uint8)
        m[:, :40] = 0
        m[30:40, :] = 0
        m[5, 100] = 254
        m[60, 5] = 1
    elif p["mask"] == "zero":
        m = np.zeros((h, w), np.uint8)
    return img, m


def oracle_kwargs(cid):
    p = params(cid)
    return dict(nfeatures=p["nfeatures"], scale_factor=p["scale"], nlevels=p["nlevels"], edge_threshold=p["edge"],
                patch_size=p["patch"], fast_threshold=p["thr"], harris=p["harris"])


def level_info(cid):
    p = params(cid)
    return O.orb_level_info(p["w"], p["h"], p["scale"], p["nlevels"], p["nfeatures"])


@lru_cache(maxsize=None)
def oracle_detect(cid):
    """(keypoints (n, 3), octaves (n,)) of the oracle. cap 2^16 holds every case."""
    img, m = inputs(cid)
    return O.orb_detect(img, m, **oracle_kwargs(cid))


@lru_cache(maxsize=None)
def oracle_levels(cid):
    """([level images], [level masks] or None): each level resized from the previous
    one, the masks thresholded (254, TOZERO) from level 1 on, as ORB builds them."""
    img, m = inputs(cid)
    lw, lh, _, _ = level_info(cid)
    lv, mk = [img], None if m is None else [m]
    for l in range(1, len(lw)):
        lv.append(O.resize_linear_exact(lv[-1], int(lw[l]), int(lh[l])))
        if mk is not None:
            r = O.resize_linear_exact(mk[-1], int(lw[l]), int(lh[l]))
            mk.append(np.where(r > 254, r, 0).astype(np.uint8))
    return lv, mk


def level_xy(cid):
    """Integer level coordinates (n, 2) of the oracle's keypoints: rint(pt / scale_l)."""
    kp, octv = oracle_detect(cid)
    ls = level_info(cid)[2]
    s = ls[octv].astype(np.float32)
    return np.rint(kp[:, :2].astype(np.float32) / s[:, None]).astype(int)


def check_reaches_target(cid):
    """The conditions on the oracle's output without which a case could pass while
    missing what it is there for."""
    p = params(cid)
    kp, octv = oracle_detect(cid)
    lw, lh, _, nper = level_info(cid)
    nlev, e = p["nlevels"], p["edge"]
    counts = np.bincount(octv, minlength=nlev)
    xy = level_xy(cid)
    if cid in EDGE_LINE_CASES:  # a keypoint on each of the four lines of the edge filter
        w_l, h_l = lw[octv], lh[octv]
        for name, hit in (("x == edge", xy[:, 0] == e), ("x == lw-edge-1", xy[:, 0] == w_l - e - 1),
                          ("y == edge", xy[:, 1] == e), ("y == lh-edge-1", xy[:, 1] == h_l - e - 1)):
            assert hit.sum() >= 1, f"{cid}: no keypoint on {name}"
    if cid in ("s105", "fast60"):  # ties at the quota kept by retainBest's partition
        assert (counts > nper).any(), f"{cid}: no level beyond its quota ({counts} vs {nper})"
    if cid in ("h40", "h300"):  # the 2 n_l prefilter binds, then the Harris selection
        assert counts.tolist() == nper.tolist(), f"{cid}: {counts} vs quotas {nper}"
        img, _ = inputs(cid)
        f = O.fast(img, p["thr"], True)
        inside = (f[:, 0] >= e) & (f[:, 0] < lw[0] - e) & (f[:, 1] >= e) & (f[:, 1] < lh[0] - e)
        assert inside.sum() > 2 * nper[0], f"{cid}: prefilter idle ({inside.sum()} corners, quota {nper[0]})"
    if cid == "nf7":
        assert nper.tolist() == [2, 1, 1, 1, 1, 1, 1, 0] and counts[7] == 0
    if cid == "e16":
        assert (lw[4], lh[4]) == (62, 32)
        assert (counts[4:] == 0).all() and (counts[:4] > 0).all(), f"e16: {counts}"
    if cid == "tiny":
        assert (lw[7], lh[7]) == (7, 6)
        assert (counts[5:] == 0).all() and counts.sum() > 0, f"tiny: {counts}"
    if cid in ("nf0", "thr255", "thr300", "mask0", "const"):
        assert len(kp) == 0
    if cid in ("thr0", "mask", "nl1", "w65x9"):
        assert len(kp) > 0
    if cid == "thr-5":
        k0, o0 = oracle_detect("thr0")
        assert np.array_equal(kp, k0) and np.array_equal(octv, o0)
    if cid == "same":  # an identity resize along x and along y
        assert (np.diff(lw) == 0).any() and (np.diff(lh) == 0).any(), f"same: {lw} {lh}"
        assert len(kp) > 0
    if cid == "h1":  # level 2 is resized from a level one pixel high
        assert lh.tolist() == [2, 1, 1] and len(kp) == 0
    if cid == "w65x9":
        assert (lw[1], lh[1]) == (54, 7)
    if cid == "mask":  # some level's mask must have lost pixels to the 254 threshold, and kept others
        mk = oracle_levels(cid)[1]
        assert all(set(np.unique(m)) == {0, 255} for m in mk[1:])
        assert mk[0][5, 100] == 254 and mk[0][60, 5] == 1


def level_pairs():
    """Every (sw, sh, dw, dh) of consecutive levels over all cases."""
    out = set()
    for cid in CASES:
        lw, lh, _, _ = level_info(cid)
        for l in range(1, len(lw)):
            out.add((int(lw[l - 1]), int(lh[l - 1]), int(lw[l]), int(lh[l])))
    return sorted(out)
