"""svo_match_projected's cases (TEST INFRASTRUCTURE): a seeded generator of small
synthetic problems, and the restatement (tests/match_projected_reference.py) run
on the relocalisation scene of tests/orb_describe_cases.py and on the place
memory's dropped-frame sequences (tests/places_cases.py). Computed once, shared
read-only by test_match_projected_cpu.py (which recomputes the recorded figures)
and the GPU tests."""
from __future__ import annotations

import functools

import numpy as np

import match_projected_reference as MP

W, H = 64, 48                     # the synthetic frame
K4 = (50.0, 50.0, 32.0, 24.0)
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
RELATED = 0.8                     # share of the points made from a keypoint
JITTER = 3.0                      # pixels
MAX_FLIPS = 40                    # descriptor bits flipped
# The generator's conditions (test_match_projected_cpu.py asserts them on the
# restatement): with 255 or more points and keypoints and radius 4, at least half of
# the visible points have two or more candidates, some have none, and at least one
# keypoint is bid for by two points. An empty 9 x 9 window is rare at this density
# (it happens at the frame's corners), so the seed of each such size is the first
# one under which the problem has it; every other size uses seed 0.
SEEDS = {(255, 255): 1, (255, 256): 3, (255, 257): 11, (256, 255): 3, (256, 256): 0, (256, 257): 3, (257, 255): 0,
         (257, 256): 3, (257, 257): 3}


def seed_of(n_pts, n_kp):
    return SEEDS.get((n_pts, n_kp), 0)


def rodrigues(rv):
    """A small rotation for the generator (any orthonormal R serves: the rules take T as given)."""
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th < 1e-12:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


@functools.lru_cache(maxsize=None)
def synth(n_pts, n_kp, seed=0, w=W, h=H):
    """One problem: dict of xyz (n_pts, 3) f64, pdesc, kxy (n_kp, 2) f32, kdesc, T (12,).
    Keypoints uniform over the frame. A RELATED share of the points is a keypoint's
    pixel, jittered by up to JITTER px, back-projected at a random depth through a
    random small pose, with the keypoint's descriptor and 0 .. MAX_FLIPS bits flipped;
    the rest are unrelated points around the frustum with random descriptors."""
    rng = np.random.default_rng([seed, n_pts, n_kp, w, h])
    fx, fy, cx, cy = K4
    cx, cy = cx * w / W, cy * h / H
    kxy = (rng.uniform(0, 1, (n_kp, 2)) * [w, h]).astype(np.float32)
    kdesc = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    Rm = rodrigues(rng.uniform(-0.05, 0.05, 3))
    t = rng.uniform(-0.1, 0.1, 3)
    xyz = np.zeros((n_pts, 3))
    pdesc = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    for i in range(n_pts):
        z = rng.uniform(2, 8)
        if n_kp and rng.uniform() < RELATED:
            j = int(rng.integers(n_kp))
            px = kxy[j].astype(np.float64) + rng.uniform(-JITTER, JITTER, 2)
            bits = np.unpackbits(kdesc[j])
            flip = rng.choice(256, int(rng.integers(0, MAX_FLIPS + 1)), replace=False)
            bits[flip] ^= 1
            pdesc[i] = np.packbits(bits)
        else:  # anywhere in a frame 8 px wider than the image, a fifth of them behind the camera
            px = rng.uniform(-8, 8 + np.array([w, h]), 2)
            if rng.uniform() < 0.2:
                z = -z
        xc = np.array([(px[0] - cx) / fx * z, (px[1] - cy) / fy * z, z])
        xyz[i] = Rm.T @ (xc - t)
    out = dict(xyz=xyz, pdesc=pdesc, kxy=kxy, kdesc=kdesc, T=np.r_[Rm.ravel(), t], K4=np.array([fx, fy, cx, cy]),
               size=(w, h))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synth_want(n_pts, n_kp, seed=0, w=W, h=H, radius=4.0, max_dist=64, ratio_pct=80):
    """The restatement on synth(...): dict of idx, dist, proj, ncand, pairs."""
    s = synth(n_pts, n_kp, seed, w, h)
    idx, dist, proj, ncand = MP.match_projected(s["xyz"], s["pdesc"], s["kxy"], s["kdesc"], s["T"], s["K4"], s["size"],
                                                radius)
    return dict(idx=idx, dist=dist, proj=proj, ncand=ncand, pairs=MP.pairs(idx, dist, max_dist, ratio_pct))


# ------------------------------------------------------------------ the recorded scenes
# What the restatement reaches with radius 4, max_dist 64, ratio 80 and the oracle's
# solvePnPRansac, the first pose as the existing restatements give it (recomputed
# and compared by test_match_projected_cpu.py). first / widened: (pairs, inliers);
# visible / with_candidate: map points; kept: widened pairs the first pass had too;
# rot_deg / trans_m: the widened pose against the scene (the camera only rotates).
MEASURED = {
    "n300": dict(first=(172, 172), widened=(177, 177), visible=224, with_candidate=214, kept=170, rot_deg=0.046,
                 trans_m=0.019),
    # thin: the widened set is smaller than the first pass's, and gives the same pose
    "n64": dict(first=(15, 14), widened=(14, 14), visible=25, with_candidate=18, kept=14, rot_deg=0.362, trans_m=0.080),
    "RELOC": dict(first=(234, 233), widened=(262, 262), visible=456, with_candidate=409, kept=214, rot_deg=0.158,
                  trans_m=0.051),
}


@functools.lru_cache(maxsize=None)
def scene_inputs(name):
    """dict of map_xyz, map_desc, kxy, kdesc, K (3x3), size, first = dict(pairs (frame,
    map), rvec, tvec, inliers) and pose_error(rvec, tvec) -> (deg, m)."""
    import oracle as O
    import orb_describe_cases as ODC
    if name == "RELOC":
        d = ODC.reloc_inputs()
        sc, t = d["scene"], ODC.RELOC["t"]
        kxy = np.ascontiguousarray(d["cur"]["kp"][:, :2], np.float32)
        p = ODC.reloc_pairs()
        rc, rv, tv, inl, _ = O.solve_pnp_ransac(d["xyz"][p[:, 1]], kxy[p[:, 0]], sc.K)
        assert rc == 1
        return dict(map_xyz=d["xyz"], map_desc=d["map"]["desc"], kxy=kxy, kdesc=d["cur"]["desc"], K=sc.K,
                    size=(320, 240), first=dict(pairs=p, rvec=rv, tvec=tv, inliers=inl),
                    pose_error=lambda r, tt: ODC.pose_error(sc, t, r, tt))
    import places_cases as P
    import starved_cases as C
    q = P.query(name, P.REBUILD_T, *P.BOUND)
    assert q["ok"] and q["frame_t"] == P.PICKED[name]["frame"]
    rec, cur = P.records(name)[q["frame_t"]], P.records(name)[P.REBUILD_T]
    sc = C.scene(P.CASES[name])
    return dict(map_xyz=rec["xyz"], map_desc=rec["desc"], kxy=cur["xy"], kdesc=cur["desc"], K=P.SCENE_K,
                size=(C.W, C.H), first=dict(pairs=q["pairs"], rvec=q["rvec"], tvec=q["tvec"], inliers=q["inliers"]),
                pose_error=lambda r, tt: ODC.pose_error(sc, P.REBUILD_T, r, tt))


@functools.lru_cache(maxsize=None)
def scene_want(name):
    """The restatement's widening of the scene's first pose (MP.widen's dict)."""
    d = scene_inputs(name)
    return MP.widen(d["map_xyz"], d["map_desc"], d["kxy"], d["kdesc"], d["first"]["rvec"], d["first"]["tvec"], d["K"],
                    d["size"], **MP.DEFAULTS)


def measured_row(name):
    """MEASURED's figures of one scene, recomputed."""
    d, wn = scene_inputs(name), scene_want(name)
    rot, trans = d["pose_error"](wn["rvec"], wn["tvec"]) if wn["ok"] else (np.nan, np.nan)
    first = {tuple(r) for r in d["first"]["pairs"].tolist()}
    kept = sum(tuple(r) in first for r in wn["pairs"].tolist())
    return dict(first=(len(d["first"]["pairs"]), len(d["first"]["inliers"])),
                widened=(len(wn["pairs"]), len(wn["inliers"])), visible=wn["visible"],
                with_candidate=wn["with_candidate"], kept=kept, rot_deg=round(rot, 3), trans_m=round(trans, 3))
