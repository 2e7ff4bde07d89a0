"""Inputs and the restatement's side of the ORB descriptor GPU tests
(tests/test_orb_describe_gpu.py): computed once and shared; treat as read-only.

Images: a 320x240 piece of the synthetic canvas (random rectangles, box blur) and
its 160x120 top-left crop. Parameter sets: the defaults with wta_k 2, three levels,
and patch_size 15 with edge_threshold 15.
"""
from functools import lru_cache

import numpy as np

import oracle as O
import orb_describe_reference as R

CANVAS_SEED = 1
IMAGES = ("big", "crop")
PARAMS = {
    "def": dict(nlevels=8, patch_size=31, edge_threshold=31),
    "nl3": dict(nlevels=3, patch_size=31, edge_threshold=31),
    "p15": dict(nlevels=8, patch_size=15, edge_threshold=15),
}
# Octaves that must carry keypoints. The crop's levels 4.. are at most 58 rows high:
# not above 2 * 31, so the default edge filter leaves them none (runByImageBorder).
OCTAVES = {("big", "def"): 8, ("big", "nl3"): 3, ("big", "p15"): 8,
           ("crop", "def"): 4, ("crop", "nl3"): 3, ("crop", "p15"): 8}
CASES = sorted(OCTAVES)


@lru_cache(maxsize=None)
def image(name):
    from svo_amd.scene import synth_canvas
    big = synth_canvas(CANVAS_SEED, 320, 240, 320 * 240 // 250)
    img = big if name == "big" else big[:120, :160].copy()
    img.setflags(write=False)
    return img


def orb_params(pid):
    import svo_amd as S
    p = PARAMS[pid]
    return S.OrbParams(nlevels=p["nlevels"], patch_size=p["patch_size"], edge_threshold=p["edge_threshold"], wta_k=2)


@lru_cache(maxsize=None)
def oracle_detect(name, pid):
    p = PARAMS[pid]
    return O.orb_detect(image(name), None, nlevels=p["nlevels"], patch_size=p["patch_size"],
                        edge_threshold=p["edge_threshold"])


@lru_cache(maxsize=None)
def pyramid(name, nlevels):
    """(levels, blurred levels, lscale) of the restatement."""
    lv, ls = R.levels_of(image(name), 1.2, nlevels)
    return lv, [R.blur(a) for a in lv], ls


def corner_pattern(patch_size):
    """A caller's pattern: the default one with the four corners (+-hp, +-hp) in its
    first tests, each compared with the opposite corner and with the centre."""
    hp = patch_size // 2
    pat = R.default_pattern(patch_size).copy()
    pat[:8] = [[hp, hp], [-hp, -hp], [-hp, hp], [hp, -hp], [hp, hp], [0, 0], [-hp, -hp], [0, 0]]
    return pat


@lru_cache(maxsize=None)
def reference(name, pid, corners=False):
    """(desc, angle, valid) of the restatement on the oracle's keypoints."""
    p = PARAMS[pid]
    kp, octv = oracle_detect(name, pid)
    lv, bl, ls = pyramid(name, p["nlevels"])
    pat = corner_pattern(p["patch_size"]) if corners else None
    return R.compute(lv, bl, ls, kp[:, :2], octv, p["patch_size"], pat)


# ------------------------------------------------------------------ relocalisation
RELOC = dict(seed=7, roll_deg=1.5, t=10, nfeatures=500)  # 15 degrees in the image plane
# What the restatement's chain reaches on this scene (measured on the CPU with the
# oracle's solvePnPRansac): 234 pairs, 0.915 of them within
# 2 px of the projected map point, rotation error 0.232 degrees, |t| 0.0677 m.
RELOC_MEASURED = dict(pairs=234, share=0.915, rot_deg=0.232, trans_m=0.0677)


@lru_cache(maxsize=None)
def reloc_inputs():
    """The scene, both frames' oracle keypoints and the restatement's descriptors."""
    from svo_amd.scene import Scene
    sc = Scene(320, 240, seed=RELOC["seed"], roll_deg=RELOC["roll_deg"])
    out = dict(scene=sc)
    for key, t in (("map", 0), ("cur", RELOC["t"])):
        img = sc.frame(t)
        kp, octv = O.orb_detect(img, None, nfeatures=RELOC["nfeatures"])
        desc, _, valid = R.describe_image(img, kp[:, :2], octv)
        assert valid.all()
        out[key] = dict(img=img, kp=kp, octave=octv, desc=desc)
    out["xyz"] = sc.map_points(out["map"]["kp"][:, :2], 0)
    return out


@lru_cache(maxsize=None)
def reloc_pairs():
    """The restatement's filtered pairs (frame index, map index)."""
    d = reloc_inputs()
    iqt, dqt = R.knn2(d["cur"]["desc"], d["map"]["desc"])
    itq, _ = R.knn2(d["map"]["desc"], d["cur"]["desc"])
    return R.match_filter(iqt, dqt, itq, 80)


def pose_error(sc, t, rvec, tvec):
    """(rotation error in degrees against Scene.R(t), |tvec| in metres: the camera only rotates)."""
    dR = O.rodrigues(np.asarray(rvec, np.float64)) @ sc.R(t).T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    return float(ang), float(np.linalg.norm(tvec))


def match_share(sc, t, xyz, kp_xy, pairs):
    """Share of the pairs whose map point projects within 2 px of the frame's keypoint."""
    proj = sc.project(xyz[pairs[:, 1]], t)
    return float((np.linalg.norm(proj - kp_xy[pairs[:, 0]], axis=1) < 2.0).mean())
