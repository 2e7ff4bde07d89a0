"""The place memory's cases (TEST INFRASTRUCTURE): the restatement
(tests/places_reference.py) run on the dropped-frame sequences of
tests/starved_cases.py, once per case and shared, read-only, by
test_places_cpu.py (which recomputes the recorded figures) and
test_places_gpu.py (whose bars come from them)."""
from __future__ import annotations

import functools

import numpy as np

import orb_describe_cases as K
import places_reference as PR
import starved_cases as C

CASES = {"n300": C.DROPPED_300, "n64": C.DROPPED_64}
REBUILD_T = 4          # the first frame after the loss at t = 3: the set rebuilt under the identity pose
BOUND = (0, 2)         # the records made before the loss
SCENE_K = C.scene(C.DROPPED_300).K

# What the restatement reaches on the oracle loop's lists (patch 31, default
# pattern, ratio 80, cross-check, the oracle's solvePnPRansac), recomputed and
# compared by test_places_cpu.py. rows: (query frame, record frame) -> valid
# query / record entries, filtered pairs, inliers, rotation error in degrees
# against Scene.R(query frame), |tvec| in metres (the camera only rotates).
# A record made before the loss gives the pose in the old world; one made after it
# gives more pairs and the pose of the new world (the rotation since the rebuild).
MEASURED = {
    "n300": {
        (4, 0): dict(nq=235, nt=220, pairs=167, inliers=167, rot_deg=0.090, trans_m=0.018),
        (4, 1): dict(nq=235, nt=224, pairs=172, inliers=172, rot_deg=0.053, trans_m=0.016),
        (4, 2): dict(nq=235, nt=227, pairs=172, inliers=172, rot_deg=0.035, trans_m=0.013),
        (5, 4): dict(nq=238, nt=235, pairs=230, inliers=230, rot_deg=2.226, trans_m=0.002),
        (8, 7): dict(nq=245, nt=248, pairs=242, inliers=242, rot_deg=3.900, trans_m=0.002),
    },
    # thin: 12-15 pairs; records of 5 (frame 3, a garbage model's survivors) and 0 (frame 6) entries
    "n64": {
        (4, 0): dict(nq=38, nt=26, pairs=14, inliers=14, rot_deg=0.362, trans_m=0.080),
        (4, 1): dict(nq=38, nt=25, pairs=15, inliers=14, rot_deg=0.362, trans_m=0.080),
        (4, 2): dict(nq=38, nt=24, pairs=15, inliers=14, rot_deg=0.362, trans_m=0.080),
        (5, 4): dict(nq=38, nt=38, pairs=38, inliers=38, rot_deg=2.190, trans_m=0.008),
        (8, 7): dict(nq=34, nt=35, pairs=34, inliers=34, rot_deg=3.886, trans_m=0.002),
    },
}
# entries of every frame's record (the blank frames 3 and 6 leave none at N = 300)
RECORD_SIZES = {"n300": [220, 224, 227, 0, 235, 238, 0, 248, 245], "n64": [26, 25, 24, 5, 38, 38, 0, 35, 34]}
# the query of frame 4 bounded to [0, 2]: the record it picks and its pose errors
PICKED = {
    "n300": dict(frame=1, pairs=172, rot_deg=0.053, trans_m=0.016),
    "n64": dict(frame=1, pairs=15, rot_deg=0.362, trans_m=0.080),
}


@functools.lru_cache(maxsize=None)
def records(name, patch_size=31):
    """{frame: record} of the case's oracle loop: every frame's list as the step leaves it."""
    case = CASES[name]
    tr, fr = C.oracle_trace(case), C.frames(case)
    return {t: PR.record(fr[t][0], tr[t].pts, tr[t].X, patch_size) for t in range(case.frames)}


@functools.lru_cache(maxsize=None)
def query(name, t, t_lo=0, t_hi=1 << 30, patch_size=31, min_pairs=4):
    """The restatement's query of frame t against the records of frames < t in the bound."""
    recs = {f: r for f, r in records(name, patch_size).items() if f < t}
    q = records(name, patch_size)[t]
    return PR.query(dict(desc=q["desc"], xy=q["xy"]), recs, t_lo, t_hi, SCENE_K, min_pairs=min_pairs)


def row(name, tq, tr):
    """MEASURED's figures of query frame tq against record frame tr alone."""
    res = query(name, tq, tr, tr)
    rot, trans = K.pose_error(C.scene(CASES[name]), tq, res["rvec"], res["tvec"]) if res["ok"] else (np.nan, np.nan)
    return dict(nq=len(records(name)[tq]["desc"]), nt=len(records(name)[tr]["desc"]), pairs=res["n_pairs"],
                inliers=len(res["inliers"]), rot_deg=rot, trans_m=trans)
