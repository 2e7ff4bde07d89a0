#!/usr/bin/env python3
"""Time one Levenberg-Marquardt iteration of the windowed bundle adjustment
(svo_ba_time_iteration: linearise, eliminate, solve, update, trial cost; HIP
events after one warm-up) on the batched front end's use case: 256 problems x 8
cameras x 2000 points with about 70 % of the possible observations present.
--stage: the device staging chain for the same use case given as the front end's
window holds it (svo_ba_time_staging), against the host's staging of those lists.
Prints one JSON line. Not a test and not the project's benchmark (bench.py)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import svo_amd as S  # noqa: E402

K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])


def problems(P, C, M, present, seed):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-8, 8, (P, M)), rng.uniform(-3, 3, (P, M)), rng.uniform(6, 40, (P, M))], 2)
    poses = np.zeros((P, C, 12))
    poses[:, :, [0, 4, 8]] = 1
    poses[:, :, 11] = -0.5 * np.arange(C)  # cameras stepping 0.5 m along z
    Pc = X[:, None] + poses[:, :, None, 9:]
    xy = np.stack([K[0, 0] * Pc[..., 0] / Pc[..., 2] + K[0, 2], K[1, 1] * Pc[..., 1] / Pc[..., 2] + K[1, 2]], 3)
    xy += rng.normal(0, 0.5, xy.shape)
    keep = rng.random((P, C, M)) < present
    n_obs = keep.reshape(P, -1).sum(1).astype(np.int32)
    O = int(n_obs.max())
    oc, op = np.zeros((P, O), np.int32), np.zeros((P, O), np.int32)
    oxy = np.zeros((P, O, 2), np.float32)
    for p in range(P):
        c, i = np.nonzero(keep[p])
        perm = rng.permutation(len(c))
        oc[p, :len(c)], op[p, :len(c)], oxy[p, :len(c)] = c[perm], i[perm], xy[p, c[perm], i[perm]]
    # off the truth, so that the step is not zero
    poses[:, 2:, 9:] += rng.normal(0, 0.05, (P, C - 2, 3))
    X *= 1 + rng.uniform(-0.03, 0.03, (P, M, 1))
    fixed = np.zeros((P, C), np.uint8)
    fixed[:, :2] = 1
    return poses, fixed, X, oc, op, oxy, n_obs


def window_lists(P, C, M, present, seed):
    """The same use case as the front end's window holds it: per problem and camera a
    list of the point ids it sees, ascending, with their pixels (cap: M rounded up
    to 64, the front end's feature capacity)."""
    rng = np.random.default_rng(seed)
    cap = (M + 63) // 64 * 64
    keep = rng.random((P, C, M)) < present
    counts = keep.sum(2).astype(np.int32)
    ids = np.zeros((P, C, cap), np.int32)
    xy = np.zeros((P, C, cap, 2), np.float32)
    for p in range(P):
        for j in range(C):
            i = np.nonzero(keep[p, j])[0]
            ids[p, j, :len(i)] = i
            xy[p, j, :len(i)] = rng.uniform(0, 1200, (len(i), 2))
    return counts, ids, xy


def stage_main(a):
    """--stage: the device staging chain against the host's staging of the same windows."""
    counts, ids, xy = window_lists(a.problems, a.cams, a.points, a.present, 0)
    ctx = S.Context(0)
    ms = ctx.ba_time_staging(counts, ids, xy, reps=a.reps)
    print(json.dumps({"name": "ba_staging", "problems": a.problems, "cams": a.cams, "points": a.points,
                      "observations": int(counts.sum()), "reps": a.reps,
                      "ms_device_chain": round(ms["ms_device"], 4),
                      "ms_host_readback": round(ms["ms_host_readback"], 3),
                      "ms_host_sort_and_upload": round(ms["ms_host_stage"], 3),
                      "list_bytes": int(ids.nbytes + xy.nbytes + counts.nbytes)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--stage", action="store_true",
                    help="time the device staging chain (svo_ba_time_staging) instead of the LM iteration")
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--cams", type=int, default=8)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--present", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--huber", type=float, default=2.0)
    a = ap.parse_args()
    if a.stage:
        return stage_main(a)
    poses, fixed, X, oc, op, oxy, n_obs = problems(a.problems, a.cams, a.points, a.present, 0)
    ctx = S.Context(0)
    ms = ctx.ba_time_iteration(poses, fixed, X, oc, op, oxy, K, lam=1e-4, huber_delta=a.huber, reps=a.reps,
                               n_obs=n_obs)
    p2, x2, costs, its = ctx.bundle_adjust(poses, fixed, X, oc, op, oxy, K, n_obs=n_obs, huber_delta=a.huber,
                                           max_iterations=10)
    # compulsory traffic of one iteration (each stage reads its inputs once): per
    # observation the camera passes (full + cost) read index, point index, xy and the
    # point (40 B each), the three point-side stages camera index and xy (12 B each);
    # per point the stages read X (24 B) four times and V*^-1, gp, the flag (76 B)
    # twice and write V, gp, V*^-1, the flag (124 B) and the trial point (24 B)
    O, Mtot = int(n_obs.sum()), a.problems * a.points
    moved = O * (2 * 40 + 3 * 12) + Mtot * (4 * 24 + 2 * 76 + 124 + 24)
    print(json.dumps({"name": "ba_lm_iteration", "problems": a.problems, "cams": a.cams, "points": a.points,
                      "observations": O, "reps": a.reps, "ms_per_iteration": round(ms, 4),
                      "modelled_bytes": moved, "modelled_GBps": round(moved / ms / 1e6, 1),
                      "cost_before": float(costs[:, 0].sum()), "cost_after_10": float(costs[:, 1].sum()),
                      "iterations_max": int(its.max())}))


if __name__ == "__main__":
    main()
