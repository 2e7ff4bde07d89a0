#!/usr/bin/env python3
"""What the motion-only stereo refinement costs on the front end's shape: 256
problems x 2000 points, 95 % of the observations stereo, 0.5 px noise, 5 %
outliers, Huber 2, 10 iterations from a start 0.1 m / 0.005 rad off.
svo_refine_poses_time: ms per whole LM launch of svo_refine_poses_stereo (HIP
events, `reps` launches after a warm-up) beside the wall time per call of
svo_refine_poses, the host loop with one round trip per iteration, on the same
left pixels; `runs` times. ms_device is the launch alone; ms_host contains the host
loop's upload of the points and pixels, so beside them the wall time of the two
whole calls from numpy arrays (upload, LM, download: ms_call_stereo, ms_call_host).
Also the iterations the device run takes and its cost, so the timed work is known.
Prints one JSON line. Not a test and not the project's benchmark (bench.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svo_amd as S  # noqa: E402

K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])
BASELINE = 0.54


def batch(P, n, stereo_share, seed):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-8, 8, (P, n)), rng.uniform(-3, 3, (P, n)), rng.uniform(5, 40, (P, n))], 2)
    t = rng.normal(0, 0.3, (P, 3))
    Pc = X + t[:, None]  # the true cameras do not rotate
    u = np.stack([K[0, 0] * Pc[..., 0] / Pc[..., 2] + K[0, 2], K[1, 1] * Pc[..., 1] / Pc[..., 2] + K[1, 2]], 2)
    ur = K[0, 0] * (Pc[..., 0] - BASELINE) / Pc[..., 2] + K[0, 2]
    u += rng.normal(0, 0.5, u.shape)
    ur += rng.normal(0, 0.5, ur.shape)
    m = rng.random((P, n)) < 0.05
    u[m] += rng.uniform(-60, 60, (int(m.sum()), 2))
    ur = np.where((rng.random((P, n)) < stereo_share) & (ur >= 0), ur, -1.0)
    T0 = np.tile(np.r_[np.eye(3).ravel(), 0, 0, 0], (P, 1))
    T0[:, 9:] = t + rng.normal(0, 0.06, (P, 3))  # ~0.1 m off
    w = rng.normal(0, 0.003, (P, 3))             # ~0.005 rad off (first order)
    for p in range(P):
        W = np.array([[0, -w[p, 2], w[p, 1]], [w[p, 2], 0, -w[p, 0]], [-w[p, 1], w[p, 0], 0]])
        Q, _ = np.linalg.qr(np.eye(3) + W)
        T0[p, :9] = (Q * np.sign(np.diag(Q))).ravel()
    return X, u.astype(np.float32), ur.astype(np.float32), T0


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--stereo", type=float, default=0.95)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--huber", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    ctx = S.Context(0)
    X, xy, ur, T0 = batch(a.problems, a.points, a.stereo, 0)
    _, costs, its, _ = ctx.refine_poses_stereo(X, xy, ur, T0, K, BASELINE, huber_delta=a.huber,
                                               max_iterations=a.iterations)
    dev, host = [], []
    for _ in range(a.runs):
        r = ctx.refine_poses_time(X, xy, ur, T0, K, BASELINE, huber_delta=a.huber, max_iterations=a.iterations,
                                  reps=a.reps)
        dev.append(round(r["ms_device"], 4))
        host.append(round(r["ms_host"], 4))
    call_s, call_h = [], []
    for _ in range(a.runs + 1):  # (the first pair is the warm-up)
        t0 = time.perf_counter()
        ctx.refine_poses_stereo(X, xy, ur, T0, K, BASELINE, huber_delta=a.huber, max_iterations=a.iterations)
        t1 = time.perf_counter()
        ctx.refine_poses(X, xy, T0, K, huber_delta=a.huber, max_iterations=a.iterations)
        t2 = time.perf_counter()
        call_s.append(round(1e3 * (t1 - t0), 4))
        call_h.append(round(1e3 * (t2 - t1), 4))
    md, mh = float(np.median(dev)), float(np.median(host))
    print(json.dumps({"measurement": "svo_refine_poses_time", "problems": a.problems, "points": a.points,
                      "stereo_share": round(float(np.mean(ur >= 0)), 4), "huber": a.huber,
                      "max_iterations": a.iterations, "reps": a.reps, "ms_device": dev, "ms_host": host,
                      "ms_device_median": md, "ms_host_median": mh, "host_over_device": round(mh / md, 2),
                      "ms_call_stereo": call_s[1:], "ms_call_host": call_h[1:],
                      "ms_call_stereo_median": float(np.median(call_s[1:])),
                      "ms_call_host_median": float(np.median(call_h[1:])),
                      "device_iterations_min_median_max": [int(its.min()), float(np.median(its)), int(its.max())],
                      "cost_initial_final_median": [float(np.median(costs[:, 0])), float(np.median(costs[:, 1]))]}))


if __name__ == "__main__":
    main()
