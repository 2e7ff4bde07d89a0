#!/usr/bin/env python3
"""The rectifying ingest measured.

kernel: the rectifying kernel against the plain ingest kernel on the same
    staging block (svo_frontend_time_ingest: HIP events, 20 launches after a
    warm-up), 256 sequences x 1241x376, one eye, grey and BGR, alternating in one
    process.
loop:   bench.py's streamed leg (stream_workload: its sizes, ring and timing) with
    rectification on against off at the same frame size, grey, alternating.

One JSON line per measurement on stdout. --profile-pass: only a few launches of
each kernel and nothing timed, for a `rocprofv3 --kernel-trace --stats` run."""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import svo_amd as S  # noqa: E402
from svo_amd.scene import Scene  # noqa: E402

W, H, N, ML, _ = bench.CONFIGS["kitti"]
# a rig of the size of the test's distortions, the raw frame of the config's size
DIST = {"left": (-0.08, 0.02, 5e-4, -3e-4, 0, 0, 0, 0), "right": (-0.075, 0.018, -4e-4, 2e-4, 0, 0, 0, 0)}
RVEC = {"left": (0.004, -0.003, 0.002), "right": (0.004, 0.003, 0.002)}


def rodrigues(v):
    v = np.asarray(v, np.float64)
    th = float(np.linalg.norm(v))
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def rig_maps(ctx, K):
    return [S.RectMaps(ctx, W, H, *S.init_undistort_rectify_map(K, DIST[e], rodrigues(RVEC[e]), K, W, H))
            for e in ("left", "right")]


def kernel(ctx, seqs, reps, rounds, profile_pass):
    n_dist = min(seqs, 4)
    scs = [Scene(W, H, seed=1 + i) for i in range(n_dist)]
    ml, mr = rig_maps(ctx, scs[0].K)
    for bgr in (False, True):
        shape = (n_dist, H, W, 3) if bgr else (n_dist, H, W)
        pl, pr = S.PinnedBuffer(shape), S.PinnedBuffer(shape)
        for i, sc in enumerate(scs):
            pl.array[i] = sc.frame(0)[..., None] if bgr else sc.frame(0)
            pr.array[i] = sc.right(0)[..., None] if bgr else sc.right(0)
        fe = S.Frontend(ctx, S.FrontendConfig(W, H, scs[0].K, n_seq=seqs, n_frames=4, n_features=N, max_level=ML))
        fe.set_rectification(ml, mr)
        fe.queue_frames(0, [pl.array[s % n_dist] for s in range(seqs)], [pr.array[s % n_dist] for s in range(seqs)])
        fe.upload_wait(0)
        if profile_pass:
            for rect in (True, False):
                fe.time_ingest(0, rect, 3)
        else:
            ms = {True: [], False: []}
            for _ in range(rounds):
                for rect in (True, False):
                    ms[rect].append(fe.time_ingest(0, rect, reps))
            r, p = float(np.median(ms[True])), float(np.median(ms[False]))
            px = seqs * W * H
            print(json.dumps({"measurement": "kernel", "input": "BGR 8UC3" if bgr else "grey", "sequences": seqs,
                              "size": [W, H], "launches_per_run": reps, "rectify_ms": [round(v, 4) for v in ms[True]],
                              "ingest_ms": [round(v, 4) for v in ms[False]], "rectify_ms_median": round(r, 4),
                              "ingest_ms_median": round(p, 4), "ratio": round(r / p, 3),
                              "rectify_GBps_algorithmic": round(px * (4 if bgr else 2) / r / 1e6, 1),
                              "ingest_GBps_algorithmic": round(px * (4 if bgr else 2) / p / 1e6, 1)}), flush=True)
        fe.close()
        pl.close()
        pr.close()
    ml.close()
    mr.close()


def loop(ctx, seqs, steps, warmup, rounds):
    n_dist = min(seqs, 16)
    scs = [Scene(W, H, seed=bench.sequence_seeds(0, n_dist)[i]) for i in range(n_dist)]
    P = min(warmup + steps + 3, 2 * scs[0].period)
    pairs = [[(sc.frame(t), sc.right(t)) for t in range(P)] for sc in scs]
    ml, mr = rig_maps(ctx, scs[0].K)

    class RectFrontend(S.Frontend):
        def __init__(self, c, cfg):
            super().__init__(c, cfg)
            self.set_rectification(ml, mr)

    on = types.SimpleNamespace(**{k: getattr(S, k) for k in dir(S) if not k.startswith("__")})
    on.Frontend = RectFrontend
    out = {"off": [], "on": []}
    for _ in range(rounds):
        for name, mod in (("off", S), ("on", on)):
            r = bench.stream_workload(mod, Scene, ctx, W, H, N, ML, seqs, steps, warmup, 0, False, scs[0].K,
                                      pairs=pairs)
            out[name].append(r)
    print(json.dumps({"measurement": "streamed loop", "input": "grey", "sequences": seqs, "steps": steps,
                      "warmup": warmup,
                      **{f"{k}_frames_per_s": [r["value"] for r in v] for k, v in out.items()},
                      **{f"{k}_h2d_GBps_in_loop": [r["h2d_GBps_in_loop"] for r in v] for k, v in out.items()},
                      **{f"{k}_h2d_GBps_alone": [r["h2d_GBps_alone"] for r in v] for k, v in out.items()}}),
          flush=True)
    ml.close()
    mr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "loop", "all"))
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    ctx = S.Context(0)
    if a.what in ("kernel", "all"):
        kernel(ctx, a.seq, a.reps, a.rounds, a.profile_pass)
    if a.what in ("loop", "all") and not a.profile_pass:
        loop(ctx, a.seq, a.steps, a.warmup, a.rounds)
    ctx.close()


if __name__ == "__main__":
    main()
