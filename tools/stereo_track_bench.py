#!/usr/bin/env python3
"""Stereo columns for tracked features, measured.

step:    the batched front end at KITTI size (256 sequences x 1241x376, 2000
    features, SVO_KF_EVERY, stereo window 4, the stereo LK at the keyframe) with
    svo_frontend_set_stereo_tracking at --guide (or --guide -1: never called):
    wall ms per step (timing = 0) or phase_ms_per_step (--timing), and the
    window's stereo share. One process per call, one JSON line.
    (The front end without any window against the parent commit's library is
    tools/stereo_rows_bench.py's `step` leg.)
kernels: both rules in one process for `rocprofv3 --kernel-trace --stats -- python
    tools/stereo_track_bench.py kernels`: a front end at guide 4 (per step one
    stereo_rows_guided_kernel, one stereo_rows_noprior_kernel, one
    row_priors_kernel) and one at guide 0 (per step one stereo_rows_kernel over the
    same tracked features; the keyframes use the stereo LK, so no other launch
    bears that name). Each front end's init adds one launch over empty lists.
ba:      the forward scene (640x376, seeds 3 and 8, KITTI's baseline, 800
    features, 6 frames, window 6, 2 fixed frames, Huber 2, 10 iterations), --seq
    sequences: svo_frontend_bundle_adjust_stereo's call time and the worst
    camera-centre error against the scene's truth before (PnP) and after it, with
    the creation-only columns and with every frame's (over the whole window, and over
    the free frames alone: the two fixed frames keep their PnP poses).

One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import svo_amd as S  # noqa: E402
from svo_amd.scene import Scene, SceneForward  # noqa: E402

W, H, N, ML, _ = bench.CONFIGS["kitti"]
KITTI_BASELINE = 0.537
WINDOW = 4


def share(fe, q=0):
    ur = np.concatenate(fe.window(q)["ur"])
    return round(float(np.mean(ur >= 0)), 4), int(len(ur))


def run_step(ctx, pairs, sc0, seqs, steps, warmup, timing, guide):
    T = warmup + steps + 2
    P0, P1 = sc0.projections()
    fe = S.Frontend(ctx, S.FrontendConfig(W, H, sc0.K, n_seq=seqs, n_frames=T, n_features=N, max_level=ML,
                                          timing=timing, P_left=P0, P_right=P1))
    bench.upload_resident(fe, pairs, seqs, T)
    fe.window_enable(WINDOW, stereo=True)
    if guide >= 0:
        fe.set_stereo_tracking(S.StereoRowsParams(), guide)
    fe.init(0)
    for t in range(1, warmup + 1):
        fe.step(t)
    fe.synchronize()
    fe.reset_times()
    tracked = 0
    t0 = time.perf_counter()
    for t in range(warmup + 1, warmup + steps + 1):
        st = fe.step(t).as_dict()
        tracked += st["inliers"]
    fe.synchronize()
    dt = time.perf_counter() - t0
    sh, nobs = share(fe)
    out = {"guide": guide, "ms_per_step": round(dt / steps * 1e3, 4), "matched_features_per_step": round(tracked / steps, 1),
           "window_stereo_share_seq0": sh, "window_observations_seq0": nobs}
    if timing:
        out["phase_ms_per_step"] = {k: round(v[0] / steps, 4) for k, v in fe.phase_times().items()}
    fe.close()
    return out


def forward(seed):
    sc = SceneForward(640, 376, seed=seed)
    bf = float(sc.K[0, 0]) * KITTI_BASELINE
    return sc, bf


def centre_errors(fe, scs, n_seq, first=0):
    """Worst |C - C_true| over the window's frames from index `first` on and the sequences, metres."""
    worst = 0.0
    for q in range(n_seq):
        w = fe.window(q)
        sc = scs[q % len(scs)][0]
        for t, P in list(zip(w["frame_t"], w["poses"]))[first:]:
            R, tv = np.asarray(P[:9]).reshape(3, 3), np.asarray(P[9:])
            worst = max(worst, float(np.linalg.norm(-R.T @ tv - sc.C(int(t)))))
    return worst


def run_ba(ctx, seqs, guide, calls):
    T, NF, WIN = 6, 800, 6
    scs = [forward(3), forward(8)]
    out = {"guide": guide, "sequences": seqs}
    per_seed = {}
    for only in (None, 0, 1):  # the batch for the call time; each seed alone for its error
        use = scs if only is None else [scs[only]]
        n_seq = seqs if only is None else 1
        sc0, bf = use[0]
        P0, P1 = sc0.projections(bf)
        call_ms = []
        for rep in range(calls if only is None else 1):
            fe = S.Frontend(ctx, S.FrontendConfig(640, 376, sc0.K, n_seq=n_seq, n_frames=T, n_features=NF, P_left=P0,
                                                  P_right=P1))
            fe.set_stereo_matcher(S.StereoRowsParams())
            for q in range(n_seq):
                sc, b = use[q % len(use)]
                for t in range(T):
                    fe.set_frame(q, t, sc.frame(t), sc.right(t, b))
            fe.window_enable(WIN, stereo=True)
            if guide >= 0:
                fe.set_stereo_tracking(S.StereoRowsParams(), guide)
            fe.init(0)
            for t in range(1, T):
                fe.step(t)
            fe.synchronize()
            before, before_free = centre_errors(fe, use, n_seq), centre_errors(fe, use, n_seq, 2)
            sh, nobs = share(fe)
            t0 = time.perf_counter()
            costs, its, sizes = fe.bundle_adjust(2, 2.0, 10, stereo=True)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            after, after_free = centre_errors(fe, use, n_seq), centre_errors(fe, use, n_seq, 2)
            fe.close()
        if only is None:
            out.update(call_ms=[round(v, 3) for v in call_ms], call_ms_median=round(float(np.median(call_ms)), 3),
                       stereo_share_seq0=sh, observations_seq0=nobs, iterations_seq0=int(its[0]))
        else:
            per_seed[str((3, 8)[only])] = {"pnp_worst_centre_mm": round(before * 1e3, 2),
                                           "ba_worst_centre_mm": round(after * 1e3, 2),
                                           "pnp_worst_free_centre_mm": round(before_free * 1e3, 2),
                                           "ba_worst_free_centre_mm": round(after_free * 1e3, 2), "stereo_share": sh,
                                           "iterations": int(its[0])}
    out["per_seed"] = per_seed
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("step", "kernels", "ba"))
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--guide", type=int, default=4)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    ctx = S.Context(0)
    if a.what == "ba":
        for g in (-1, a.guide):
            print(json.dumps({"measurement": "svo_frontend_bundle_adjust_stereo on the forward window",
                              **run_ba(ctx, a.seq, g, a.calls)}), flush=True)
        ctx.close()
        return
    n_dist = min(a.seq, a.distinct)
    scs = [Scene(W, H, seed=bench.sequence_seeds(0, n_dist)[i]) for i in range(n_dist)]
    T = a.warmup + a.steps + 2
    pairs = [bench.PinnedPairs(S, sc, min(T, 2 * sc.period)) for sc in scs]
    base = {"sequences": a.seq, "size": [W, H], "features": N, "steps": a.steps, "warmup": a.warmup, "window": WINDOW,
            "label": a.label}
    if a.what == "step":
        r = run_step(ctx, pairs, scs[0], a.seq, a.steps, a.warmup, 1 if a.timing else 0, a.guide)
        print(json.dumps({"measurement": "step with the stereo window, timing = %d" % (1 if a.timing else 0), **base,
                          **r}), flush=True)
    else:
        for g in (4, 0):
            r = run_step(ctx, pairs, scs[0], a.seq, a.steps, a.warmup, 0, g)
            print(json.dumps({"measurement": "kernels (read the profiler's statistics)", **base, **r}), flush=True)
    for p in pairs:
        p.close()
    ctx.close()


if __name__ == "__main__":
    main()
