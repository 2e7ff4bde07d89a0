#!/usr/bin/env python3
"""Row SAD as the front end's stereo match, measured.

phase: the batched front end with timing = 1 on one scene (a rig at KITTI's own
    fx * b = 386.1448: 18-129 px of disparity at 1241x376), 256 sequences x 2000
    features, SVO_KF_EVERY, with and without svo_frontend_set_stereo_matcher,
    alternating in one process: phase 3 (stereo_lk) ms per step -- the matcher's
    kernel against the stereo LK's -- and what each keyframe adds.
step:   the same front end WITHOUT the matcher and without timers: wall ms per
    step. One process per call and one JSON line, so that a shell loop can
    alternate two builds of the library (SVO_GPU_LIB names the other one).

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
from svo_amd.scene import STEREO_BF, Scene  # noqa: E402

W, H, N, ML, _ = bench.CONFIGS["kitti"]
KITTI_BF = 386.1448


class Rig(Scene):
    """Scene whose right view and projections default to the rig's fx * b."""
    bf = KITTI_BF

    def right(self, t, bf=None):
        return super().right(t, self.bf if bf is None else bf)

    def projections(self, bf=None):
        return super().projections(self.bf if bf is None else bf)


def rig(seed, bf):
    sc = Rig(W, H, seed=seed)
    sc.bf = bf
    return sc


def run(ctx, pairs, sc0, seqs, steps, warmup, timing, rows):
    """One front end over the resident pairs: init, warm-up, `steps` timed steps."""
    T = warmup + steps + 2
    P0, P1 = sc0.projections()
    fe = S.Frontend(ctx, S.FrontendConfig(W, H, sc0.K, n_seq=seqs, n_frames=T, n_features=N, max_level=ML,
                                          timing=timing, P_left=P0, P_right=P1))
    if rows is not None:
        fe.set_stereo_matcher(rows)
    bench.upload_resident(fe, pairs, seqs, T)
    fe.init(0)
    for t in range(1, warmup + 1):
        fe.step(t)
    fe.synchronize()
    fe.reset_times()
    tot = {"added": 0, "tracked": 0, "inliers": 0, "serial_keyframe": 0}
    t0 = time.perf_counter()
    for t in range(warmup + 1, warmup + steps + 1):
        st = fe.step(t).as_dict()
        for k in tot:
            tot[k] += st[k]
    fe.synchronize()
    dt = time.perf_counter() - t0
    out = {"ms_per_step": round(dt / steps * 1e3, 4), **{k + "_per_step": round(v / steps, 2) for k, v in tot.items()}}
    if timing:
        ms, launches = fe.phase_times()["stereo_lk"]
        out["stereo_ms_per_step"] = round(ms / steps, 4)
        out["stereo_launches_per_step"] = round(launches / steps, 2)
    fe.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("phase", "step"))
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--bf", type=float, default=KITTI_BF)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    ctx = S.Context(0)
    n_dist = min(a.seq, a.distinct)
    bf = a.bf if a.what == "phase" else STEREO_BF
    scs = [rig(bench.sequence_seeds(0, n_dist)[i], bf) for i in range(n_dist)]
    T = a.warmup + a.steps + 2
    pairs = [bench.PinnedPairs(S, sc, min(T, 2 * sc.period)) for sc in scs]
    base = {"sequences": a.seq, "size": [W, H], "features": N, "steps": a.steps, "warmup": a.warmup,
            "distinct_sequences": n_dist, "fx_b": round(bf, 4)}
    if a.what == "phase":
        rows = S.StereoRowsParams()
        res = {"stereo_lk": [], "row_sad": []}
        for _ in range(a.rounds):
            for name, p in (("stereo_lk", None), ("row_sad", rows)):
                res[name].append(run(ctx, pairs, scs[0], a.seq, a.steps, a.warmup, 1, p))
        med = {k: float(np.median([r["stereo_ms_per_step"] for r in v])) for k, v in res.items()}
        print(json.dumps({"measurement": "phase 3 (stereo_lk), timing = 1", **base,
                          "params": {k: getattr(rows, k) for k, _ in rows._fields_}, "runs": res,
                          "stereo_lk_ms_per_step_median": round(med["stereo_lk"], 4),
                          "row_sad_ms_per_step_median": round(med["row_sad"], 4),
                          "ratio": round(med["row_sad"] / med["stereo_lk"], 3)}), flush=True)
    else:
        r = run(ctx, pairs, scs[0], a.seq, a.steps, a.warmup, 0, None)
        print(json.dumps({"measurement": "step without the matcher, timing = 0", **base, "label": a.label,
                          "library": os.path.basename(os.path.dirname(S.lib_path())) + "/" +
                          os.path.basename(S.lib_path()), **r}), flush=True)
    for p in pairs:
        p.close()
    ctx.close()


if __name__ == "__main__":
    main()
