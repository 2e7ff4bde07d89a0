#!/usr/bin/env python3
"""What stereo observations cost the windowed bundle adjustment, on a window-shaped
batch (256 problems x 16 cameras x 2000 points, about 70 % of the possible
observations present; tools/ba_bench.py's generator).
--mode iteration: ms per Levenberg-Marquardt iteration of the monocular path
(svo_ba_time_iteration, HIP events), `runs` times; with SVO_GPU_LIB naming another
build of the library this is the A/B measurement of the monocular kernels.
--mode stereo: wall time of svo_bundle_adjust against svo_bundle_adjust_stereo at a
fixed max_iterations on the same batch, with one observation per point stereo (the
front end's share: the camera that created the point) and with all of them stereo;
the median of `runs` calls each, after one warm-up call, at `iterations` and at twice
as many: the calls' difference is the LM iterations alone (the host's staging and
the transfers are the same in both) and gives the ms per iteration of each variant.
Prints one JSON line. Not a test and not the project's benchmark (bench.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svo_amd as S  # noqa: E402
from ba_bench import K, problems  # noqa: E402

BASELINE = 0.54


def right_columns(poses, X, oc, op, n_obs, share, seed):
    """ur per observation from the state the batch starts at (+ N(0, 0.5) px);
    share "one": stereo only in camera (point index mod cameras), "all": everywhere."""
    rng = np.random.default_rng(seed)
    P, C = poses.shape[:2]
    ur = np.full(oc.shape, -1.0, np.float32)
    for p in range(P):
        n = n_obs[p]
        c, i = oc[p, :n], op[p, :n]
        Pc = X[p, i] + poses[p, c, 9:]  # the generator's cameras do not rotate
        u = K[0, 0] * (Pc[:, 0] - BASELINE) / Pc[:, 2] + K[0, 2] + rng.normal(0, 0.5, n)
        on = (u >= 0) & (Pc[:, 2] > 0)
        if share == "one":
            on &= c == i % C
        ur[p, :n] = np.where(on, u, -1.0)
    return ur


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--mode", choices=("iteration", "stereo"), default="iteration")
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--present", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--huber", type=float, default=2.0)
    ap.add_argument("--variants", default="monocular,one,all",
                    help="--mode stereo: which of them to run (a kernel trace of one share at a time)")
    a = ap.parse_args()
    poses, fixed, X, oc, op, oxy, n_obs = problems(a.problems, a.cams, a.points, a.present, 0)
    ctx = S.Context(0)
    out = {"name": "ba_stereo_" + a.mode, "lib": os.environ.get("SVO_GPU_LIB", "default"), "problems": a.problems,
           "cams": a.cams, "points": a.points, "observations": int(n_obs.sum())}
    if a.mode == "iteration":
        out["ms_per_iteration"] = [round(ctx.ba_time_iteration(poses, fixed, X, oc, op, oxy, K, lam=1e-4,
                                                                huber_delta=a.huber, reps=a.reps, n_obs=n_obs), 4)
                                   for _ in range(a.runs)]
    else:
        def wall(iterations, **kw):
            ts = []
            for r in range(a.runs + 1):
                t0 = time.perf_counter()
                res = ctx.bundle_adjust(poses, fixed, X, oc, op, oxy, K, n_obs=n_obs, huber_delta=a.huber,
                                        max_iterations=iterations, **kw)
                ts.append(time.perf_counter() - t0)
            return 1e3 * float(np.median(ts[1:])), int(res[3].sum())

        out["max_iterations"] = a.iterations
        variants = {"monocular": {}}
        shares = [v for v in ("one", "all") if v in a.variants.split(",")]
        for share in shares:
            ur = right_columns(poses, X, oc, op, n_obs, share, 1)
            out[f"stereo_share_{share}"] = round(float((ur >= 0).sum()) / float(n_obs.sum()), 4)
            variants["stereo_" + share] = dict(obs_ur=ur, baseline=BASELINE)
        for name, kw in variants.items():
            (ms1, it1), (ms2, it2) = wall(a.iterations, **kw), wall(2 * a.iterations, **kw)
            out[name] = {"ms_call": round(ms1, 2), "ms_call_twice_the_iterations": round(ms2, 2),
                         "iterations_begun": [it1, it2], "ms_per_lm_iteration": round((ms2 - ms1) / a.iterations, 3)}
        for share in shares:
            out[f"ratio_call_{share}"] = round(out["stereo_" + share]["ms_call"] / out["monocular"]["ms_call"], 3)
            out[f"ratio_lm_iteration_{share}"] = round(out["stereo_" + share]["ms_per_lm_iteration"] /
                                                       out["monocular"]["ms_per_lm_iteration"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
