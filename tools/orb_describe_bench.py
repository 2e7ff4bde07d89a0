#!/usr/bin/env python3
"""What the ORB descriptor kernels and the Hamming matcher cost (HIP events, no
transfers; svo_orb_describe_time / svo_match_hamming_time):
  describe: `images` distinct 1241x376 synthetic canvases at the default ORB
    parameters (150 features, 8 levels, patch 31, WTA_K 2), one after the other;
    per image ms per launch of orb_blur_kernel (all levels), orb_angle_kernel and
    orb_brief_kernel over `reps` launches, summed over the images. The kernels are
    per image, so `images` images cost `images` launches of each.
  match: `problems` problems of `n` x `n` random descriptors in ONE launch of
    hamming_knn2_kernel, ms per launch over `reps` launches; beside it the
    algorithmic bytes (queries and train rows read once, idx and dist written) and
    the popcount rate (8 per pair of descriptors).
Prints one JSON line. Not a test and not the project's benchmark (bench.py)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svo_amd as S  # noqa: E402
from svo_amd.scene import synth_canvas  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx = S.Context(0)
    prm = S.OrbParams(wta_k=2)
    tot = np.zeros(3)
    nkp = 0
    for i in range(a.images):
        g = ctx.image(synth_canvas(1000 + i, 1241, 376, 1241 * 376 // 250), max_levels=0)
        ms, n = ctx.orb_describe_time(g, prm, reps=a.reps)
        tot += ms
        nkp += n
        g.close()
    rng = np.random.default_rng(0)
    P, n = a.problems, a.n
    q = rng.integers(0, 256, (P, n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (P, n, 32), dtype=np.uint8)
    cnt = np.full(P, n, np.int32)
    runs = [ctx.match_hamming_time(q, t, cnt, cnt, reps=max(a.reps // 4, 1)) for _ in range(3)]
    ms_match = float(np.median(runs))
    pairs = P * n * n
    out = {
        "measurement": "orb_describe_bench", "images": a.images, "reps": a.reps, "keypoints_total": nkp,
        "ms_blur_sum": round(tot[0], 4), "ms_angle_sum": round(tot[1], 4), "ms_brief_sum": round(tot[2], 4),
        "ms_blur_per_image": round(tot[0] / a.images, 5), "ms_angle_per_image": round(tot[1] / a.images, 5),
        "ms_brief_per_image": round(tot[2] / a.images, 5),
        "match_problems": P, "match_n": n, "ms_match": [round(r, 4) for r in runs], "ms_match_median": round(ms_match, 4),
        "match_algorithmic_bytes": P * (2 * n * 32 + n * 16),
        "match_popcounts": pairs * 8,
        "match_gpopc_per_s": round(pairs * 8 / (ms_match * 1e-3) / 1e9, 1),
        "match_gpairs_per_s": round(pairs / (ms_match * 1e-3) / 1e9, 2),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
