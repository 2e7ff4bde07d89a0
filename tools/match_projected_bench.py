#!/usr/bin/env python3
"""The guided search, measured (profiles/match_projected_timing.txt).

--problems problems (default 256) of --n map points x --n keypoints (default 2000)
on a 1241x376 frame: keypoints uniform over the frame with random descriptors;
every point is a keypoint's pixel jittered by up to 2 px, back-projected at a
random depth under a small pose, with the keypoint's descriptor and up to 40 bits
flipped. For each radius (default 4 and 16): svo_match_projected_time's three
figures (bin, match, pairs; HIP-event ms per launch, no transfers), the match
kernel's figure with a quarter wave per point (SVO_PROJ_LANES=16), the candidates
per visible point counted on the host for problem 0, the pairs the call returns,
and, in the same process, svo_match_hamming_time on the same descriptor sets: one
direction of the brute force the search stands in for. Every timing call is made
--calls times and every sample is printed. One JSON line on stdout."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import svo_amd as S  # noqa: E402

W, H = 1241, 376
K4 = np.array([718.856, 718.856, 607.1928, 185.2157])


def problems(P, n, seed=0):
    rng = np.random.default_rng(seed)
    kxy = (rng.uniform(0, 1, (P, n, 2)) * [W, H]).astype(np.float32)
    kdesc = rng.integers(0, 256, (P, n, 32), dtype=np.uint8)
    T = np.tile(np.r_[np.eye(3).ravel(), np.zeros(3)], (P, 1))
    T[:, 9:] = rng.uniform(-0.05, 0.05, (P, 3))
    j = np.stack([rng.permutation(n) for _ in range(P)])  # every keypoint is some point's origin
    px = np.take_along_axis(kxy, j[:, :, None], axis=1).astype(np.float64) + rng.uniform(-2, 2, (P, n, 2))
    z = rng.uniform(4, 40, (P, n))
    xc = np.stack([(px[..., 0] - K4[2]) / K4[0] * z, (px[..., 1] - K4[3]) / K4[1] * z, z], axis=-1)
    xyz = xc - T[:, None, 9:]  # R = I
    pdesc = np.take_along_axis(kdesc, j[:, :, None], axis=1)
    flips = rng.integers(0, 256, (P, n, 40))
    use = (np.arange(40) < rng.integers(0, 41, (P, n, 1))).astype(np.uint8)  # the first k of 40 positions
    mask = np.zeros((P, n, 256), np.uint8)
    np.put_along_axis(mask, flips, use, axis=2)
    pdesc = pdesc ^ np.packbits(mask, axis=2)
    return xyz, np.ascontiguousarray(pdesc), kxy, kdesc, T


def candidates(xyz, kxy, T, radius):
    """Candidates per visible point of one problem, on the host (rules 1 and 2)."""
    p = xyz @ T[:9].reshape(3, 3).T + T[9:]
    uf = (K4[0] * (p[:, 0] / p[:, 2]) + K4[2]).astype(np.float32)
    vf = (K4[1] * (p[:, 1] / p[:, 2]) + K4[3]).astype(np.float32)
    vis = (p[:, 2] > 0) & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
    r = np.float32(radius)
    n = [(int(((np.abs(kxy[:, 0] - uf[i]) <= r) & (np.abs(kxy[:, 1] - vf[i]) <= r)).sum())) for i in np.nonzero(vis)[0]]
    return int(vis.sum()), float(np.mean(n)), int(np.max(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--radius", type=float, nargs="+", default=[4.0, 16.0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    ctx = S.Context(0)
    P, n = a.problems, a.n
    xyz, pdesc, kxy, kdesc, T = problems(P, n)
    counts = np.full(P, n, np.int32)
    out = {"measurement": "match_projected_bench", "problems": P, "points": n, "keypoints": n, "size": [W, H],
           "reps": a.reps, "radius": {}}
    for radius in a.radius:
        prm = S.ProjMatchParams(radius=radius)
        os.environ["SVO_PROJ_LANES"] = "16"  # the other launch shape of proj_match_kernel: a quarter wave per point
        ms16 = [ctx.match_projected_time(xyz, pdesc, kxy, kdesc, T, K4, (W, H), counts, counts, prm, a.reps)
                for _ in range(a.calls)]
        del os.environ["SVO_PROJ_LANES"]
        ms = [ctx.match_projected_time(xyz, pdesc, kxy, kdesc, T, K4, (W, H), counts, counts, prm, a.reps)
              for _ in range(a.calls)]
        brute = [ctx.match_hamming_time(pdesc, kdesc, counts, counts, a.reps) for _ in range(a.calls)]
        npairs = ctx.match_projected(xyz, pdesc, kxy, kdesc, T, K4, (W, H), prm, counts, counts)[4]
        vis, mean_c, max_c = candidates(xyz[0], kxy[0], T[0], radius)
        best = min(float(m.sum()) for m in ms)
        out["radius"][str(radius)] = {
            "ms_bin_match_pairs": [[round(float(v), 4) for v in m] for m in ms],
            "ms_guided_total": [round(float(m.sum()), 4) for m in ms],
            "ms_match_quarter_wave_per_point": [round(float(m[1]), 4) for m in ms16],
            "ms_hamming_one_direction": [round(b, 4) for b in brute],
            "brute_over_guided": round(min(brute) / best, 1),
            "visible_points_problem0": vis, "candidates_per_visible_point": round(mean_c, 2), "candidates_max": max_c,
            "pairs_median": int(np.median(npairs))}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
