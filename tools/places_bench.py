#!/usr/bin/env python3
"""The place memory, measured (profiles/places_timing.txt).

The batched front end at KITTI size (256 sequences x 1241x376, 2000 features,
SVO_KF_EVERY) with svo_frontend_places_enable(8 slots, every frame): --steps
steps fill the ring, then svo_frontend_places_time gives the HIP-event time of
one record (blur, describe, compaction, point copy over all sequences) and of a
query's device half (the query set, the 2-NN of every (sequence, record) problem
in both directions, the filter); the call is made --calls times and every sample
is printed. Then one whole svo_frontend_places_query in wall
time: the device half, the choice of the record and the host's RANSAC of every
sequence, one after the other. Also the wall ms per step with the memory and
without it, same process. One JSON line on stdout."""
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
from svo_amd.scene import Scene  # noqa: E402

W, H, N, ML, _ = bench.CONFIGS["kitti"]


def run(ctx, pairs, sc0, seqs, steps, slots, calls):
    T = steps + 2
    P0, P1 = sc0.projections()
    fe = S.Frontend(ctx, S.FrontendConfig(W, H, sc0.K, n_seq=seqs, n_frames=T, n_features=N, max_level=ML, P_left=P0,
                                          P_right=P1))
    bench.upload_resident(fe, pairs, seqs, T)
    if slots:
        fe.places_enable(slots, 1, 31)
    fe.init(0)
    fe.step(1)
    fe.synchronize()
    t0 = time.perf_counter()
    for t in range(2, steps + 1):
        fe.step(t)
    fe.synchronize()
    out = {"ms_per_step": round((time.perf_counter() - t0) / (steps - 1) * 1e3, 4)}
    if slots:
        samples = [fe.places_time() for _ in range(calls)]
        out.update(problems=samples[0][2], ms_record=[round(s[0], 4) for s in samples],
                   ms_query_device=[round(s[1], 4) for s in samples],
                   record_entries_seq0=[len(fe.place(0, k)["desc"]) for k in range(slots)])
        t0 = time.perf_counter()
        res = fe.places_query(0, steps - 1)  # every record but the frame's own
        out.update(ms_query_wall=round((time.perf_counter() - t0) * 1e3, 3), query_ok=int(res["ok"].sum()),
                   query_pairs_median=int(np.median(res["n_pairs"])),
                   query_inliers_median=int(np.median(res["n_inliers"])))
    fe.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=8)
    a = ap.parse_args()
    ctx = S.Context(0)
    n_dist = min(a.seq, a.distinct)
    scs = [Scene(W, H, seed=bench.sequence_seeds(0, n_dist)[i]) for i in range(n_dist)]
    T = a.steps + 2
    pairs = [bench.PinnedPairs(S, sc, min(T, 2 * sc.period)) for sc in scs]
    on = run(ctx, pairs, scs[0], a.seq, a.steps, a.slots, a.calls)
    off = run(ctx, pairs, scs[0], a.seq, a.steps, 0, 0)
    print(json.dumps({"measurement": "places_bench", "sequences": a.seq, "size": [W, H], "features": N,
                      "slots": a.slots, "steps": a.steps, **on, "ms_per_step_without": off["ms_per_step"]}), flush=True)
    for p in pairs:
        p.close()
    ctx.close()


if __name__ == "__main__":
    main()
