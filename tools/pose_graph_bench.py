#!/usr/bin/env python3
"""What the pose-graph optimisation costs: 256 problems of the circle scene of
tests/pose_graph_reference.py (one node per metre, odometry noise 0.02 m / 0.002
rad, information diag(sigma^-2), the start the chained odometry, node 0 fixed), at
64 nodes with the loop edges (0,63), (5,40), (20,58) and at 512 nodes with
(0,511), (100,400). `distinct` scenes by seed, tiled to the batch.
svo_pose_graph_time: ms per whole launch of svo_pose_graph_optimize (HIP events,
`reps` launches after a warm-up, no transfers), `runs` times; beside it the LM
iterations the problems took, the conjugate-gradient products per LM iteration
and the costs, so the timed work is known. Prints one JSON line per scene. Not a
test and not the project's benchmark (bench.py)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_graph_reference as R  # noqa: E402
import svo_amd as S  # noqa: E402

SCENES = {"64-nodes-3-loops": (64, R.LOOPS64), "512-nodes-2-loops": (512, [(0, 511), (100, 400)])}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--max-cg", type=int, default=4096)
    ap.add_argument("--huber", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scenes", nargs="*", default=list(SCENES))
    a = ap.parse_args()
    ctx = S.Context(0)
    for name in a.scenes:
        n, loops = SCENES[name]
        made = [R.circle_scene(n, loops, seed=s) for s in range(a.distinct)]
        pick = [made[p % a.distinct] for p in range(a.problems)]
        args = [np.stack([sc[k] for sc in pick]) for k in ("poses", "fixed", "ij", "Z", "info")]
        kw = dict(huber_delta=a.huber, max_iterations=a.iterations, max_cg=a.max_cg)
        poses, costs, its, cgs = ctx.pose_graph_optimize(*args, **kw)
        ms = [round(ctx.pose_graph_time(*args, reps=a.reps, **kw)["ms"], 4) for _ in range(a.runs)]
        per = cgs / np.maximum(its, 1)
        err0 = [R.position_error(sc["poses"], sc["truth"]) for sc in made]
        err1 = [R.position_error(poses[p], made[p]["truth"]) for p in range(min(a.distinct, a.problems))]
        print(json.dumps({"measurement": "svo_pose_graph_time", "scene": name, "problems": a.problems,
                          "distinct": a.distinct, "nodes": n, "edges": int(args[2].shape[1]), "huber": a.huber,
                          "max_iterations": a.iterations, "max_cg": a.max_cg, "reps": a.reps, "ms_launch": ms,
                          "ms_launch_median": float(np.median(ms)),
                          "lm_iterations_min_median_max": [int(its.min()), float(np.median(its)), int(its.max())],
                          "cg_products_total_min_median_max": [int(cgs.min()), float(np.median(cgs)), int(cgs.max())],
                          "cg_per_lm_iteration_min_median_max": [round(float(per.min()), 1), round(float(np.median(per)), 1),
                                                                round(float(per.max()), 1)],
                          "cost_initial_final_median": [float(np.median(costs[:, 0])), float(np.median(costs[:, 1]))],
                          "max_position_error_m_before_after_median": [round(float(np.median(err0)), 4),
                                                                       round(float(np.median(err1)), 4)]}))


if __name__ == "__main__":
    main()
