// Windowed bundle adjustment on the device (ba.hip): the staged problem batch
// and the launchers of one Levenberg-Marquardt iteration's stages. bundle.cpp
// stages the batch and runs the LM control.
#pragma once

#include "common.hpp"

namespace svo {

constexpr int kBaNE = 28;  // per camera: 21 U + 6 gc + 1 cost (reproj.hip's layout)

// P problems, strides max_cams / max_points / max_obs per problem. Observations
// are staged sorted by (point, camera): point i owns [pt_off[i], pt_off[i + 1])
// and camera j the sorted positions cam_idx[cam_off[j] .. cam_off[j + 1]), ascending.
struct BaBatch {
    int P, maxC, maxM, maxO;
    double fx, fy, cx, cy, delta;
    const int* n_cams;     // [P]
    const int* n_points;   // [P]
    const uint8_t* fixed;  // [P][maxC]
    const int* ocam;       // [P][maxO]
    const float* oxy;      // [P][maxO][2]
    const int* pt_off;     // [P][maxM + 1]
    const int* cam_off;    // [P][maxC + 1]
    const int* cam_idx;    // [P][maxO]
    const int* cam_pt;     // [P][maxO]: point of the observation cam_idx names
    // per-problem control, written by the host before each pass
    const double* lambda;  // [P]
    const int* active;     // [P]: 0 = every stage leaves the problem alone
    // linearisation
    double* cam_ne;   // [P][maxC][28]
    int* cam_cnt;     // [P][maxC]: observations in front of the camera
    double* pt_V;     // [P][maxM][6] upper triangle
    double* pt_g;     // [P][maxM][3]
    double* pt_Vinv;  // [P][maxM][6]: (V + lambda diag V)^-1
    int* pt_free;     // [P][maxM]: 0 = held constant this iteration
    // solve
    double* dc;        // [P][maxC][6], zero for cameras outside the reduced system
    int* status;       // [P]: 0 solved, 1 reduced system not positive definite
    int* n_free;       // [P]: cameras in the reduced system
    double* step_part; // [P][point blocks][2]: |dp|^2, |X|^2 of the free points
    double* stepinfo;  // [P][2]: |step|^2, |free state|^2
    double* cam_cost;  // [P][maxC]: cost-only pass
};

int ba_point_blocks(int max_points);
// stage 1: U, gc, cost and the in-front counts per camera; V, gp, V*^-1 per point
hipError_t launch_ba_linearize(const BaBatch& b, const double* poses, const double* points, hipStream_t st);
// stages 2 + 3: reduced system and its Cholesky solve, one workgroup per problem.
// S_out / b_out (nullable): [P][6 maxC][6 maxC] / [P][6 maxC], zeroed by the caller.
hipError_t launch_ba_schur_solve(const BaBatch& b, const double* poses, const double* points, double* S_out,
                                 double* b_out, hipStream_t st);
// stage 4: trial points and poses; dp_out nullable [P][maxM][3]
hipError_t launch_ba_update(const BaBatch& b, const double* poses, const double* points, double* trial_poses,
                            double* trial_points, double* dp_out, hipStream_t st);
// stage 5 (and the initial cost): cost[p] of a state, cameras summed in index order
hipError_t launch_ba_cost(const BaBatch& b, const double* poses, const double* points, double* cost, hipStream_t st);
// trial -> current for the problems with accept[p] != 0
hipError_t launch_ba_commit(const BaBatch& b, const int* accept, const double* trial_poses,
                            const double* trial_points, double* poses, double* points, hipStream_t st);

}  // namespace svo
