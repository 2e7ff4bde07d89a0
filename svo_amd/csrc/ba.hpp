// Windowed bundle adjustment on the device (ba.hip): the staged problem batch
// and the launchers of one Levenberg-Marquardt iteration's stages. bundle.cpp
// stages the batch and runs the LM control.
#pragma once

#include "common.hpp"
#include "reproj_model.hpp"  // per camera, kNE sums: 21 U + 6 gc + 1 cost

namespace svo {

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
    // stereo (nullable: null runs the monocular kernels)
    const float* our;  // [P][maxO]: the right image's column, < 0 = monocular observation
    double baseline;   // > 0: the right camera's centre on the left camera's x axis
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

// ---- device staging (ba_stage.hip): a problem's observations arrive as W lists
// on the device, one per camera, each with strictly increasing point ids (the
// front end's feature lists), so the (point, camera) order
// above is a merge of W sorted lists and every staged position follows from
// binary searches alone: no sort, no atomics, a fixed order.
// Camera j of problem p reads list l = slot ? slot[p W + j] : j of the
// problem's W lists: counts[p W + j] entries of ids / xy at (p W + l) cap.
struct BaLists {
    int P, W, cap;
    const int* slot;    // [P][W], nullable
    const int* counts;  // [P][W], by camera
    const int* ids;     // [P][W][cap], by list
    const float* xy;    // [P][W][cap][2], by list
    const float* ur = nullptr;  // [P][W][cap], by list: the right column (< 0: none); nullable
};
// the chain's own memory, sized for W cap observations per problem (12 bytes each)
struct BaStageWork {
    int* pos;       // [P][W cap]: staged position | first-of-its-point << 31, by (camera, k)
    int* part;      // [P][ba_stage_blocks]: first observations per placing workgroup
    int* flag;      // [P][W cap]: by staged position, first-of-its-point, then the point index
    int* smid;      // [P][W cap]: by staged position, the point's id
    int* n_points;  // [P]
    int* n_obs;     // [P]
};
// the BA's arrays the chain fills, strides maxM / maxO / W (BaBatch's layout);
// points, map, n_cams_out are nullable (map: [P][map_cap][3], gathered by id)
struct BaStageOut {
    int maxM, maxO;
    int *ocam, *pt_off, *cam_off, *cam_idx, *cam_pt, *pt_id, *n_points;
    float* oxy;
    double* points;
    const double* map;
    int map_cap;
    float* our = nullptr;  // written where the lists carry ur and this is not null
};
int ba_stage_blocks(int W, int cap);
// the layout of that memory (layout.hpp): w's arrays from c
void ba_stage_layout(Carver& c, int P, int W, int cap, BaStageWork& w);
// pass 1: every observation's staged position and the counts n_points / n_obs
hipError_t launch_ba_stage_place(const BaLists& l, const BaStageWork& w, hipStream_t st);
// pass 2: the observations into (point, camera) order, the index lists per point
// and per camera, the compact points and their ids
hipError_t launch_ba_stage_fill(const BaLists& l, const BaStageWork& w, const BaStageOut& o, hipStream_t st);
// The cameras of a window: poses[p][j] = ring[(p W + slot[p W + j]) 12 ..] for j <
// n_cams[p] (zero behind), fixed[p][j] = j < n_fixed or j >= n_cams[p].
hipError_t launch_ba_stage_cams(const BaLists& l, const int* n_cams, const double* ring, int n_fixed, double* poses,
                                uint8_t* fixed, hipStream_t st);
// Back from the BA: points[p][i] to map[p][pt_id[i]] for i < n_points[p], the free
// cameras' poses to their ring slots.
hipError_t launch_ba_stage_unstage(const BaLists& l, const int* n_cams, const int* n_points, const int* pt_id,
                                   int maxM, const double* points, const double* poses, const uint8_t* fixed,
                                   double* map, int map_cap, double* ring, hipStream_t st);

// A windowed bundle adjustment whose problems lie on the device (bundle.cpp):
// stage from the lists, run svo_bundle_adjust's LM, write points and poses back.
// Host <-> device traffic: the staged counts once, the LM's control numbers per
// iteration. costs [P][2], iterations [P], sizes [P][3] (cameras, points,
// observations): nullable, host.
struct BaDeviceWindow {
    BaLists lists;
    const int* n_cams;  // [P] device: valid cameras (the first of each problem's W)
    double* ring;       // poses by list: [(p W + l) 12], world -> camera
    double* map;        // [P][map_cap][3]
    int map_cap;
    int n_fixed;
    double baseline = 0;  // > 0 with lists.ur: the stereo term
};
int ba_adjust_device(svo_ctx* ctx, const BaDeviceWindow& w, const double K[9], double huber_delta,
                     int max_iterations, double* costs, int* iterations, int* sizes);

}  // namespace svo
