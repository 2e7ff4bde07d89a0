// Motion-only stereo refinement on the device (pose_refine.hip): one workgroup
// runs the whole Levenberg-Marquardt of one problem in one launch.
#pragma once

#include "common.hpp"
#include "reproj_model.hpp"

namespace svo {

// Problem p reads its pose from poses_in and writes it to poses_out (the two may
// be one array). Dense form (sel_nc null): pose p at 12 p, observations
// [p*cap, p*cap + n_p), n_p = counts ? counts[p] : cap. Ring form (sel_nc set,
// the front end's window: launch_window_select's outputs): the problem is the
// newest valid slot sl of sequence p -- pose at 12 (p*window + sl), observations
// [(p*window + sl)*cap, + sel_cnt of that slot); no valid slot: the empty
// problem, no pose read or written. Points: obj (one per observation) or, with
// ids set, map[p*map_cap + ids[k]] read in place (an id outside [0, map_cap)
// contributes nothing). ur null: every observation monocular.
struct PoseRefineBatch {
    int P = 0, cap = 0;
    const double* poses_in = nullptr;
    double* poses_out = nullptr;
    const int* counts = nullptr;
    const int *sel_slot = nullptr, *sel_cnt = nullptr, *sel_nc = nullptr;
    int window = 0;
    const double* obj = nullptr;
    const double* map = nullptr;
    int map_cap = 0;
    const int* ids = nullptr;
    const float* xy = nullptr;
    const float* ur = nullptr;
    double fx = 0, fy = 0, cx = 0, cy = 0, baseline = 0, delta = 0;
    int max_iterations = 0;
    double* costs = nullptr;    // [P][2], required
    int* iterations = nullptr;  // [P], required
    int* n_used = nullptr;      // [P], nullable: the observations of each problem
    double* normal = nullptr;   // [P][28], nullable
};
// hipErrorInvalidValue (nothing launched): max_iterations outside 0 ..
// SVO_REFINE_MAX_ITERATIONS, sizes < 0, a required pointer null.
hipError_t launch_pose_refine(const PoseRefineBatch& b, hipStream_t st);

}  // namespace svo
