// Motion-only stereo refinement, the C ABI around pose_refine.hip (§8 a11d):
// svo_refine_poses_stereo (one upload, one launch, one download) and its timing
// probe. The front end's entry, svo_frontend_refine_poses, is in frontend_api.cpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "pose_refine.hpp"

using namespace svo;

namespace {

const char* bad_args(const double* obj, const float* xy, const float* ur, const int* counts, int P, int max_n,
                     const double* K, double baseline, int max_iterations, const double* poses) {
    if (P < 0 || max_n < 0 || !K) return "sizes < 0 or K null";
    if (P > 0 && !poses) return "poses null";
    if (P > 0 && max_n > 0 && (!obj || !xy)) return "obj_xyz / img_xy null";
    if (P > 0 && max_n > 0 && !ur) return "img_ur null";
    if (!(std::isfinite(baseline) && baseline > 0)) return "baseline not finite or <= 0";
    if (max_iterations < 0 || max_iterations > SVO_REFINE_MAX_ITERATIONS)
        return "max_iterations outside 0 .. SVO_REFINE_MAX_ITERATIONS";
    if (counts)
        for (int b = 0; b < P; b++)
            if (counts[b] < 0 || counts[b] > max_n) return "a count outside 0 .. max_n";
    return nullptr;
}

// the inputs on the device (context stream) and the launch's arguments
int stage(svo_ctx* ctx, const double* obj, const float* xy, const float* ur, const int* counts, int P, int max_n,
          const double K[9], double baseline, double huber_delta, int max_iterations, const double* poses,
          bool separate_out, PoseRefineBatch& b) {
    const size_t np = (size_t)P * max_n;
    b = PoseRefineBatch{};
    double *d_obj, *d_poses;  // (the batch's inputs are const)
    float *d_xy, *d_ur;
    int* d_counts;
    if (!carve_scratch(ctx, kScratchRefine, [&](Carver& c) {
            b.obj = d_obj = c.take<double>(3 * np);
            b.poses_in = d_poses = c.take<double>(12 * (size_t)P);
            b.poses_out = separate_out ? c.take<double>(12 * (size_t)P) : d_poses;
            b.costs = c.take<double>(2 * (size_t)P);
            b.normal = c.take<double>(kNE * (size_t)P);
            b.xy = d_xy = c.take<float>(2 * np);
            b.ur = d_ur = c.take<float>(np);
            b.counts = d_counts = counts ? c.take<int>(P) : nullptr;
            b.iterations = c.take<int>(P);
        }))
        return set_error(ctx, SVO_ERR_HIP, "scratch alloc");
    hipStream_t st = ctx->stream;
    if (np) {
        SVO_HIP(ctx, hipMemcpyAsync(d_obj, obj, sizeof(double) * 3 * np, hipMemcpyHostToDevice, st));
        SVO_HIP(ctx, hipMemcpyAsync(d_xy, xy, sizeof(float) * 2 * np, hipMemcpyHostToDevice, st));
        SVO_HIP(ctx, hipMemcpyAsync(d_ur, ur, sizeof(float) * np, hipMemcpyHostToDevice, st));
    }
    if (counts) SVO_HIP(ctx, hipMemcpyAsync(d_counts, counts, sizeof(int) * P, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(d_poses, poses, sizeof(double) * 12 * P, hipMemcpyHostToDevice, st));
    b.P = P;
    b.cap = max_n;
    b.fx = K[0], b.fy = K[4], b.cx = K[2], b.cy = K[5];
    b.baseline = baseline;
    b.delta = huber_delta;
    b.max_iterations = max_iterations;
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_refine_poses_stereo(svo_ctx* ctx, const double* obj_xyz, const float* img_xy, const float* img_ur,
                            const int* counts, int n_problems, int max_n, const double K[9], double baseline,
                            double huber_delta, int max_iterations, double* poses, double* costs, int* iterations,
                            double* normal) {
    if (!ctx) return SVO_ERR_ARG;
    if (const char* why = bad_args(obj_xyz, img_xy, img_ur, counts, n_problems, max_n, K, baseline, max_iterations,
                                   poses))
        return set_error(ctx, SVO_ERR_ARG, "svo_refine_poses_stereo: %s", why);
    if (n_problems == 0) return SVO_OK;
    const size_t P = (size_t)n_problems;
    PoseRefineBatch b;
    int rc = stage(ctx, obj_xyz, img_xy, img_ur, counts, n_problems, max_n, K, baseline, huber_delta, max_iterations,
                   poses, false, b);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    SVO_HIP(ctx, launch_pose_refine(b, st));
    // one block: poses_out (= poses), costs and normal are carved side by side,
    // each downloaded where the caller wants it
    SVO_HIP(ctx, hipMemcpyAsync(poses, b.poses_out, sizeof(double) * 12 * P, hipMemcpyDeviceToHost, st));
    if (costs) SVO_HIP(ctx, hipMemcpyAsync(costs, b.costs, sizeof(double) * 2 * P, hipMemcpyDeviceToHost, st));
    if (iterations) SVO_HIP(ctx, hipMemcpyAsync(iterations, b.iterations, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    if (normal) SVO_HIP(ctx, hipMemcpyAsync(normal, b.normal, sizeof(double) * kNE * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    return SVO_OK;
}

int svo_refine_poses_time(svo_ctx* ctx, const double* obj_xyz, const float* img_xy, const float* img_ur,
                          const int* counts, int n_problems, int max_n, const double K[9], double baseline,
                          double huber_delta, int max_iterations, const double* poses, int reps, double* ms_device,
                          double* ms_host) {
    if (!ctx) return SVO_ERR_ARG;
    if (const char* why = bad_args(obj_xyz, img_xy, img_ur, counts, n_problems, max_n, K, baseline, max_iterations,
                                   poses))
        return set_error(ctx, SVO_ERR_ARG, "svo_refine_poses_time: %s", why);
    if (n_problems <= 0 || max_n <= 0 || reps <= 0 || !ms_device || !ms_host)
        return set_error(ctx, SVO_ERR_ARG, "svo_refine_poses_time: bad arguments");
    PoseRefineBatch b;
    // every launch starts from the staged poses: the results go to a block of their own
    int rc = stage(ctx, obj_xyz, img_xy, img_ur, counts, n_problems, max_n, K, baseline, huber_delta, max_iterations,
                   poses, true, b);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    hipEvent_t e0, e1;
    SVO_HIP(ctx, hipEventCreate(&e0));
    SVO_HIP(ctx, hipEventCreate(&e1));
    hipError_t e = launch_pose_refine(b, st);  // untimed first
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int i = 0; i < reps && e == hipSuccess; i++) e = launch_pose_refine(b, st);
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    SVO_HIP(ctx, e);
    *ms_device = ms / reps;
    // the host loop on the same left pixels from the same poses, the same iterations cap
    std::vector<double> T((size_t)12 * n_problems);
    double wall = 0;
    for (int i = 0; i <= reps; i++) {  // (the first run is the warm-up)
        std::copy(poses, poses + T.size(), T.begin());
        const auto t0 = std::chrono::steady_clock::now();
        rc = svo_refine_poses(ctx, obj_xyz, img_xy, counts, n_problems, max_n, K, huber_delta, max_iterations,
                              T.data(), nullptr, nullptr);
        if (rc) return rc;
        if (i) wall += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    *ms_host = wall / reps;
    return SVO_OK;
}

}  // extern "C"
