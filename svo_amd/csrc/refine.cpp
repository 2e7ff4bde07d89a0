// Reprojection cost C ABI (§8 a11) and the host pose solver it feeds:
// Levenberg-Marquardt over SE(3) (motion-only bundle adjustment, what a Ceres
// problem with one pose block and AutoDiff reprojection residuals would solve;
// the reference never builds one). Every iteration is one batched
// GPU evaluation (reproj.hip) of residuals, J^T J, J^T r and cost for all
// problems; the 6x6 solves, the pose updates and the LM decisions run on the
// host, all three from reproj_model.hpp.
#include <cstring>
#include <vector>

#include "common.hpp"
#include "reproj_model.hpp"

using namespace svo;

namespace {

struct Staged {
    double *obj, *poses, *res, *jac, *partial, *normal;
    float* img;
    int* counts;
};

int stage(svo_ctx* ctx, const double* obj, const float* img, const int* counts, int P, int max_n, bool want_res,
          bool want_jac, Staged& s) {
    const size_t np = (size_t)P * max_n;
    if (!carve_scratch(ctx, kScratchSolve, [&](Carver& c) {
            s.obj = c.take<double>(3 * np);
            s.poses = c.take<double>(12 * (size_t)P);
            s.res = want_res ? c.take<double>(2 * np) : nullptr;
            s.jac = want_jac ? c.take<double>(12 * np) : nullptr;
            s.partial = c.take<double>(reproj_partial_doubles(P, max_n));
            s.normal = c.take<double>(kNE * (size_t)P);
            s.img = c.take<float>(2 * np);
            s.counts = counts ? c.take<int>(P) : nullptr;
        }))
        return set_error(ctx, SVO_ERR_HIP, "scratch alloc");
    SVO_HIP(ctx, hipMemcpyAsync(s.obj, obj, sizeof(double) * 3 * np, hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(ctx, hipMemcpyAsync(s.img, img, sizeof(float) * 2 * np, hipMemcpyHostToDevice, ctx->stream));
    if (counts) SVO_HIP(ctx, hipMemcpyAsync(s.counts, counts, sizeof(int) * P, hipMemcpyHostToDevice, ctx->stream));
    return SVO_OK;
}

bool bad_args(const double* obj, const float* img, const int* counts, int P, int max_n, const double* K) {
    if (P < 0 || max_n < 0 || !K) return true;
    if (P > 0 && max_n > 0 && (!obj || !img)) return true;
    if (counts)
        for (int b = 0; b < P; b++)
            if (counts[b] < 0 || counts[b] > max_n) return true;
    return false;
}

}  // namespace

extern "C" {

int svo_reprojection_jacobians(svo_ctx* ctx, const double* obj_xyz, const float* img_xy, const int* counts,
                               int n_problems, int max_n, const double* poses, const double K[9],
                               double huber_delta, double* res, double* jac, double* normal) {
    if (!ctx || bad_args(obj_xyz, img_xy, counts, n_problems, max_n, K) || (n_problems > 0 && !poses))
        return set_error(ctx, SVO_ERR_ARG, "svo_reprojection_jacobians: bad arguments");
    if (n_problems == 0) return SVO_OK;
    Staged s;
    int rc = stage(ctx, obj_xyz, img_xy, counts, n_problems, max_n, res != nullptr, jac != nullptr, s);
    if (rc) return rc;
    SVO_HIP(ctx, hipMemcpyAsync(s.poses, poses, sizeof(double) * 12 * n_problems, hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(ctx, launch_reproj(s.obj, s.img, s.counts, n_problems, max_n, max_n, s.poses, K, huber_delta, s.res, s.jac,
                               s.partial, normal ? s.normal : nullptr, ctx->stream));
    const size_t np = (size_t)n_problems * max_n;
    if (res) SVO_HIP(ctx, hipMemcpyAsync(res, s.res, sizeof(double) * 2 * np, hipMemcpyDeviceToHost, ctx->stream));
    if (jac) SVO_HIP(ctx, hipMemcpyAsync(jac, s.jac, sizeof(double) * 12 * np, hipMemcpyDeviceToHost, ctx->stream));
    if (normal)
        SVO_HIP(ctx, hipMemcpyAsync(normal, s.normal, sizeof(double) * kNE * n_problems, hipMemcpyDeviceToHost,
                                    ctx->stream));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

int svo_refine_poses(svo_ctx* ctx, const double* obj_xyz, const float* img_xy, const int* counts, int n_problems,
                     int max_n, const double K[9], double huber_delta, int max_iterations, double* poses,
                     double* costs, int* iterations) {
    if (!ctx || bad_args(obj_xyz, img_xy, counts, n_problems, max_n, K) || (n_problems > 0 && !poses) ||
        max_iterations < 0)
        return set_error(ctx, SVO_ERR_ARG, "svo_refine_poses: bad arguments");
    if (iterations) *iterations = 0;
    if (n_problems == 0) return SVO_OK;
    const int P = n_problems;
    Staged s;
    int rc = stage(ctx, obj_xyz, img_xy, counts, P, max_n, false, false, s);
    if (rc) return rc;
    std::vector<double> cur(poses, poses + 12 * (size_t)P), trial(cur), ne(kNE * (size_t)P), ne_t(ne);
    std::vector<double> lambda((size_t)P, kLmLambda0);
    std::vector<char> done((size_t)P, 0);
    auto evaluate = [&](const std::vector<double>& T, std::vector<double>& out) -> int {
        SVO_HIP(ctx, hipMemcpyAsync(s.poses, T.data(), sizeof(double) * 12 * P, hipMemcpyHostToDevice, ctx->stream));
        SVO_HIP(ctx, launch_reproj(s.obj, s.img, s.counts, P, max_n, max_n, s.poses, K, huber_delta, nullptr, nullptr,
                                   s.partial, s.normal, ctx->stream));
        SVO_HIP(ctx, hipMemcpyAsync(out.data(), s.normal, sizeof(double) * kNE * P, hipMemcpyDeviceToHost, ctx->stream));
        SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return SVO_OK;
    };
    if ((rc = evaluate(cur, ne))) return rc;
    int it = 0;
    for (; it < max_iterations; it++) {
        bool any = false;
        for (int b = 0; b < P; b++) {
            std::memcpy(&trial[12 * (size_t)b], &cur[12 * (size_t)b], sizeof(double) * 12);
            if (done[b]) continue;
            double dx[6];
            bool ok = false;
            while (!ok && lambda[b] < kLmCeiling) {
                ok = lm_solve6(&ne[kNE * (size_t)b], lambda[b], dx);
                if (!ok) lambda[b] *= kLmUp;
            }
            if (!ok) {
                done[b] = 1;
                continue;
            }
            double nx = 0, nt = 0;
            for (int k = 0; k < 6; k++) nx += dx[k] * dx[k];
            for (int k = 9; k < 12; k++) nt += cur[12 * (size_t)b + k] * cur[12 * (size_t)b + k];
            if (lm_step_is_small(nx, nt)) {
                done[b] = 1;
                continue;
            }
            se3_left_update(dx, &trial[12 * (size_t)b], &trial[12 * (size_t)b]);
            any = true;
        }
        if (!any) break;
        if ((rc = evaluate(trial, ne_t))) return rc;
        for (int b = 0; b < P; b++) {
            if (done[b]) continue;
            const double c0 = ne[kNE * (size_t)b + 27], c1 = ne_t[kNE * (size_t)b + 27];
            const LmVerdict v = lm_verdict(c0, c1, lambda[b]);
            if (v.accept) {
                std::memcpy(&cur[12 * (size_t)b], &trial[12 * (size_t)b], sizeof(double) * 12);
                std::memcpy(&ne[kNE * (size_t)b], &ne_t[kNE * (size_t)b], sizeof(double) * kNE);
            }
            done[b] = v.stop;
        }
    }
    std::memcpy(poses, cur.data(), sizeof(double) * 12 * P);
    if (costs)
        for (int b = 0; b < P; b++) costs[b] = ne[kNE * (size_t)b + 27];
    if (iterations) *iterations = it;
    return SVO_OK;
}

}  // extern "C"
