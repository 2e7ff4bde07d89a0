// Batched pinhole reprojection residuals, SE(3) Jacobians and per-problem
// normal equations (§8 a11: the north star's "ceres reprojection cost"; the
// reference links Ceres but never calls it, SURVEY §0.2, so this is pinned by
// finite differences only). Feeds the host pose solver in refine.cpp.
//
// The observation model and the layout of the 28 sums are reproj_model.hpp's;
// this is its monocular evaluation, one thread per point.
// Reduction: per block in a fixed order (wave shuffles, then LDS), partial sums
// per (problem, block), then a second pass summing blocks in index order, so
// every run gives the same bits.
#include "common.hpp"
#include "reproj_model.hpp"

namespace svo {

namespace {

__global__ __launch_bounds__(256) void reproj_kernel(const double* __restrict__ obj, const float* __restrict__ img,
                                                     const int* __restrict__ counts, int cap,
                                                     const double* __restrict__ poses, double fx, double fy,
                                                     double cx, double cy, double delta, double* __restrict__ res,
                                                     double* __restrict__ jac, double* __restrict__ partial) {
    const int b = blockIdx.y;
    const int n = counts ? counts[b] : cap;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double* T = poses + 12 * (size_t)b;
    double e[kNE];
#pragma unroll
    for (int k = 0; k < kNE; k++) e[k] = 0;
    if (i < n) {
        const double* X = obj + 3 * ((size_t)b * cap + i);
        const float* u = img + 2 * ((size_t)b * cap + i);
        double r0 = 0, r1 = 0, r2, w, J[12];
#pragma unroll
        for (int k = 0; k < 12; k++) J[k] = 0;
        const Cam k{fx, fy, cx, cy, delta, 0};
        if (obs_eval<false>(k, T, X, u, nullptr, r0, r1, r2, w, e[27], J))
            normal_terms<false, false>(false, w, r0, r1, 0, J, e);
        if (res) {
            res[2 * ((size_t)b * cap + i)] = r0;
            res[2 * ((size_t)b * cap + i) + 1] = r1;
        }
        if (jac)
#pragma unroll
            for (int k = 0; k < 12; k++) jac[12 * ((size_t)b * cap + i) + k] = J[k];
    }
    if (!partial) return;
    __shared__ double S[4][kNE];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kNE; k++) {
        const double s = wave_sum(e[k]);
        if (lane == 0) S[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kNE) {
        const int k = threadIdx.x;
        partial[((size_t)b * gridDim.x + blockIdx.x) * kNE + k] = wave_fold(S, k);
    }
}

__global__ void reproj_reduce_kernel(const double* __restrict__ partial, int nblk, int nprob, double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nprob * kNE) return;
    const int b = t / kNE, k = t - b * kNE;
    double s = 0;
    for (int j = 0; j < nblk; j++) s += partial[((size_t)b * nblk + j) * kNE + k];
    out[t] = s;
}

}  // namespace

size_t reproj_partial_doubles(int n_problems, int max_n) {
    return (size_t)n_problems * ((max_n + 255) / 256) * kNE;
}

hipError_t launch_reproj(const double* d_obj, const float* d_img, const int* d_counts, int n_problems, int cap,
                         int max_n, const double* d_poses, const double K[9], double delta, double* d_res,
                         double* d_jac, double* d_partial, double* d_normal, hipStream_t st) {
    if (n_problems <= 0 || max_n <= 0) {
        if (d_normal && n_problems > 0)
            return hipMemsetAsync(d_normal, 0, sizeof(double) * kNE * (size_t)n_problems, st);
        return hipSuccess;
    }
    const int nblk = (max_n + 255) / 256;
    hipLaunchKernelGGL(reproj_kernel, dim3(nblk, n_problems), dim3(256), 0, st, d_obj, d_img, d_counts, cap, d_poses,
                       K[0], K[4], K[2], K[5], delta, d_res, d_jac, d_normal ? d_partial : nullptr);
    if (d_normal) {
        const int tot = n_problems * kNE;
        hipLaunchKernelGGL(reproj_reduce_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, d_partial, nblk,
                           n_problems, d_normal);
    }
    return hipGetLastError();
}

}  // namespace svo
