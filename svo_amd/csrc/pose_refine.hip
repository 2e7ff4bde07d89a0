// Motion-only stereo refinement (§8 a11d): the pose of one frame from its stereo
// observations, the points held constant -- svo_refine_poses' Levenberg-Marquardt
// with svo_bundle_adjust_stereo's observation model, run for one problem by one
// workgroup inside a single launch (no host step between iterations).
//
// The observation model (include/svo_gpu.h, svo_bundle_adjust_stereo), the 6x6
// solve, the pose update and the LM decisions are reproj_model.hpp's: with
// ur >= 0 its stereo evaluation, with ur < 0 (or no ur plane) the monocular one
// that reproj_kernel runs, term by term. All arithmetic is f64.
//
// The 28 sums (H upper triangle 21, g 6, cost 1), in one fixed order:
//   1. thread t adds its observations i = t, t + 256, ... in ascending i;
//   2. the 64 lanes of a wave are summed by the xor butterfly 32, 16, ..., 1;
//   3. the four waves are summed through LDS as ((w0 + w1) + w2) + w3.
// A thread's sum starts from its first observation's terms, an observation that
// contributes nothing adds +0 and a thread without observations holds +0: for
// n <= 256 these are reproj_kernel's bits. Nothing outside the problem enters
// the order (not the batch size, not cap, not the other problems).
//
// Control: every branch that leads to a barrier tests a kernel argument or a
// value read from LDS behind a barrier (made scalar with readfirstlane), so it
// is uniform over the workgroup; lane 0 solves the 6x6 system between two
// barriers, never inside one. Loops are bounded: the outer one by
// max_iterations <= SVO_REFINE_MAX_ITERATIONS, the lambda retry by kMaxRetry.
#include "pose_refine.hpp"

namespace svo {

namespace {

constexpr int kBlock = 256;
// lambda x10 from its floor 1e-12 passes 1e16 after 28 steps
constexpr int kMaxRetry = 32;

struct Shared {
    double T[12];    // the current pose
    double Tt[12];   // the trial pose
    double ne[kNE];  // the sums at T
    double nt[kNE];  // the sums at Tt
    double S[4][kNE];
    double lambda, c_first;
    int bad[4];
    int go, its, poisoned;
};

// one problem's slice of the batch
struct Problem {
    int n;
    const double* pts;  // obj + 3 first observation, or the problem's map
    const int* ids;     // nullable
    const float2* xy;
    const float* ur;    // nullable
    int map_cap;
};

// observation i's point, null for an id outside the map
__device__ __forceinline__ const double* point_of(const Problem& q, int i) {
    if (!q.ids) return q.pts + 3 * (size_t)i;
    const int m = q.ids[i];
    return (m >= 0 && m < q.map_cap) ? q.pts + 3 * (size_t)m : nullptr;
}

// The 28 sums of problem q at the pose Tsh (LDS) into out (LDS), visible to every
// thread on return. Every thread of the block calls it.
__device__ __forceinline__ void linearize(const PoseRefineBatch& B, const Problem& q, const double* Tsh,
                                          double (*S)[kNE], double* out) {
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = Tsh[k];
    const Cam cam{B.fx, B.fy, B.cx, B.cy, B.delta, B.baseline};
    double e[kNE];
    // -0 is the identity of +: the first observation's terms keep their bits
    const double first = (int)threadIdx.x < q.n ? -0.0 : 0.0;
#pragma unroll
    for (int k = 0; k < kNE; k++) e[k] = first;
    for (int i = threadIdx.x; i < q.n; i += kBlock) {
        const double* X = point_of(q, i);
        const float2 u = q.xy[i];
        const float ur = q.ur ? q.ur[i] : -1.f;
        double v[kNE], r0, r1, r2, w, J[18];
        const int kind = X ? obs_eval<true>(cam, T, X, &u.x, &ur, r0, r1, r2, w, v[27], J) : 0;
        if (!kind) {  // nothing to add, but +0 is added: a leading -0 becomes +0, as stated above
#pragma unroll
            for (int k = 0; k < kNE; k++) e[k] += 0.0;
            continue;
        }
        normal_terms<true, false>(kind == 2, w, r0, r1, r2, J, v);
#pragma unroll
        for (int k = 0; k < kNE; k++) e[k] += v[k];
    }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kNE; k++) {
        const double s = wave_sum(e[k]);
        if (lane == 0) S[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kNE) {
        const int k = threadIdx.x;
        out[k] = wave_fold(S, k);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void pose_refine_kernel(PoseRefineBatch B) {
    __shared__ Shared sh;
    const int p = blockIdx.x, t = threadIdx.x;
    // ---- the problem's slice (every value below is uniform over the block)
    Problem q;
    size_t pose_at = 12 * (size_t)p, obs_at = (size_t)p * B.cap;
    bool has_pose = true;
    if (B.sel_nc) {
        const int nc = min(max(B.sel_nc[p], 0), B.window);
        has_pose = nc > 0;
        const int v = p * B.window + max(nc - 1, 0);
        const int sl = min(max(B.sel_slot[v], 0), B.window - 1);
        q.n = has_pose ? min(max(B.sel_cnt[v], 0), B.cap) : 0;
        pose_at = 12 * ((size_t)p * B.window + sl);
        obs_at = ((size_t)p * B.window + sl) * B.cap;
    } else {
        q.n = B.counts ? min(max(B.counts[p], 0), B.cap) : B.cap;
    }
    q.ids = B.ids ? B.ids + obs_at : nullptr;
    q.pts = B.ids ? B.map + 3 * (size_t)p * B.map_cap : B.obj + 3 * obs_at;
    q.map_cap = B.map_cap;
    q.xy = reinterpret_cast<const float2*>(B.xy) + obs_at;
    q.ur = B.ur ? B.ur + obs_at : nullptr;

    // ---- the pose, and the scan for values that are not finite (a block-wide OR)
    bool bad = false;
    if (t < 12) {
        const double v = has_pose ? B.poses_in[pose_at + t] : ((t == 0 || t == 4 || t == 8) ? 1.0 : 0.0);
        sh.T[t] = v;
        bad = !isfinite(v);
    }
    for (int i = t; i < q.n; i += kBlock) {
        const double* X = point_of(q, i);
        if (X) bad = bad || !(isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]));
        const float2 u = q.xy[i];
        bad = bad || !(isfinite(u.x) && isfinite(u.y));
        if (q.ur) bad = bad || !isfinite(q.ur[i]);
    }
    const bool wave_bad = __any(bad);
    if ((t & 63) == 0) sh.bad[t >> 6] = wave_bad;
    __syncthreads();

    linearize(B, q, sh.T, sh.S, sh.ne);

    if (t == 0) {
        const double c = sh.ne[27];
        sh.poisoned = (sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3]) || !isfinite(c);
        sh.c_first = c;
        sh.lambda = kLmLambda0;
        sh.its = 0;
        sh.go = 0;
    }
    __syncthreads();
    const int poisoned = __builtin_amdgcn_readfirstlane(sh.poisoned);

    if (!poisoned) {
        for (int it = 0; it < B.max_iterations; it++) {
            if (t == 0) {
                // reproj_model.hpp's LM control: solve (lambda up while not positive
                // definite), the step rule, the trial pose
                double lambda = sh.lambda, dx[6];
                bool ok = false;
                for (int r = 0; r < kMaxRetry && !ok && lambda < kLmCeiling; r++) {
                    ok = lm_solve6(sh.ne, lambda, dx);
                    if (!ok) lambda *= kLmUp;
                }
                sh.lambda = lambda;
                sh.its = it + 1;
                int go = 0;
                if (ok) {
                    double nx = 0, nt = 0;
#pragma unroll
                    for (int k = 0; k < 6; k++) nx += dx[k] * dx[k];
#pragma unroll
                    for (int k = 9; k < 12; k++) nt += sh.T[k] * sh.T[k];
                    if (!lm_step_is_small(nx, nt)) {
                        se3_left_update(dx, sh.T, sh.Tt);
                        go = 1;
                    }
                }
                sh.go = go;
            }
            __syncthreads();
            if (!__builtin_amdgcn_readfirstlane(sh.go)) break;  // gave up, or the step rule
            linearize(B, q, sh.Tt, sh.S, sh.nt);
            // the verdict (every thread reads the same LDS words)
            double lambda = sh.lambda;
            const auto [accept, stop] = lm_verdict(sh.ne[27], sh.nt[27], lambda);
            __syncthreads();  // c0 and lambda are read before anyone overwrites them
            if (accept) {
                if (t < 12) sh.T[t] = sh.Tt[t];
                if (t >= 64 && t < 64 + kNE) sh.ne[t - 64] = sh.nt[t - 64];
            }
            if (t == 0) sh.lambda = lambda;
            __syncthreads();
            if (__builtin_amdgcn_readfirstlane((int)stop)) break;
        }
    }

    // ---- results
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (t < 12 && has_pose && !poisoned) B.poses_out[pose_at + t] = sh.T[t];
    if (t == 64) {
        B.costs[2 * (size_t)p] = poisoned ? nan : sh.c_first;
        B.costs[2 * (size_t)p + 1] = poisoned ? nan : sh.ne[27];
        B.iterations[p] = sh.its;
        if (B.n_used) B.n_used[p] = q.n;
    }
    if (B.normal && t >= 128 && t < 128 + kNE) B.normal[kNE * (size_t)p + t - 128] = poisoned ? nan : sh.ne[t - 128];
}

}  // namespace

hipError_t launch_pose_refine(const PoseRefineBatch& b, hipStream_t st) {
    if (b.P < 0 || b.cap < 0 || b.max_iterations < 0 || b.max_iterations > SVO_REFINE_MAX_ITERATIONS)
        return hipErrorInvalidValue;
    if (b.P == 0) return hipSuccess;
    if (!b.poses_in || !b.poses_out || !b.costs || !b.iterations) return hipErrorInvalidValue;
    if (b.cap > 0 && (!b.xy || (b.ids ? !b.map || b.map_cap < 0 : !b.obj))) return hipErrorInvalidValue;
    if (b.sel_nc && (!b.sel_slot || !b.sel_cnt || b.window < 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_refine_kernel, dim3(b.P), dim3(kBlock), 0, st, b);
    return hipGetLastError();
}

}  // namespace svo
