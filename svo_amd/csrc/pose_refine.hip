// Motion-only stereo refinement (§8 a11d): the pose of one frame from its stereo
// observations, the points held constant -- svo_refine_poses' Levenberg-Marquardt
// with svo_bundle_adjust_stereo's observation model, run for one problem by one
// workgroup inside a single launch (no host step between iterations).
//
// Per observation (include/svo_gpu.h, svo_bundle_adjust_stereo): P = R X + t,
// the two left rows are reproj_kernel's; with ur >= 0 a third residual
//   r2 = fx (Px - baseline) / Pz + cx - ur,  xr = (Px - baseline) / Pz,
//   J2 = [fx/Pz, 0, -fx xr/Pz, -fx xr y, fx (1 + xr x), -fx y];
// the Huber weight and the cost take the norm of the residual the observation
// has; Pz <= 0 contributes nothing; ur < 0 is reproj_kernel's evaluation, term
// by term. All arithmetic is f64.
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

constexpr int kNE = kPoseRefineNE;
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

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

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
    const double fx = B.fx, fy = B.fy, cx = B.cx, cy = B.cy, delta = B.delta, bl = B.baseline;
    double e[kNE];
    // -0 is the identity of +: the first observation's terms keep their bits
    const double first = (int)threadIdx.x < q.n ? -0.0 : 0.0;
#pragma unroll
    for (int k = 0; k < kNE; k++) e[k] = first;
    for (int i = threadIdx.x; i < q.n; i += kBlock) {
        double v[kNE];
#pragma unroll
        for (int k = 0; k < kNE; k++) v[k] = 0;
        const double* X = point_of(q, i);
        if (X) {
            const double px = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[9];
            const double py = T[3] * X[0] + T[4] * X[1] + T[5] * X[2] + T[10];
            const double pz = T[6] * X[0] + T[7] * X[1] + T[8] * X[2] + T[11];
            if (pz > 0) {
                const float2 u = q.xy[i];
                const float urv = q.ur ? q.ur[i] : -1.f;
                const bool st = urv >= 0.f;
                const double iz = 1.0 / pz, x = px * iz, y = py * iz;
                const double r0 = fx * x + cx - (double)u.x;
                const double r1 = fy * y + cy - (double)u.y;
                double J[18];
                J[0] = fx * iz;
                J[1] = 0;
                J[2] = -fx * x * iz;
                J[3] = -fx * x * y;
                J[4] = fx * (1 + x * x);
                J[5] = -fx * y;
                J[6] = 0;
                J[7] = fy * iz;
                J[8] = -fy * y * iz;
                J[9] = -fy * (1 + y * y);
                J[10] = fy * x * y;
                J[11] = fy * x;
                const double xr = (px - bl) * iz;
                const double r2 = fx * xr + cx - (double)urv;
                J[12] = fx * iz;
                J[13] = 0;
                J[14] = -fx * xr * iz;
                J[15] = -fx * xr * y;
                J[16] = fx * (1 + xr * x);
                J[17] = -fx * y;
                const double n2m = r0 * r0 + r1 * r1;
                const double n2 = st ? n2m + r2 * r2 : n2m;
                const double nr = sqrt(n2);
                const bool robust = delta > 0 && nr > delta;
                const double w = robust ? delta / nr : 1.0;
                int k = 0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int c = a; c < 6; c++) {
                        const double m = J[a] * J[c] + J[6 + a] * J[6 + c];
                        v[k++] = w * (st ? m + J[12 + a] * J[12 + c] : m);
                    }
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    const double m = J[a] * r0 + J[6 + a] * r1;
                    v[21 + a] = w * (st ? m + J[12 + a] * r2 : m);
                }
                v[27] = robust ? delta * (nr - 0.5 * delta) : 0.5 * n2;
            }
        }
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
        out[k] = ((S[0][k] + S[1][k]) + S[2][k]) + S[3][k];
    }
    __syncthreads();
}

// refine.cpp's lm_solve: (H + lambda diag(H)) x = -g by Cholesky; false if not
// positive definite. Fully unrolled: A, L, y stay in registers.
__device__ __forceinline__ bool lm_solve(const double* ne, double lambda, double x[6]) {
    double A[36], b[6];
    {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = a; c < 6; c++) {
                A[6 * a + c] = A[6 * c + a] = ne[k];
                k++;
            }
    }
#pragma unroll
    for (int a = 0; a < 6; a++) {
        A[7 * a] += lambda * (A[7 * a] > 0 ? A[7 * a] : 1e-12);
        b[a] = -ne[21 + a];
    }
    double L[36];
#pragma unroll
    for (int k = 0; k < 36; k++) L[k] = 0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = A[6 * i + j];
#pragma unroll
            for (int q = 0; q < j; q++) s -= L[6 * i + q] * L[6 * j + q];
            if (i == j) {
                ok = ok && s > 0;
                L[7 * i] = sqrt(ok ? s : 1.0);
            } else {
                L[6 * i + j] = s / L[7 * j];
            }
        }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int q = 0; q < i; q++) s -= L[6 * i + q] * y[q];
        y[i] = s / L[7 * i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int q = i + 1; q < 6; q++) s -= L[6 * q + i] * x[q];
        x[i] = s / L[7 * i];
    }
    return ok;
}

// refine.cpp's se3_left_update: Tn = exp(xi^) T, xi = (rho, phi)
__device__ __forceinline__ void se3_left_update(const double xi[6], const double* T, double* Tn) {
    const double* rho = xi;
    const double* ph = xi + 3;
    const double th2 = ph[0] * ph[0] + ph[1] * ph[1] + ph[2] * ph[2];
    const double th = sqrt(th2);
    double A, Bc, C;  // sin/th, (1-cos)/th^2, (th-sin)/th^3
    if (th < 1e-8) {
        A = 1 - th2 / 6;
        Bc = 0.5 - th2 / 24;
        C = 1.0 / 6 - th2 / 120;
    } else {
        A = sin(th) / th;
        Bc = (1 - cos(th)) / th2;
        C = (th - sin(th)) / (th2 * th);
    }
    const double W[9] = {0, -ph[2], ph[1], ph[2], 0, -ph[0], -ph[1], ph[0], 0};
    double W2[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
    double R[9], V[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double I = (k % 4 == 0);
        R[k] = I + A * W[k] + Bc * W2[k];
        V[k] = I + Bc * W[k] + C * W2[k];
    }
    const double tx[3] = {V[0] * rho[0] + V[1] * rho[1] + V[2] * rho[2], V[3] * rho[0] + V[4] * rho[1] + V[5] * rho[2],
                          V[6] * rho[0] + V[7] * rho[1] + V[8] * rho[2]};
    double Ti[12];
#pragma unroll
    for (int k = 0; k < 12; k++) Ti[k] = T[k];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++)
            Tn[3 * i + j] = R[3 * i] * Ti[j] + R[3 * i + 1] * Ti[3 + j] + R[3 * i + 2] * Ti[6 + j];
        Tn[9 + i] = R[3 * i] * Ti[9] + R[3 * i + 1] * Ti[10] + R[3 * i + 2] * Ti[11] + tx[i];
    }
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
        sh.lambda = 1e-4;
        sh.its = 0;
        sh.go = 0;
    }
    __syncthreads();
    const int poisoned = __builtin_amdgcn_readfirstlane(sh.poisoned);

    if (!poisoned) {
        for (int it = 0; it < B.max_iterations; it++) {
            if (t == 0) {
                // refine.cpp:195-212: solve (lambda x10 while not positive definite),
                // the step rule, the trial pose
                double lambda = sh.lambda, dx[6];
                bool ok = false;
                for (int r = 0; r < kMaxRetry && !ok && lambda < 1e16; r++) {
                    ok = lm_solve(sh.ne, lambda, dx);
                    if (!ok) lambda *= 10;
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
                    if (!(sqrt(nx) < 1e-12 * (1 + sqrt(nt)))) {
                        se3_left_update(dx, sh.T, sh.Tt);
                        go = 1;
                    }
                }
                sh.go = go;
            }
            __syncthreads();
            if (!__builtin_amdgcn_readfirstlane(sh.go)) break;  // gave up, or the step rule
            linearize(B, q, sh.Tt, sh.S, sh.nt);
            // refine.cpp:219-228: the verdict (every thread reads the same LDS words)
            const double c0 = sh.ne[27], c1 = sh.nt[27];
            const bool accept = c1 <= c0;
            double lambda = sh.lambda;
            bool stop;
            if (accept) {
                lambda = lambda * 0.1 > 1e-12 ? lambda * 0.1 : 1e-12;
                stop = c0 - c1 <= 1e-15 * c0;
            } else {
                lambda *= 10;
                stop = lambda >= 1e16;
            }
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
