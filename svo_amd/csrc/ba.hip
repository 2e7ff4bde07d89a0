// Windowed bundle adjustment: poses and points together.
// A problem has C <= SVO_BA_MAX_CAMS cameras (world -> camera, 12 doubles,
// reproj_model.hpp's conventions), M points and O monocular observations (camera,
// point, u, v). Per observation the residual, Huber weight, cost, Pz <= 0 rule
// and pose Jacobian Jc (2x6, left perturbation) are reproj_model.hpp's obs_eval;
// the point Jacobian is Jp = Jc[:, :3] R (2x3). One Levenberg-Marquardt iteration:
//   1 linearise   U_j = sum w Jc^T Jc, gc_j, cost (per camera); V_i = sum w Jp^T Jp,
//                 gp_i (per point); W_ij = w Jc^T Jp is recomputed where it is used
//   2 eliminate   V*_i = V_i + lambda diag V_i inverted in closed form,
//                 S = U* - sum_i W_ij V*_i^-1 W_ik^T, b = -gc + sum_i W_ij V*_i^-1 gp_i
//   3 solve       S dc = b by Cholesky, packed lower triangle in LDS
//   4 update      dp_i = V*_i^-1 (-gp_i - sum_j W_ij^T dc_j); trial points and poses
//   5 cost        of the trial state (stage 1's camera pass, cost only)
// Every sum has a fixed order (a thread's own items in index order, wave
// shuffles, LDS, then partials in index order) and nothing is accumulated with
// atomics, so two runs give the same bits. A camera may observe a point more than
// once: the observations are summed (one W_ij) and count as one camera. Points
// seen by fewer than two cameras in front of them, and points whose damped block
// is not positive definite, are held constant; a free camera with no observation
// in front of it is treated as fixed.
// Stereo (kStereo, the batch's `our` plane; DESIGN.md section 10, "Stereo observations"): an
// observation whose right column ur is >= 0 has a third residual row, on the
// rectified right camera at +baseline on the left camera's x axis, added behind
// the two left rows in every sum; it weighs and costs by its 3-norm and counts
// as two views of its point. An observation with ur < 0 has no third row in the
// camera sums and a zero one in the point sums, and so the monocular bits (every
// sum here starts at +0 and adds, so a -0 term and a +0 term are the same).
#include "ba.hpp"

namespace svo {

namespace {

constexpr int kMaxCams = SVO_BA_MAX_CAMS;
constexpr int kMaxN = 6 * kMaxCams;               // reduced system order
constexpr int kMaxNS = kMaxN * (kMaxN + 1) / 2;   // packed lower triangle
constexpr int kSolveThreads = 512;
constexpr int kEPT = (kMaxNS + kSolveThreads - 1) / kSolveThreads;  // S entries per thread
constexpr int kPT = 4;                            // points staged per pass of the elimination
constexpr int kWStride = kMaxCams * 18;           // doubles of W (or Y) per staged point

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// obs_eval for the point side: a monocular observation's r2 and third row are
// zeroed, so point_jacobian and rows_dot may read them
template <bool kStereo>
__device__ __forceinline__ int obs_eval_rows(const Cam& k, const double* __restrict__ T, const double* __restrict__ X,
                                             const float* __restrict__ u, const float* __restrict__ ur, double& r0,
                                             double& r1, double& r2, double& w, double& cost,
                                             double J[6 * kRows<kStereo>]) {
    const int kind = obs_eval<kStereo>(k, T, X, u, ur, r0, r1, r2, w, cost, J);
    if constexpr (kStereo)
        if (kind == 1) {
            r2 = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) J[12 + a] = 0;
        }
    return kind;
}

// Jp = Jc[:, :3] R (row a of Jp at Jp[3 a])
template <bool kStereo>
__device__ __forceinline__ void point_jacobian(const double J[6 * kRows<kStereo>], const double* __restrict__ T,
                                               double Jp[3 * kRows<kStereo>]) {
#pragma unroll
    for (int a = 0; a < kRows<kStereo>; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) Jp[3 * a + c] = J[6 * a] * T[c] + J[6 * a + 1] * T[3 + c] + J[6 * a + 2] * T[6 + c];
}

// w (a0 b0 + a1 b1), and behind them the stereo row's a2 b2 (never read in the
// monocular instantiation, where the row does not exist)
template <bool kStereo>
__device__ __forceinline__ double rows_dot(double w, double a0, double b0, double a1, double b1, const double* a2,
                                           const double* b2) {
    if constexpr (kStereo)
        return w * ((a0 * b0 + a1 * b1) + *a2 * *b2);
    else
        return w * (a0 * b0 + a1 * b1);
}

// ------------------------------------------------------------------ stage 1 / 5: per camera
// One block per (camera, problem); thread t takes the camera's observations
// t, t + 256, ... in order. kFull: U, gc, cost and the in-front count; else the
// cost alone.
template <bool kFull, bool kStereo>
__global__ __launch_bounds__(256) void ba_camera_kernel(BaBatch d, const double* __restrict__ poses,
                                                        const double* __restrict__ points) {
    constexpr int kN = kFull ? kNE : 1;
    const int p = blockIdx.y, j = blockIdx.x;
    if (!d.active[p] || j >= d.n_cams[p]) return;
    const Cam k{d.fx, d.fy, d.cx, d.cy, d.delta, d.baseline};
    const double* T = poses + 12 * ((size_t)p * d.maxC + j);
    const size_t ob = (size_t)p * d.maxO;
    const int o0 = d.cam_off[(size_t)p * (d.maxC + 1) + j], o1 = d.cam_off[(size_t)p * (d.maxC + 1) + j + 1];
    double e[kN];
#pragma unroll
    for (int q = 0; q < kN; q++) e[q] = 0;
    int cnt = 0;
    for (int a = o0 + (int)threadIdx.x; a < o1; a += 256) {
        const int o = d.cam_idx[ob + a];
        const double* X = points + 3 * ((size_t)p * d.maxM + d.cam_pt[ob + a]);
        double r0, r1, r2, w, c, J[6 * kRows<kStereo>];
        const float* ur = kStereo ? d.our + (ob + o) : nullptr;
        const int kind = obs_eval<kStereo>(k, T, X, d.oxy + 2 * (ob + o), ur, r0, r1, r2, w, c, J);
        if (!kind) continue;
        cnt++;
        if constexpr (kFull) normal_terms<kStereo, true>(kind == 2, w, r0, r1, r2, J, e);
        e[kN - 1] += c;
    }
    __shared__ double S[4][kN];
    __shared__ int Sc[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < kN; q++) {
        const double s = wave_sum(e[q]);
        if (lane == 0) S[wv][q] = s;
    }
    const int cs = wave_sum_int(cnt);
    if (lane == 0) Sc[wv] = cs;
    __syncthreads();
    const size_t cj = (size_t)p * d.maxC + j;
    if ((int)threadIdx.x < kN) {
        const int q = threadIdx.x;
        const double s = wave_fold(S, q);
        if (kFull)
            d.cam_ne[cj * kNE + q] = s;
        else
            d.cam_cost[cj] = s;
    }
    if (kFull && threadIdx.x == 0) d.cam_cnt[cj] = Sc[0] + Sc[1] + Sc[2] + Sc[3];
}

// cost[p] = sum over the cameras, in index order, of src[(p maxC + j) stride + off]
__global__ void ba_cost_sum_kernel(BaBatch d, const double* __restrict__ src, int stride, int off,
                                   double* __restrict__ cost) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= d.P || !d.active[p]) return;
    double s = 0;
    for (int j = 0; j < d.n_cams[p]; j++) s += src[((size_t)p * d.maxC + j) * stride + off];
    cost[p] = s;
}

// ------------------------------------------------------------------ stage 1 / 2: per point
// One thread per point: V, gp over its observations in camera order, then the
// damped block's inverse by cofactors.
template <bool kStereo>
__global__ __launch_bounds__(256) void ba_point_kernel(BaBatch d, const double* __restrict__ poses,
                                                       const double* __restrict__ points) {
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (!d.active[p] || i >= d.n_points[p]) return;
    const Cam k{d.fx, d.fy, d.cx, d.cy, d.delta, d.baseline};
    const size_t ob = (size_t)p * d.maxO, pi = (size_t)p * d.maxM + i;
    const double* X = points + 3 * pi;
    const int o0 = d.pt_off[(size_t)p * (d.maxM + 1) + i], o1 = d.pt_off[(size_t)p * (d.maxM + 1) + i + 1];
    double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    int nfront = 0, prev = -1;  // distinct cameras in front: a camera's observations are consecutive
    bool two = false;           // the current camera's run already counts its stereo view
    for (int a = o0; a < o1; a++) {
        const int cam = d.ocam[ob + a];
        const double* T = poses + 12 * ((size_t)p * d.maxC + cam);
        double r0, r1, r2, w, c, J[6 * kRows<kStereo>], Jp[3 * kRows<kStereo>];
        const int kind = obs_eval_rows<kStereo>(k, T, X, d.oxy + 2 * (ob + a), kStereo ? d.our + (ob + a) : nullptr, r0,
                                                r1, r2, w, c, J);
        if (!kind) continue;
        nfront += cam != prev;
        if constexpr (kStereo) {
            two = two && cam == prev;
            nfront += kind == 2 && !two;
            two = two || kind == 2;
        }
        prev = cam;
        point_jacobian<kStereo>(J, T, Jp);
        int q = 0;
#pragma unroll
        for (int s = 0; s < 3; s++)
#pragma unroll
            for (int t = s; t < 3; t++)
                V[q++] += rows_dot<kStereo>(w, Jp[s], Jp[t], Jp[3 + s], Jp[3 + t], Jp + 6 + s, Jp + 6 + t);
#pragma unroll
        for (int s = 0; s < 3; s++) g[s] += rows_dot<kStereo>(w, Jp[s], r0, Jp[3 + s], r1, Jp + 6 + s, &r2);
    }
#pragma unroll
    for (int q = 0; q < 6; q++) d.pt_V[6 * pi + q] = V[q];
#pragma unroll
    for (int q = 0; q < 3; q++) d.pt_g[3 * pi + q] = g[q];
    const double lam = d.lambda[p];
    const double a = V[0] + lam * V[0], b = V[1], c = V[2], dd = V[3] + lam * V[3], e = V[4], f = V[5] + lam * V[5];
    const double c00 = dd * f - e * e, c01 = c * e - b * f, c02 = b * e - c * dd;
    const double c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * dd - b * b;
    const double det = (a * c00 + b * c01) + c * c02;
    const bool ok = nfront >= 2 && a > 0 && c22 > 0 && det > 0;
    const double id = ok ? 1.0 / det : 0.0;
    d.pt_Vinv[6 * pi + 0] = c00 * id;
    d.pt_Vinv[6 * pi + 1] = c01 * id;
    d.pt_Vinv[6 * pi + 2] = c02 * id;
    d.pt_Vinv[6 * pi + 3] = c11 * id;
    d.pt_Vinv[6 * pi + 4] = c12 * id;
    d.pt_Vinv[6 * pi + 5] = c22 * id;
    d.pt_free[pi] = ok ? 1 : 0;
}

// W_ij = sum over point i's observations by camera `cam` of w Jc^T Jp (6x3, row-major)
template <bool kStereo>
__device__ __forceinline__ void accumulate_W(const Cam& k, const double* __restrict__ T, const double* __restrict__ X,
                                             const float* __restrict__ u, const float* __restrict__ ur, double W[18]) {
    double r0, r1, r2, w, c, J[6 * kRows<kStereo>], Jp[3 * kRows<kStereo>];
    if (!obs_eval_rows<kStereo>(k, T, X, u, ur, r0, r1, r2, w, c, J)) return;
    point_jacobian<kStereo>(J, T, Jp);
#pragma unroll
    for (int x = 0; x < 6; x++)
#pragma unroll
        for (int t = 0; t < 3; t++)
            W[3 * x + t] += rows_dot<kStereo>(w, J[x], Jp[t], J[6 + x], Jp[3 + t], J + 12 + x, Jp + 6 + t);
}

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

// ------------------------------------------------------------------ stages 2 + 3
// One workgroup per problem. Thread t owns the packed entries t, t + 512, ... of
// S in registers while the points stream through LDS kPT at a time: one lane per
// observation of those points stages W_ij and Y_ij = W_ij V*_i^-1 (zero where the
// camera does not see the point or the point is constant), then every thread
// subtracts Y_ij W_ik^T from its entries, points in index order. The assembled
// system is factored and solved in LDS.
template <bool kStereo>
__global__ __launch_bounds__(kSolveThreads) void ba_schur_solve_kernel(BaBatch d, const double* __restrict__ poses,
                                                                       const double* __restrict__ points,
                                                                       double* __restrict__ S_out,
                                                                       double* __restrict__ b_out) {
    const int p = blockIdx.x, t = threadIdx.x;
    if (!d.active[p]) return;
    __shared__ double Sl[kMaxNS];
    __shared__ double Wl[kPT * kWStride], Yl[kPT * kWStride];
    __shared__ double gpl[kPT * 3];
    __shared__ double bl[kMaxN];
    __shared__ int freecam[kMaxCams], camslot[kMaxCams];  // free index -> camera and back (-1: not free)
    __shared__ int soff[kPT + 1], slive[kPT];
    __shared__ int s_nfree;
    const Cam k{d.fx, d.fy, d.cx, d.cy, d.delta, d.baseline};
    const int C = d.n_cams[p], M = d.n_points[p];
    const size_t cb = (size_t)p * d.maxC, ob = (size_t)p * d.maxO, pb = (size_t)p * d.maxM;
    if (t == 0) {
        int nf = 0;
        for (int j = 0; j < kMaxCams; j++) camslot[j] = -1;
        for (int j = 0; j < C; j++)
            if (!d.fixed[cb + j] && d.cam_cnt[cb + j] > 0) {
                camslot[j] = nf;
                freecam[nf++] = j;
            }
        s_nfree = nf;
        d.n_free[p] = nf;
        d.status[p] = 0;
    }
    for (int q = t; q < 6 * d.maxC; q += kSolveThreads) d.dc[6 * cb + q] = 0;
    __syncthreads();
    const int nf = s_nfree, n = 6 * nf, NS = n * (n + 1) / 2;
    if (n == 0) return;
    const double lam = d.lambda[p];

    // this thread's entries: LDS offsets of the Y row and the W row, and U* as the start
    int offY[kEPT], offW[kEPT];
    double acc[kEPT];
#pragma unroll
    for (int q = 0; q < kEPT; q++) {
        const int e = t + q * kSolveThreads;
        offY[q] = offW[q] = 0;
        acc[q] = 0;
        if (e < NS) {
            int r = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
            while (tri(r, 0) > e) r--;
            while (tri(r + 1, 0) <= e) r++;
            const int c = e - tri(r, 0);
            const int jr = r / 6, x = r - 6 * jr, jc = c / 6, y = c - 6 * jc;
            offY[q] = jr * 18 + x * 3;
            offW[q] = jc * 18 + y * 3;
            if (jr == jc) {  // y <= x: entry (y, x) of the upper triangle of U
                const double u = d.cam_ne[(cb + freecam[jr]) * kNE + (y * 6 - y * (y - 1) / 2 + (x - y))];
                acc[q] = r == c ? u + lam * u : u;
            }
        }
    }
    double accb = 0;
    const int offB = t < n ? (t / 6) * 18 + (t % 6) * 3 : 0;

    for (int base = 0; base < M; base += kPT) {
        // clear the staging area; the first kPT + 1 lanes fetch the points' runs, flags and gp
        for (int z = t; z < kPT * kWStride; z += kSolveThreads) Wl[z] = Yl[z] = 0;
        if (t <= kPT) {
            const int i = base + t < M ? base + t : M;
            soff[t] = d.pt_off[(size_t)p * (d.maxM + 1) + i];
            if (t < kPT) {
                const bool live = base + t < M && d.pt_free[pb + i] != 0;
                slive[t] = live;
#pragma unroll
                for (int z = 0; z < 3; z++) gpl[3 * t + z] = live ? d.pt_g[3 * (pb + i) + z] : 0.0;
            }
        }
        __syncthreads();
        // one lane per staged observation of these points (their runs are contiguous);
        // the first observation of a (point, camera) run sums the run and owns the slot
        for (int a = soff[0] + t; a < soff[kPT]; a += kSolveThreads) {
            int q = 0;
#pragma unroll
            for (int z = 1; z < kPT; z++) q += a >= soff[z];
            const int cam = d.ocam[ob + a], jf = camslot[cam];
            if (jf < 0 || !slive[q] || (a > soff[q] && d.ocam[ob + a - 1] == cam)) continue;
            const int i = base + q;
            const double* T = poses + 12 * (cb + cam);
            const double* X = points + 3 * (pb + i);
            double W[18];
#pragma unroll
            for (int z = 0; z < 18; z++) W[z] = 0;
            for (int a2 = a; a2 < soff[q + 1] && d.ocam[ob + a2] == cam; a2++)
                accumulate_W<kStereo>(k, T, X, d.oxy + 2 * (ob + a2), kStereo ? d.our + (ob + a2) : nullptr, W);
            const double* Vi = d.pt_Vinv + 6 * (pb + i);
            const double v00 = Vi[0], v01 = Vi[1], v02 = Vi[2], v11 = Vi[3], v12 = Vi[4], v22 = Vi[5];
            double* Wo = Wl + q * kWStride + jf * 18;
            double* Yo = Yl + q * kWStride + jf * 18;
#pragma unroll
            for (int x = 0; x < 6; x++) {
                Wo[3 * x] = W[3 * x];
                Wo[3 * x + 1] = W[3 * x + 1];
                Wo[3 * x + 2] = W[3 * x + 2];
                Yo[3 * x + 0] = (W[3 * x] * v00 + W[3 * x + 1] * v01) + W[3 * x + 2] * v02;
                Yo[3 * x + 1] = (W[3 * x] * v01 + W[3 * x + 1] * v11) + W[3 * x + 2] * v12;
                Yo[3 * x + 2] = (W[3 * x] * v02 + W[3 * x + 1] * v12) + W[3 * x + 2] * v22;
            }
        }
        __syncthreads();
        // one staged point at a time: unrolled over the points as well, the
        // compiler hoists every LDS read of the pass and spills
#pragma unroll 1
        for (int s = 0; s < kPT; s++)
#pragma unroll
            for (int q = 0; q < kEPT; q++) {
                const double* Yr = Yl + s * kWStride + offY[q];
                const double* Wr = Wl + s * kWStride + offW[q];
                acc[q] -= Yr[0] * Wr[0];
                acc[q] -= Yr[1] * Wr[1];
                acc[q] -= Yr[2] * Wr[2];
            }
        if (t < n)
#pragma unroll
            for (int s = 0; s < kPT; s++) {
                const double* Yr = Yl + s * kWStride + offB;
                accb += Yr[0] * gpl[3 * s];
                accb += Yr[1] * gpl[3 * s + 1];
                accb += Yr[2] * gpl[3 * s + 2];
            }
        __syncthreads();
    }

#pragma unroll
    for (int q = 0; q < kEPT; q++) {
        const int e = t + q * kSolveThreads;
        if (e < NS) Sl[e] = acc[q];
    }
    if (t < n) bl[t] = accb - d.cam_ne[(cb + freecam[t / 6]) * kNE + 21 + t % 6];
    __syncthreads();
    if (S_out) {
        const int ld = 6 * d.maxC;
        double* So = S_out + (size_t)p * ld * ld;
        for (int q = t; q < n * n; q += kSolveThreads) {
            const int r = q / n, c = q - r * n;
            So[(size_t)r * ld + c] = r >= c ? Sl[tri(r, c)] : Sl[tri(c, r)];
        }
    }
    if (b_out && t < n) b_out[(size_t)p * 6 * d.maxC + t] = bl[t];
    __syncthreads();

    // Cholesky S = L L^T, column by column: thread i owns row i
    bool bad = false;
    for (int j = 0; j < n; j++) {
        double s = 0;
        if (t >= j && t < n) {
            s = Sl[tri(t, j)];
            for (int q = 0; q < j; q++) s -= Sl[tri(t, q)] * Sl[tri(j, q)];
            Sl[tri(t, j)] = s;
        }
        __syncthreads();
        const double dj = Sl[tri(j, j)];
        __syncthreads();
        if (!(dj > 0)) {
            bad = true;
            break;
        }
        if (t >= j && t < n) Sl[tri(t, j)] = t == j ? sqrt(dj) : s / sqrt(dj);
        __syncthreads();
    }
    if (bad) {
        if (t == 0) d.status[p] = 1;
        return;
    }
    for (int j = 0; j < n; j++) {  // L y = b
        if (t == j) bl[j] = bl[j] / Sl[tri(j, j)];
        __syncthreads();
        if (t > j && t < n) bl[t] -= Sl[tri(t, j)] * bl[j];
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; j--) {  // L^T x = y
        if (t == j) bl[j] = bl[j] / Sl[tri(j, j)];
        __syncthreads();
        if (t < j) bl[t] -= Sl[tri(j, t)] * bl[j];
        __syncthreads();
    }
    if (t < n) d.dc[6 * (cb + freecam[t / 6]) + t % 6] = bl[t];
}

// ------------------------------------------------------------------ stage 4: points
template <bool kStereo>
__global__ __launch_bounds__(256) void ba_point_update_kernel(BaBatch d, const double* __restrict__ poses,
                                                              const double* __restrict__ points,
                                                              double* __restrict__ trial_points,
                                                              double* __restrict__ dp_out) {
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (!d.active[p]) return;
    const Cam k{d.fx, d.fy, d.cx, d.cy, d.delta, d.baseline};
    const size_t cb = (size_t)p * d.maxC, ob = (size_t)p * d.maxO, pi = (size_t)p * d.maxM + i;
    double sd = 0, sx = 0;
    if (i < d.n_points[p]) {
        const double X[3] = {points[3 * pi], points[3 * pi + 1], points[3 * pi + 2]};
        double dp[3] = {0, 0, 0};
        const bool moves = d.status[p] == 0 && d.pt_free[pi] != 0;
        if (moves) {
            double a3[3] = {-d.pt_g[3 * pi], -d.pt_g[3 * pi + 1], -d.pt_g[3 * pi + 2]};
            const int o0 = d.pt_off[(size_t)p * (d.maxM + 1) + i], o1 = d.pt_off[(size_t)p * (d.maxM + 1) + i + 1];
            for (int a = o0; a < o1; a++) {
                const int cam = d.ocam[ob + a];
                if (d.fixed[cb + cam]) continue;
                double W[18];
#pragma unroll
                for (int z = 0; z < 18; z++) W[z] = 0;
                accumulate_W<kStereo>(k, poses + 12 * (cb + cam), X, d.oxy + 2 * (ob + a),
                                      kStereo ? d.our + (ob + a) : nullptr, W);
                const double* dc = d.dc + 6 * (cb + cam);
#pragma unroll
                for (int s = 0; s < 3; s++)
#pragma unroll
                    for (int x = 0; x < 6; x++) a3[s] -= W[3 * x + s] * dc[x];
            }
            const double* Vi = d.pt_Vinv + 6 * pi;
            dp[0] = (Vi[0] * a3[0] + Vi[1] * a3[1]) + Vi[2] * a3[2];
            dp[1] = (Vi[1] * a3[0] + Vi[3] * a3[1]) + Vi[4] * a3[2];
            dp[2] = (Vi[2] * a3[0] + Vi[4] * a3[1]) + Vi[5] * a3[2];
            sd = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2];
            sx = (X[0] * X[0] + X[1] * X[1]) + X[2] * X[2];
        }
#pragma unroll
        for (int s = 0; s < 3; s++) {
            trial_points[3 * pi + s] = moves ? X[s] + dp[s] : X[s];
            if (dp_out) dp_out[3 * pi + s] = dp[s];
        }
    }
    __shared__ double S[4][2];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    sd = wave_sum(sd);
    sx = wave_sum(sx);
    if (lane == 0) {
        S[wv][0] = sd;
        S[wv][1] = sx;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        d.step_part[((size_t)p * gridDim.x + blockIdx.x) * 2 + q] = wave_fold(S, q);
    }
}

// ------------------------------------------------------------------ stage 4: poses, step size
// One wave per problem: lane j moves camera j; lane 0 then sums the step and
// state norms, cameras and point blocks in index order.
__global__ __launch_bounds__(64) void ba_pose_update_kernel(BaBatch d, const double* __restrict__ poses,
                                                            double* __restrict__ trial_poses, int nblk) {
    const int p = blockIdx.x, j = threadIdx.x;
    if (!d.active[p]) return;
    const size_t cb = (size_t)p * d.maxC;
    const int C = d.n_cams[p];
    __shared__ double nrm[kMaxCams][2];
    if (j < kMaxCams) nrm[j][0] = nrm[j][1] = 0;
    if (j < C) {
        const double* T = poses + 12 * (cb + j);
        double* out = trial_poses + 12 * (cb + j);
        const bool moves = d.status[p] == 0 && !d.fixed[cb + j] && d.cam_cnt[cb + j] > 0;
        if (moves) {
            double xi[6];
#pragma unroll
            for (int q = 0; q < 6; q++) xi[q] = d.dc[6 * (cb + j) + q];
            se3_left_update(xi, T, out);
            double s = 0;
#pragma unroll
            for (int q = 0; q < 6; q++) s += xi[q] * xi[q];
            nrm[j][0] = s;
            nrm[j][1] = (T[9] * T[9] + T[10] * T[10]) + T[11] * T[11];
        } else {
#pragma unroll
            for (int q = 0; q < 12; q++) out[q] = T[q];
        }
    }
    __syncthreads();
    if (j == 0) {
        double s0 = 0, s1 = 0;
        for (int q = 0; q < C; q++) {
            s0 += nrm[q][0];
            s1 += nrm[q][1];
        }
        for (int q = 0; q < nblk; q++) {
            s0 += d.step_part[((size_t)p * nblk + q) * 2];
            s1 += d.step_part[((size_t)p * nblk + q) * 2 + 1];
        }
        d.stepinfo[2 * p] = s0;
        d.stepinfo[2 * p + 1] = s1;
    }
}

__global__ __launch_bounds__(256) void ba_commit_kernel(BaBatch d, const int* __restrict__ accept,
                                                        const double* __restrict__ trial_poses,
                                                        const double* __restrict__ trial_points,
                                                        double* __restrict__ poses, double* __restrict__ points) {
    const int p = blockIdx.y;
    if (!accept[p]) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int nc = 12 * d.n_cams[p], np = 3 * d.n_points[p];
    if (q < nc) poses[12 * (size_t)p * d.maxC + q] = trial_poses[12 * (size_t)p * d.maxC + q];
    if (q < np) points[3 * (size_t)p * d.maxM + q] = trial_points[3 * (size_t)p * d.maxM + q];
}

}  // namespace

int ba_point_blocks(int max_points) { return max_points > 0 ? (max_points + 255) / 256 : 1; }

hipError_t launch_ba_linearize(const BaBatch& b, const double* poses, const double* points, hipStream_t st) {
    if (b.P <= 0) return hipSuccess;
    if (b.maxC > 0) {
        if (b.our)
            hipLaunchKernelGGL((ba_camera_kernel<true, true>), dim3(b.maxC, b.P), dim3(256), 0, st, b, poses, points);
        else
            hipLaunchKernelGGL((ba_camera_kernel<true, false>), dim3(b.maxC, b.P), dim3(256), 0, st, b, poses, points);
    }
    if (b.maxM > 0) {
        const dim3 grid((b.maxM + 255) / 256, b.P);
        if (b.our)
            hipLaunchKernelGGL(ba_point_kernel<true>, grid, dim3(256), 0, st, b, poses, points);
        else
            hipLaunchKernelGGL(ba_point_kernel<false>, grid, dim3(256), 0, st, b, poses, points);
    }
    return hipGetLastError();
}

hipError_t launch_ba_schur_solve(const BaBatch& b, const double* poses, const double* points, double* S_out,
                                 double* b_out, hipStream_t st) {
    if (b.P <= 0) return hipSuccess;
    if (b.our)
        hipLaunchKernelGGL(ba_schur_solve_kernel<true>, dim3(b.P), dim3(kSolveThreads), 0, st, b, poses, points, S_out,
                           b_out);
    else
        hipLaunchKernelGGL(ba_schur_solve_kernel<false>, dim3(b.P), dim3(kSolveThreads), 0, st, b, poses, points, S_out,
                           b_out);
    return hipGetLastError();
}

hipError_t launch_ba_update(const BaBatch& b, const double* poses, const double* points, double* trial_poses,
                            double* trial_points, double* dp_out, hipStream_t st) {
    if (b.P <= 0) return hipSuccess;
    const int nblk = ba_point_blocks(b.maxM);
    if (b.our)
        hipLaunchKernelGGL(ba_point_update_kernel<true>, dim3(nblk, b.P), dim3(256), 0, st, b, poses, points,
                           trial_points, dp_out);
    else
        hipLaunchKernelGGL(ba_point_update_kernel<false>, dim3(nblk, b.P), dim3(256), 0, st, b, poses, points,
                           trial_points, dp_out);
    hipLaunchKernelGGL(ba_pose_update_kernel, dim3(b.P), dim3(64), 0, st, b, poses, trial_poses, nblk);
    return hipGetLastError();
}

hipError_t launch_ba_cost(const BaBatch& b, const double* poses, const double* points, double* cost, hipStream_t st) {
    if (b.P <= 0) return hipSuccess;
    if (b.maxC > 0) {
        if (b.our)
            hipLaunchKernelGGL((ba_camera_kernel<false, true>), dim3(b.maxC, b.P), dim3(256), 0, st, b, poses, points);
        else
            hipLaunchKernelGGL((ba_camera_kernel<false, false>), dim3(b.maxC, b.P), dim3(256), 0, st, b, poses, points);
    }
    hipLaunchKernelGGL(ba_cost_sum_kernel, dim3((b.P + 255) / 256), dim3(256), 0, st, b, b.cam_cost, 1, 0, cost);
    return hipGetLastError();
}

hipError_t launch_ba_commit(const BaBatch& b, const int* accept, const double* trial_poses,
                            const double* trial_points, double* poses, double* points, hipStream_t st) {
    if (b.P <= 0) return hipSuccess;
    const int most = 12 * b.maxC > 3 * b.maxM ? 12 * b.maxC : 3 * b.maxM;
    if (most <= 0) return hipSuccess;
    hipLaunchKernelGGL(ba_commit_kernel, dim3((most + 255) / 256, b.P), dim3(256), 0, st, b, accept, trial_poses,
                       trial_points, poses, points);
    return hipGetLastError();
}

}  // namespace svo
