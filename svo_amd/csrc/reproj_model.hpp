// The reprojection model and the Levenberg-Marquardt rules of the pose solvers,
// each stated once and compiled into both sides: reproj.hip, pose_refine.hip and
// ba.hip on the device, refine.cpp and bundle.cpp on the host. No HIP include:
// tools/reproj_model_check.cpp builds this header alone with the host compiler.
// sqrt / sin / cos are the unqualified <cmath> names, so the host resolves libm
// and the device its own library; the two differ in the last bits, as they did.
//
// The 28 sums of one pose over its observations (kNE):
//   H = sum w J^T J, upper triangle row-major (21), g = sum w J^T r (6), cost (1).
// Per observation: pose T = [R|t] (world -> camera, 12 doubles, R row-major),
// point X, pixel u (float xy), K (fx, fy, cx, cy):
//   P = R X + t,  r = (fx Px/Pz + cx - u, fy Py/Pz + cy - v)
//   J = dr/dxi for the left perturbation T <- exp(xi^) T, xi = (rho, phi):
//       dP/dxi = [I | -[P]x]
// and with a right column ur >= 0 (the rectified right camera at +baseline on the
// left camera's x axis) a third row
//   r2 = fx xr + cx - ur,  xr = (Px - baseline) / Pz,
//   J2 = [fx/Pz, 0, -fx xr/Pz, -fx xr y, fx (1 + xr x), -fx y].
// Robust weight (Huber, delta > 0): w = 1 if |r| <= delta else delta/|r|;
// cost = rho(|r|) (rho = |r|^2/2 or Huber), |r| over the rows the observation
// has. A point with Pz <= 0 adds nothing.
#pragma once

#include <cmath>

#ifdef __HIPCC__
#define SVO_MODEL_HD __host__ __device__ __forceinline__
#else
#define SVO_MODEL_HD inline
#endif

namespace svo {

constexpr int kNE = 28;  // 21 H + 6 g + 1 cost

struct Cam {
    double fx, fy, cx, cy, delta, bl;
};

template <bool kStereo>
constexpr int kRows = kStereo ? 3 : 2;

// One observation: 0 (nothing written) when the point is not in front of the
// camera, else 1, or 2 for a stereo observation (*ur >= 0; ur is read only by
// the stereo instantiation). kStereo: r2 and row 2 of J are the right column's,
// computed for a monocular observation too but meaningless there -- normal_terms
// leaves them out by the kind; the weight and the cost take the norm of the rows
// the observation has.
template <bool kStereo>
SVO_MODEL_HD int obs_eval(const Cam& k, const double* T, const double* X, const float* u, const float* ur, double& r0,
                          double& r1, double& r2, double& w, double& cost, double J[6 * kRows<kStereo>]) {
    const double px = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[9];
    const double py = T[3] * X[0] + T[4] * X[1] + T[5] * X[2] + T[10];
    const double pz = T[6] * X[0] + T[7] * X[1] + T[8] * X[2] + T[11];
    if (!(pz > 0)) return 0;
    const double iz = 1.0 / pz, x = px * iz, y = py * iz;
    r0 = k.fx * x + k.cx - (double)u[0];
    r1 = k.fy * y + k.cy - (double)u[1];
    J[0] = k.fx * iz;
    J[1] = 0;
    J[2] = -k.fx * x * iz;
    J[3] = -k.fx * x * y;
    J[4] = k.fx * (1 + x * x);
    J[5] = -k.fx * y;
    J[6] = 0;
    J[7] = k.fy * iz;
    J[8] = -k.fy * y * iz;
    J[9] = -k.fy * (1 + y * y);
    J[10] = k.fy * x * y;
    J[11] = k.fy * x;
    const double n2m = r0 * r0 + r1 * r1;
    double n2 = n2m;
    bool st = false;
    if constexpr (kStereo) {
        const float urv = *ur;
        st = urv >= 0.f;
        const double xr = (px - k.bl) * iz;
        r2 = k.fx * xr + k.cx - (double)urv;
        J[12] = k.fx * iz;
        J[13] = 0;
        J[14] = -k.fx * xr * iz;
        J[15] = -k.fx * xr * y;
        J[16] = k.fx * (1 + xr * x);
        J[17] = -k.fx * y;
        n2 = st ? n2m + r2 * r2 : n2m;
    }
    const double nr = sqrt(n2);
    const bool robust = k.delta > 0 && nr > k.delta;
    w = robust ? k.delta / nr : 1.0;
    cost = robust ? k.delta * (nr - 0.5 * k.delta) : 0.5 * n2;
    return st ? 2 : 1;
}

// The observation's 21 + 6 terms of H and g into e: w (J0 J0' + J1 J1'), and for
// a stereo observation (st) the third row's product behind them; assigned, or
// with kAdd added. A monocular observation's term is selected, not summed with a
// zero product: where it is -0 (a point on x = 0 or y = 0) it stays -0, which an
// assignment, and a sum that starts from -0, can see.
template <bool kStereo, bool kAdd>
SVO_MODEL_HD void normal_terms(bool st, double w, double r0, double r1, double r2, const double J[6 * kRows<kStereo>],
                               double e[27]) {
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = a; c < 6; c++) {
            const double m = J[a] * J[c] + J[6 + a] * J[6 + c];
            double t = w * m;
            if constexpr (kStereo) t = w * (st ? m + J[12 + a] * J[12 + c] : m);
            e[k] = kAdd ? e[k] + t : t;
            k++;
        }
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const double m = J[a] * r0 + J[6 + a] * r1;
        double t = w * m;
        if constexpr (kStereo) t = w * (st ? m + J[12 + a] * r2 : m);
        e[21 + a] = kAdd ? e[21 + a] + t : t;
    }
}

// out = exp(xi^) T, xi = (rho, phi); the series below |phi| = 1e-8. out may be T.
SVO_MODEL_HD void se3_left_update(const double xi[6], const double* T, double* out) {
    const double* rho = xi;
    const double* ph = xi + 3;
    const double th2 = ph[0] * ph[0] + ph[1] * ph[1] + ph[2] * ph[2];
    const double th = sqrt(th2);
    double A, B, C;  // sin/th, (1-cos)/th^2, (th-sin)/th^3
    if (th < 1e-8) {
        A = 1 - th2 / 6;
        B = 0.5 - th2 / 24;
        C = 1.0 / 6 - th2 / 120;
    } else {
        A = sin(th) / th;
        B = (1 - cos(th)) / th2;
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
        R[k] = I + A * W[k] + B * W2[k];
        V[k] = I + B * W[k] + C * W2[k];
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
            out[3 * i + j] = R[3 * i] * Ti[j] + R[3 * i + 1] * Ti[3 + j] + R[3 * i + 2] * Ti[6 + j];
        out[9 + i] = R[3 * i] * Ti[9] + R[3 * i + 1] * Ti[10] + R[3 * i + 2] * Ti[11] + tx[i];
    }
}

// (H + lambda diag(H)) x = -g by Cholesky over the 28 sums ne; a diagonal entry
// that is not positive is damped by lambda 1e-12. False if the damped matrix is
// not positive definite, and x is then unspecified. No branch on the data, and
// fully unrolled: on the device A, L, y stay in registers.
SVO_MODEL_HD bool lm_solve6(const double* ne, double lambda, double x[6]) {
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

// The LM control (include/svo_gpu.h, svo_refine_poses). A solver starts at
// kLmLambda0 and, while lm_solve6 (or the reduced system) is not positive
// definite and lambda < kLmCeiling, multiplies lambda by kLmUp and solves again;
// it stops without a trial when that gives up or the step is small.
constexpr double kLmLambda0 = 1e-4, kLmUp = 10, kLmDown = 0.1, kLmFloor = 1e-12, kLmCeiling = 1e16;
constexpr double kLmStepTol = 1e-12, kLmCostTol = 1e-15;

// |dx| < 1e-12 (1 + |t|), from the squared norms of the step and of the state
SVO_MODEL_HD bool lm_step_is_small(double dx2, double t2) { return sqrt(dx2) < kLmStepTol * (1 + sqrt(t2)); }

struct LmVerdict {
    bool accept, stop;
};
// The trial's cost c1 against the current c0. Accepted on c1 <= c0: lambda falls
// to max(0.1 lambda, 1e-12), and the solver stops once the cost no longer falls
// by more than 1e-15 of itself. Rejected (a NaN c1 is): lambda x10, and the
// solver stops at 1e16.
SVO_MODEL_HD LmVerdict lm_verdict(double c0, double c1, double& lambda) {
    LmVerdict v;
    v.accept = c1 <= c0;
    if (v.accept) {
        lambda = lambda * kLmDown > kLmFloor ? lambda * kLmDown : kLmFloor;
        v.stop = c0 - c1 <= kLmCostTol * c0;
    } else {
        lambda *= kLmUp;
        v.stop = lambda >= kLmCeiling;
    }
    return v;
}

#ifdef __HIPCC__
// ---- the block reduction of the sums, in one fixed order: a thread's own terms,
// the 64 lanes of a wave by the xor butterfly 32, 16, ..., 1, then the four
// waves through LDS as ((w0 + w1) + w2) + w3.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// entry k of the four waves' sums S[wave][k]
template <int kN>
__device__ __forceinline__ double wave_fold(const double (*S)[kN], int k) {
    return ((S[0][k] + S[1][k]) + S[2][k]) + S[3][k];
}
#endif

}  // namespace svo
