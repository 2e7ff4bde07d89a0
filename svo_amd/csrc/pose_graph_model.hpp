// The pose-graph edge and its normal-equation terms, stated once and compiled
// into both sides: pose_graph.hip on the device, pose_graph_api.cpp and
// tools/pose_graph_model_check.cpp on the host. It includes reproj_model.hpp (the
// LM rules, se3_left_update) and trig_pa.hpp (acos / sin / cos in plain arithmetic:
// the one HIP include), so an edge's terms are the same bits on host and device.
//
// Nodes: T = [R|t], world -> camera, 12 doubles, R row-major.
// Edge (i, j, Z, Omega): Z ~ T_j T_i^-1 (12 doubles), Omega a symmetric 6x6
// information matrix as its 21 upper-triangle entries row-major, order (rho, phi):
// the first 21 entries of svo_refine_poses_stereo's normal.
//   A = T_j T_i^-1,  E = A Z^-1 = [R_e | t_e],  e = (t_e, log R_e)
//   log R = f(th) v,  v = 1/2 vee(R - R'),  th = acos(clamp((tr R - 1)/2, -1, 1)),
//   f = th / sin th, and 1 + th^2/6 for th < kPgSmallAngle.
// Only the even function f of the acos enters, so a small angle loses nothing
// (th = 0 from a trace that rounds to 3 gives f = 1, off by th^2/6 < 1e-16).
// The rule is for th < pi. At th = pi (the clamp included) sin th is the sine of
// the double nearest pi, 1.2e-16, and f = 2.6e16: every term stays finite, an
// exact half turn (v = 0) gives log R = 0, and any other R that close to a half
// turn gives a vector that is no rotation vector. Such an edge is not refused.
// Jacobians for T <- exp(xi^) T, xi = (rho, phi) (se3_left_update):
//   D = [[I, -[t_e]x], [0, Jl^-1(log R_e)]],
//   Jl^-1(p) = I - 1/2 [p]x + k(th) [p]x^2, k = 1/th^2 - (1 + cos th)/(2 th sin th),
//   and 1/12 for th < kPgSmallAngle;
//   J_j = D,  J_i = -D Ad(A),  Ad(A) = [[R_A, [t_A]x R_A], [0, R_A]].
// Robust cost: q = e' Omega e, s = sqrt(q), Huber on s (delta <= 0: none):
// w = 1 or delta/s, cost = q/2 or delta (s - delta/2). q < 0 (an indefinite
// Omega) adds nothing: w = 0, cost = 0.
#pragma once

#include <cstddef>

#include "reproj_model.hpp"
#include "trig_pa.hpp"

namespace svo {

// below it the series of f and k: their next terms are 7 th^4/360 < 2e-18 and
// th^2/720 < 1.4e-11 (k multiplies [p]x^2 = O(th^2): 1e-19 of J)
constexpr double kPgSmallAngle = 1e-4;
// PCG stops at r'z <= kPgCgTol^2 r0'z0
constexpr double kPgCgTol = 1e-8;
// per edge: J_i' W J_j (36), then for end i and end j the 21 + 6 terms of the
// node's diagonal block and gradient
constexpr int kPgEdgeTerms = 36 + 27 + 27;

// Z = T_j T_i^-1 (also A of an edge)
SVO_MODEL_HD void pg_relative(const double* Ti, const double* Tj, double* Z) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            Z[3 * r + c] = Tj[3 * r] * Ti[3 * c] + Tj[3 * r + 1] * Ti[3 * c + 1] + Tj[3 * r + 2] * Ti[3 * c + 2];
#pragma unroll
    for (int r = 0; r < 3; r++) Z[9 + r] = Tj[9 + r] - (Z[3 * r] * Ti[9] + Z[3 * r + 1] * Ti[10] + Z[3 * r + 2] * Ti[11]);
}

// The edge at (Ti, Tj): e (6), J_i and J_j (6x6 row-major), the weight and the cost.
SVO_MODEL_HD void pg_edge_eval(const double* Ti, const double* Tj, const double* Z, const double* info, double delta,
                               double e[6], double Ji[36], double Jj[36], double& w, double& cost) {
    double A[12], E[12];
    pg_relative(Ti, Tj, A);
    pg_relative(Z, A, E);  // A Z^-1
    const double c0 = ((E[0] + E[4] + E[8]) - 1) * 0.5;
    const double c = c0 > 1 ? 1.0 : (c0 < -1 ? -1.0 : c0);
    const double th = la::pa::acos(c);
    double f, k;
    if (th < kPgSmallAngle) {
        f = 1 + th * th / 6;
        k = 1.0 / 12;
    } else {
        double sn, cs;
        la::pa::sincos(th, &sn, &cs);
        f = th / sn;
        k = 1 / (th * th) - (1 + cs) / (2 * th * sn);
    }
    e[0] = E[9], e[1] = E[10], e[2] = E[11];
    e[3] = f * (0.5 * (E[7] - E[5]));
    e[4] = f * (0.5 * (E[2] - E[6]));
    e[5] = f * (0.5 * (E[3] - E[1]));
    const double P[9] = {0, -e[5], e[4], e[5], 0, -e[3], -e[4], e[3], 0};  // [phi]x
    double Jl[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const double p2 = P[3 * r] * P[q] + P[3 * r + 1] * P[3 + q] + P[3 * r + 2] * P[6 + q];
            Jl[3 * r + q] = ((r == q ? 1.0 : 0.0) - 0.5 * P[3 * r + q]) + k * p2;
        }
    const double Tx[9] = {0, -e[2], e[1], e[2], 0, -e[0], -e[1], e[0], 0};  // [t_e]x
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            Jj[6 * r + q] = r == q ? 1.0 : 0.0;
            Jj[6 * r + 3 + q] = -Tx[3 * r + q];
            Jj[6 * (r + 3) + q] = 0.0;
            Jj[6 * (r + 3) + 3 + q] = Jl[3 * r + q];
        }
    // D Ad(A) = [[R_A, ([t_A]x - [t_e]x) R_A], [0, Jl^-1 R_A]]
    const double M[9] = {0, -(A[11] - e[2]), A[10] - e[1], A[11] - e[2], 0, -(A[9] - e[0]), -(A[10] - e[1]), A[9] - e[0], 0};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            Ji[6 * r + q] = -A[3 * r + q];
            Ji[6 * r + 3 + q] = -(M[3 * r] * A[q] + M[3 * r + 1] * A[3 + q] + M[3 * r + 2] * A[6 + q]);
            Ji[6 * (r + 3) + q] = 0.0;
            Ji[6 * (r + 3) + 3 + q] = -(Jl[3 * r] * A[q] + Jl[3 * r + 1] * A[3 + q] + Jl[3 * r + 2] * A[6 + q]);
        }
    double Om[36];
    {
        int n = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) {
                Om[6 * a + b] = Om[6 * b + a] = info[n];
                n++;
            }
    }
    double q = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double s = 0;
#pragma unroll
        for (int b = 0; b < 6; b++) s += Om[6 * a + b] * e[b];
        q += e[a] * s;
    }
    if (q < 0) {
        w = 0;
        cost = 0;
        return;
    }
    const double s = sqrt(q);
    const bool robust = delta > 0 && s > delta;
    w = robust ? delta / s : 1.0;
    cost = robust ? delta * (s - 0.5 * delta) : 0.5 * q;
}

// x' (w Omega) y for the columns a of X and b of Y (6x6 row-major), W = w Omega given
// as WY = W Y: sum over the rows in ascending order
SVO_MODEL_HD double pg_col_dot(const double* X, int a, const double* WY, int b) {
    double s = X[a] * WY[b];
#pragma unroll
    for (int r = 1; r < 6; r++) s += X[6 * r + a] * WY[6 * r + b];
    return s;
}

// The edge's kPgEdgeTerms from its e, J_i, J_j, w: out[k * stride], k =
//   [0, 36)  J_i' W J_j row-major, W = w Omega
//   [36, 63) end i: J_i' W J_i upper triangle row-major (21), J_i' W e (6)
//   [63, 90) end j: the same of J_j
SVO_MODEL_HD void pg_edge_terms(const double* info, double w, const double e[6], const double Ji[36], const double Jj[36],
                                double* out, size_t stride) {
    double W[36];
    {
        int n = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) {
                W[6 * a + b] = W[6 * b + a] = w * info[n];
                n++;
            }
    }
    double WJ[36], We[6];
    // W J_j, W e
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = 0; b < 6; b++) {
            double s = W[6 * a] * Jj[b];
#pragma unroll
            for (int r = 1; r < 6; r++) s += W[6 * a + r] * Jj[6 * r + b];
            WJ[6 * a + b] = s;
        }
        double s = W[6 * a] * e[0];
#pragma unroll
        for (int r = 1; r < 6; r++) s += W[6 * a + r] * e[r];
        We[a] = s;
    }
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) out[(6 * a + b) * stride] = pg_col_dot(Ji, a, WJ, b);
    {
        int n = 63;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) out[(n++) * stride] = pg_col_dot(Jj, a, WJ, b);
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double s = Jj[a] * We[0];
#pragma unroll
            for (int r = 1; r < 6; r++) s += Jj[6 * r + a] * We[r];
            out[(84 + a) * stride] = s;
        }
    }
    // W J_i
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) {
            double s = W[6 * a] * Ji[b];
#pragma unroll
            for (int r = 1; r < 6; r++) s += W[6 * a + r] * Ji[6 * r + b];
            WJ[6 * a + b] = s;
        }
    {
        int n = 36;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) out[(n++) * stride] = pg_col_dot(Ji, a, WJ, b);
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double s = Ji[a] * We[0];
#pragma unroll
            for (int r = 1; r < 6; r++) s += Ji[6 * r + a] * We[r];
            out[(57 + a) * stride] = s;
        }
    }
}

// lm_solve6's arithmetic in two halves, for a preconditioner that is factored
// once and applied many times. The factor: L (6x6 row-major, lower) of the block
// h (21 upper-triangle entries) damped as lm_solve6 damps it. False if the damped
// block is not positive definite; L is then unspecified.
SVO_MODEL_HD bool pg_chol6(const double* h, size_t stride, double lambda, double L[36]) {
    double A[36];
    {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = a; c < 6; c++) {
                A[6 * a + c] = A[6 * c + a] = h[k * stride];
                k++;
            }
    }
#pragma unroll
    for (int a = 0; a < 6; a++) A[7 * a] += lambda * (A[7 * a] > 0 ? A[7 * a] : 1e-12);
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
    return ok;
}

// x = (L L')^-1 b, lm_solve6's two substitutions. x may be b.
SVO_MODEL_HD void pg_chol6_solve(const double L[36], const double b[6], double x[6]) {
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
}

}  // namespace svo
