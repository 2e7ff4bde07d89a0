// What the two one-feature-per-wave kernels for any window share (lk_kernel in
// lk_generic.hip, lk_cv_kernel in lk_cv.hip): the strip lane map with run-time
// window sizes, the staging of the prev window and the next-image region as pixel
// pairs, and the fixed-point sampling of a lane's strip.
//  * Lane <-> pixel map: lane = g*win_w + c owns column c, rows [g*RPG,
//    (g+1)*RPG): vertically adjacent window pixels share J rows, so one GN
//    iteration reads RPG+1 rows x 2 bytes per lane instead of 4 per pixel.
//    21x21 -> 63 lanes x 7 rows exactly. FULL: groups * RPG == win_h, no row test.
#pragma once
#include "lk_device.hpp"

namespace svo {

namespace {

// Image region at (x0, y0) as horizontal pixel pairs: entry (r, e) =
// L(x0+e, y0+r) | L(x0+e+1, y0+r) << 16, ready for one v_dot2_i32_i16 per row;
// REFLECT_101 outside the image, as OpenCV's padded pyramid levels.
__device__ __forceinline__ void stage_pairs(unsigned* dst, const ImgLevel& L, int x0, int y0, int rw,
                                            int rh, int lr, int lc, int rpp) {
    if (lr >= rpp) return;
    gu8 src = (gu8)L.data;
    const bool inside = x0 >= 0 && y0 >= 0 && x0 + rw + 1 <= L.w && y0 + rh <= L.h;
    if (inside) {
        gu8 q = src + (size_t)(y0 + lr) * L.pitch + (x0 + lc);
        const size_t step = (size_t)rpp * L.pitch;
        for (int r = lr; r < rh; r += rpp, q += step) dst[r * rw + lc] = (unsigned)q[0] | ((unsigned)q[1] << 16);
    } else {
        const int sx0 = refl101(x0 + lc, L.w), sx1 = refl101(x0 + lc + 1, L.w);
        for (int r = lr; r < rh; r += rpp) {
            gu8 row = src + (size_t)refl101(y0 + r, L.h) * L.pitch;
            dst[r * rw + lc] = (unsigned)row[sx0] | ((unsigned)row[sx1] << 16);
        }
    }
}

// a lane's place in the strip map and in the two staging passes, and its wave's LDS
struct StripLane {
    int sc, r0;   // column and first row of the lane's strip
    bool strip;   // lanes past the map idle
    int i_rpp, i_lr, i_lc, j_rpp, j_lr, j_lc;  // staging: rows per pass, the lane's row and entry
    unsigned *ipair, *jreg;  // the prev window (+1 row/col) and the next-image region, as pixel pairs
};
template <int RPG>
__device__ __forceinline__ StripLane strip_lane(int lane, const LKDev& p, uint8_t* wave_lds) {
    StripLane m;
    m.sc = lane % p.win_w;
    const int sg = lane / p.win_w;
    m.strip = sg < p.groups;
    m.r0 = sg * RPG;
    m.i_rpp = 64 / p.ip_w, m.i_lr = lane / p.ip_w, m.i_lc = lane - m.i_lr * p.ip_w;
    m.j_rpp = 64 / p.jr_w, m.j_lr = lane / p.jr_w, m.j_lc = lane - m.j_lr * p.jr_w;
    m.ipair = reinterpret_cast<unsigned*>(wave_lds);
    m.jreg = reinterpret_cast<unsigned*>(wave_lds + p.ip_bytes);
    return m;
}
__device__ __forceinline__ void stage_next(const StripLane& m, const LKDev& p, const ImgLevel& J, int jx0, int jy0) {
    stage_pairs(m.jreg, J, jx0, jy0, p.jr_w, p.jr_h, m.j_lr, m.j_lc, m.j_rpp);
}

// A level's setup: stage the prev window (+1 row/col, as pixel pairs) and the
// next-image region around the initial window: one load burst, one LDS sync. The
// Scharr derivative comes from the precomputed derivative pyramid (zero outside the
// image, as OpenCV's zero-padded derivative level). Then the per-lane strip: bilinear
// I (x32), Ix, Iy at its window pixels and the lane's part of the normal matrix.
// (Returned by value: filled through references, the tall strips held the samples
// twice -- 239 VGPRs instead of 162 at 32 rows.)
template <int RPG>
struct StripSamples {
    int ival[RPG], gix[RPG], giy[RPG];  // I (x32), Ix, Iy at the lane's window pixels
    int a11, a12, a22;                  // the lane's part of the normal matrix
};
template <int RPG, bool FULL>
__device__ __forceinline__ StripSamples<RPG> strip_setup(const StripLane& m, const LKDev& p, const ImgLevel& I,
                                                         const ImgLevel& J, const DerivDesc& dprev, int level, int ipx,
                                                         int ipy, int jx0, int jy0, BiW iw) {
    StripSamples<RPG> s;
    auto& ival = s.ival;
    auto& gix = s.gix;
    auto& giy = s.giy;
    int a11 = 0, a12 = 0, a22 = 0;
    const int win_w = p.win_w, win_h = p.win_h, sc = m.sc, r0 = m.r0;
    const bool strip = m.strip;
    stage_pairs(m.ipair, I, ipx, ipy, p.ip_w, p.ip_h, m.i_lr, m.i_lc, m.i_rpp);
    stage_next(m, p, J, jx0, jy0);
    uint32_t dv[RPG + 1][2];
    {
        const int dpitch = dprev.pitch[level];
        gu32 dsrc = (gu32)dprev.data[level];
        const bool full_in = ipx >= 0 && ipy >= 0 && ipx + win_w < I.w && ipy + win_h < I.h;
        const int X = ipx + sc;
        if (full_in) {
            gu32 q = dsrc + (size_t)(ipy + r0) * dpitch + X;
#pragma unroll
            for (int k = 0; k <= RPG; k++) {
                dv[k][0] = dv[k][1] = 0;
                if (strip && (FULL || r0 + k <= win_h)) {
                    dv[k][0] = q[(size_t)k * dpitch];
                    dv[k][1] = q[(size_t)k * dpitch + 1];
                }
            }
        } else {
            const bool c0 = X >= 0 && X < I.w, c1 = X + 1 >= 0 && X + 1 < I.w;
#pragma unroll
            for (int k = 0; k <= RPG; k++) {
                dv[k][0] = dv[k][1] = 0;
                const int Y = ipy + r0 + k;
                if (strip && (FULL || r0 + k <= win_h) && Y >= 0 && Y < I.h) {
                    gu32 q = dsrc + (size_t)Y * dpitch + X;
                    if (c0) dv[k][0] = q[0];
                    if (c1) dv[k][1] = q[1];
                }
            }
        }
    }
    wave_lds_sync();

    const unsigned IW0 = iw.W0, IW1 = iw.W1;
    const unsigned* ip = m.ipair + r0 * p.ip_w + sc;
    unsigned P0 = strip ? ip[0] : 0u;
#pragma unroll
    for (int j = 0; j < RPG; j++) {
        ival[j] = gix[j] = giy[j] = 0;
        if (strip && (FULL || r0 + j < win_h)) {
            const unsigned P1 = ip[(j + 1) * p.ip_w];
            ival[j] = sdot2(P0, IW0, sdot2(P1, IW1, 1 << (W_BITS - 6))) >> (W_BITS - 5);
            P0 = P1;
            const unsigned X0 = __builtin_amdgcn_perm(dv[j][1], dv[j][0], 0x05040100u);
            const unsigned X1 = __builtin_amdgcn_perm(dv[j + 1][1], dv[j + 1][0], 0x05040100u);
            const unsigned Y0 = __builtin_amdgcn_perm(dv[j][1], dv[j][0], 0x07060302u);
            const unsigned Y1 = __builtin_amdgcn_perm(dv[j + 1][1], dv[j + 1][0], 0x07060302u);
            constexpr int DS = W_BITS + kDerShift;  // derivatives are stored x 2^kDerShift
            const int ix = sdot2(X0, IW0, sdot2(X1, IW1, 1 << (DS - 1))) >> DS;
            const int iy = sdot2(Y0, IW0, sdot2(Y1, IW1, 1 << (DS - 1))) >> DS;
            gix[j] = ix;
            giy[j] = iy;
            a11 += ix * ix;
            a12 += ix * iy;
            a22 += iy * iy;
        }
    }
    s.a11 = a11;
    s.a12 = a12;
    s.a22 = a22;
    return s;
}

// the lane's strip of the next image at window top-left (x, y) inside the staged
// region at (jx0, jy0): f(k, J (x32) at row r0 + k) for the strip's rows
template <int RPG, bool FULL, class F>
__device__ __forceinline__ void for_next_rows(const StripLane& m, const LKDev& p, int x, int y, int jx0, int jy0,
                                              BiW w, F f) {
    if (!m.strip) return;
    const unsigned* jp = m.jreg + (y - jy0 + m.r0) * p.jr_w + (x - jx0 + m.sc);
    unsigned p0 = jp[0];
#pragma unroll
    for (int k = 0; k < RPG; k++) {
        if (FULL || m.r0 + k < p.win_h) {
            const unsigned p1 = jp[(k + 1) * p.jr_w];
            f(k, sdot2(p0, w.W0, sdot2(p1, w.W1, 1 << (W_BITS - 6))) >> (W_BITS - 5));
            p0 = p1;
        }
    }
}

// the error of flags 0 + err (sad_error) on the strip map
template <int RPG, bool FULL>
__device__ __forceinline__ bool strip_sad_error(const StripLane& m, const LKDev& p, const ImgLevel& J, float nx,
                                                float ny, int& jx0, int& jy0, const int (&ival)[RPG], float& errv) {
    return sad_error<JM>(
        nx, ny, J.w, J.h, p.win_w, p.win_h, jx0, jy0, [&] { stage_next(m, p, J, jx0, jy0); },
        [&](int x, int y, BiW w) {
            int sad = 0;
            for_next_rows<RPG, FULL>(m, p, x, y, jx0, jy0, w, [&](int k, int jv) {
                const int diff = jv - ival[k];
                sad += diff < 0 ? -diff : diff;
            });
            return sad;
        },
        errv);
}

}  // namespace

}  // namespace svo
