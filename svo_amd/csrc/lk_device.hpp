// What more than one Lucas-Kanade kernel uses (lk.hip is the host entry; the
// kernels live in lk_multi.hip, lk_cvq.hip, lk_fast.hip, lk_generic.hip and
// lk_cv.hip): the kernels' parameter block, OpenCV's fixed-point and exit rules
// -- each stated once, here -- the exact wave reductions and the global-load
// forms. Everything is internal to a translation unit (unnamed namespace): only
// the launch wrappers declared at the end cross files.
#pragma once
#include "common.hpp"

#include <cfloat>
#include <cmath>

namespace svo {

namespace {

constexpr int W_BITS = 14;
constexpr float FLT_SCALE = 1.f / (1 << 20);
constexpr int JM = 3;  // margin (px) of the staged next-image region around the window (one feature per wave)

struct LKDev {
    int win_w, win_h, groups;      // strip map: groups = lanes/win_w, RPG rows each
    int ip_w, ip_h, jr_w, jr_h;    // staged prev / next pair regions (entries x rows)
    int ip_bytes, lds_wave;        // per-wave LDS carve
    int max_level, max_count;
    double eps2;
    float eps2_lo, eps2_hi;  // float brackets of eps2 (see converged())
    int flags, want_err;
    float min_eig;
};

// the kernels' parameter block of one call (every launch wrapper fills its own)
inline LKDev lk_dev(const LKParams& lp) {
    LKDev d;
    d.win_w = lp.win_w;
    d.win_h = lp.win_h;
    d.groups = 64 / lp.win_w;
    d.ip_w = lp.win_w;                // prev window: win_w pairs x (win_h + 1) rows
    d.ip_h = lp.win_h + 1;
    d.jr_w = lp.win_w + 2 * JM;       // next region: pair entries per row (win_w + 2JM + 1 pixels)
    d.jr_h = lp.win_h + 1 + 2 * JM;
    d.ip_bytes = (d.ip_w * d.ip_h * 4 + 15) & ~15;
    d.lds_wave = d.ip_bytes + ((d.jr_w * d.jr_h * 4 + 15) & ~15);
    d.max_level = lp.max_level;
    d.max_count = lp.max_count;
    d.eps2 = lp.eps2;
    // |float(dx*dx + dy*dy) / exact - 1| <= 3 * 2^-24: outside eps2 * (1 -+ 2^-20) the
    // float sum decides the double comparison exactly
    d.eps2_lo = (float)(lp.eps2 * (1.0 - 0x1p-20));
    d.eps2_hi = (float)(lp.eps2 * (1.0 + 0x1p-20));
    if ((double)d.eps2_lo > lp.eps2 * (1.0 - 0x1p-20)) d.eps2_lo = nextafterf(d.eps2_lo, 0.f);
    if ((double)d.eps2_hi < lp.eps2 * (1.0 + 0x1p-20)) d.eps2_hi = nextafterf(d.eps2_hi, INFINITY);
    d.flags = lp.flags;
    d.want_err = lp.want_err;
    d.min_eig = lp.min_eig;
    return d;
}

// OpenCV's `delta.ddot(delta) <= criteria.epsilon^2` (double products of float
// deltas) decided in float where the float sum is far enough from eps2, in double
// only inside the 2^-20 band around it
__device__ __forceinline__ bool converged(float dx, float dy, float lo, float hi, double eps2) {
    const float sf = dx * dx + dy * dy;
    bool c = sf < lo;
    if (__builtin_expect(sf >= lo && sf <= hi, 0)) {
        // (a real branch: if-converted, the double products cost every iteration of
        // every wave ~10 VALU issue slots for a band no lane is in)
        asm volatile("" ::: "memory");
        c = (double)dx * dx + (double)dy * dy <= eps2;
    }
    return c;
}
// `std::abs(a + b) < 0.01` with a float sum promoted to double: the largest float
// below 0.01 is the bound
__device__ __forceinline__ bool below_001(float v) { return fabsf(v) <= 0x1.47ae14p-7f; }

__device__ __forceinline__ int refl101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        p = p < 0 ? -p : 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

__device__ __forceinline__ int ufloor(float v) {  // cvFloor (identical for |v| < 2^31)
    return (int)__builtin_floorf(v);
}
__device__ __forceinline__ float uni_f(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ int uni_i(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the first point of sequence seq a launch covers (LKBatch::first; 0 without it)
__device__ __forceinline__ int lk_first(const LKBatch& B, int seq) { return B.first ? B.first[seq] : 0; }

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Exact wave sum of int32 values whose 64-lane total may exceed int32: sum the
// high and low 16-bit halves separately with DPP adds (exact), combine in int64.
__device__ __forceinline__ int dpp_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xb1, 0xf, 0xf, true);   // quad_perm 1,0,3,2
    v += __builtin_amdgcn_update_dpp(0, v, 0x4e, 0xf, 0xf, true);   // quad_perm 2,3,0,1
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);  // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);  // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ double wave_sum_exact(int v) {
    int hi = dpp_sum(v >> 16);
    int lo = dpp_sum(v & 0xFFFF);
    return (double)((long long)hi * 65536 + (long long)lo);
}
template <int CTRL, int ROW_MASK, bool BC>
__device__ __forceinline__ int dpp_add(int v) {
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, BC);
}

typedef const __attribute__((address_space(1))) uint8_t* gu8;  // global (not flat) loads
typedef const __attribute__((address_space(1))) uint32_t* gu32;
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint16_t u16a1 __attribute__((aligned(1)));  // unaligned 2-byte global loads
typedef uint32_t u32a1 __attribute__((aligned(1)));  // dword loads at any byte address (tools/unaligned_probe.hip)
typedef const __attribute__((address_space(4))) PyrDesc* cpyr;  // scalar (s_load) descriptor reads

// Global loads at a wave-uniform base plus an unsigned 32-bit byte offset: the
// saddr + voffset form (no 64-bit address arithmetic per lane). Padded levels:
// the base is the padded origin, so every offset inside the padding is >= 0.
template <typename T>
__device__ __forceinline__ T ldg_off(gu8 base, unsigned off) {
    return *(const __attribute__((address_space(1))) T*)(base + off);
}
__device__ __forceinline__ gu8 pad_origin(const uint8_t* data, int pitch, int pad_px, int elem) {
    return (gu8)data - (size_t)pad_px * ((size_t)pitch + 1) * elem;
}

// v_dot2_i32_i16: both operands signed 16-bit -- OpenCV's rounded bilinear weights
// can be -1 (iw11 = 2^14 - iw00 - iw01 - iw10), pixels 0..255 and Scharr values
// |v| <= 4080 fit, and every partial sum fits int32.
__device__ __forceinline__ int sdot2(unsigned a, unsigned b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, false);
}
// v_dot2_i32_i16 in its VOP3P form with a register accumulator: the compiler
// otherwise picks v_dot2c (accumulator = destination) plus a v_mov of the
// rounding constant for every use.
__device__ __forceinline__ int sdot2_r(unsigned a, unsigned b, int c) {
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ unsigned lo16x2(int lo, int hi) {  // (lo & 0xffff) | (hi << 16) in one v_perm
    return __builtin_amdgcn_perm((unsigned)hi, (unsigned)lo, 0x05040100u);
}

// OpenCV's rounded bilinear weights (LKTrackerInvoker: iw00 = cvRound((1 - a)(1 - b)
// 2^14), iw01, iw10, iw11 = 2^14 - the others), packed for v_dot2 as (w00 | w01 << 16,
// w10 | w11 << 16). cvRound(p 2^14) for a float product p in [0, 1] is computed as
// p + 768: that sum lies in [768, 1024), where the float grid is 2^-14, so the
// addition rounds p to a multiple of 2^-14 with ties to even -- rint's rounding --
// and the low mantissa bits then hold round(p 2^14) (768.f = 0x44400000 has zero
// low bits). Fast-rate adds in place of rndne + cvt (both half-rate on gfx950).
__device__ __forceinline__ unsigned wbits(float p) { return __float_as_uint(p + 768.f); }
struct BiW {
    unsigned W0, W1;
};
__device__ __forceinline__ BiW bilinear_weights(float a, float b) {
    const float ia = 1.f - a, ib = 1.f - b;
    const unsigned b00 = wbits(ia * ib), b01 = wbits(a * ib), b10 = wbits(ia * b);
    // 2^14 - w00 - w01 - w10 with w = bits - 0x44400000, modulo 2^32 (w11 may be -1)
    const unsigned w11 = (1u << W_BITS) + 3u * 0x44400000u - b00 - b01 - b10;
    return {__builtin_amdgcn_perm(b01, b00, 0x05040100u), __builtin_amdgcn_perm(w11, b10, 0x05040100u)};
}

// floor(x), floor(y) as ints and the weights of the fractions: a = x - floor(x) --
// the float of the floor is the floor (|x| < 2^24)
struct SubPix {
    int ix, iy;
    BiW w;
};
__device__ __forceinline__ SubPix sub_pixel(float x, float y) {
    const float fx = __builtin_floorf(x), fy = __builtin_floorf(y);
    return {(int)fx, (int)fy, bilinear_weights(x - fx, y - fy)};
}
// OpenCV's bounds test of a window's top-left pixel: x < -win_w || x >= w || y < -win_h
// || y >= h is out; one unsigned compare per axis
__device__ __forceinline__ bool window_in_bounds(int x, int y, int w, int h, int win_w, int win_h) {
    return (unsigned)(x + win_w) < (unsigned)(w + win_w) && (unsigned)(y + win_h) < (unsigned)(h + win_h);
}

// The start of a pyramid level (LKTrackerInvoker's prologue): the feature at this
// level's scale, the guess (the initial flow or the feature itself at the top level,
// twice the level above's result below it: the caller stores it to (nx, ny), the
// result of a level that is skipped), the prev window's top-left pixel, its bounds
// test and the fractions (a, b) for bilinear_weights. (nextx, nexty) is the guess as
// the window's centre. Everything by value, and the weights left to the caller: the
// kernels' code then comes out as if the statements stood in their bodies.
struct LevelStart {
    float nextx, nexty;
    int ipx, ipy;
    bool inb;
    float a, b;
};
__device__ __forceinline__ LevelStart level_start(float px, float py, float nx, float ny, int level, int max_level,
                                                  int flags, int lw, int lh, int win_w, int win_h) {
    const float halfWx = (win_w - 1) * 0.5f, halfWy = (win_h - 1) * 0.5f;
    const float lscale = __builtin_amdgcn_ldexpf(1.f, -level);  // == (float)(1. / (1 << level))
    float prevx = px * lscale, prevy = py * lscale;
    float nextx, nexty;
    if (level == max_level) {
        if (flags & SVO_LK_USE_INITIAL_FLOW) {
            nextx = nx * lscale;
            nexty = ny * lscale;
        } else {
            nextx = prevx;
            nexty = prevy;
        }
    } else {
        nextx = nx * 2.f;
        nexty = ny * 2.f;
    }
    prevx -= halfWx;
    prevy -= halfWy;
    const float fpx = __builtin_floorf(prevx), fpy = __builtin_floorf(prevy);
    const int ipx = (int)fpx, ipy = (int)fpy;
    return {nextx, nexty, ipx, ipy, window_in_bounds(ipx, ipy, lw, lh, win_w, win_h), prevx - fpx, prevy - fpy};
}

// One feature per wave: the staged next-image region (origin (jx0, jy0), margin M
// around the window) follows a window position (x, y) that left it -- `stage`
// re-stages at the new origin.
template <int M, class Stage>
__device__ __forceinline__ void follow_region(int x, int y, int& jx0, int& jy0, Stage stage) {
    if ((unsigned)(x - jx0) > 2u * M || (unsigned)(y - jy0) > 2u * M) {
        // the window left the staged region: re-stage around it
        jx0 = x - M;
        jy0 = y - M;
        wave_lds_sync();
        stage();
        wave_lds_sync();
    }
}

// The error of flags 0 + err at level 0 (one feature per wave): the mean absolute
// J - I (x32) over the window at the final position. `row_sad(x, y, w)` is the
// lane's sum of |diff| over its window pixels at top-left (x, y). False (status 0)
// when the window left the image.
// |diff| sums stay < 2^24 for windows <= 2048 px: exact in float, in any order
template <int M, class Stage, class RowSad>
__device__ __forceinline__ bool sad_error(float nx, float ny, int jw, int jh, int win_w, int win_h, int& jx0,
                                          int& jy0, Stage stage, RowSad row_sad, float& errv) {
    const SubPix s = sub_pixel(nx - (win_w - 1) * 0.5f, ny - (win_h - 1) * 0.5f);
    const int ix0 = uni_i(s.ix), iy0 = uni_i(s.iy);
    if (!window_in_bounds(ix0, iy0, jw, jh, win_w, win_h)) return false;
    follow_region<M>(ix0, iy0, jx0, jy0, stage);
    errv = (float)wave_sum_exact(row_sad(ix0, iy0, s.w)) * 1.f / (float)(32 * win_w * win_h);
    return true;
}

// a feature's result (one feature per wave)
__device__ __forceinline__ void store_track(const LKBatch& B, float* next_xy, size_t base, int pt, float nx,
                                            float ny, int st, float errv, int itcount) {
    next_xy[2 * pt] = nx;
    next_xy[2 * pt + 1] = ny;
    B.status[base + pt] = (uint8_t)st;
    if (B.err) B.err[base + pt] = errv;
    if (B.iters) B.iters[base + pt] = itcount;
}

}  // namespace

// The launch wrappers, one per kernel family (each in its kernel's file); lk.hip's
// launch_lk picks among them.
hipError_t launch_lk_multi_temporal(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st);  // 21 x 21
hipError_t launch_lk_multi_stereo(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st);    // 11 x 11
hipError_t launch_lk_cvq(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st);  // 21 x 21, 11 x 11
hipError_t launch_lk_fast(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st);  // 11, 15, 21, 31 square
hipError_t launch_lk_generic(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st);
hipError_t launch_lk_cv(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st);

}  // namespace svo
