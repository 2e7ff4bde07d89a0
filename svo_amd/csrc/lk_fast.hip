// lk_fast_kernel: one wave64 per feature, compile-time window sizes (the
// reference's 21x21 and 11x11, plus 15x15 / 31x31); the kernel of the SAD error
// (flags 0 + err) and of SVO_LK_QUAD=0. Same semantics and lane map as lk_kernel
// (lk_generic.hip); the differences are all instruction count:
//  * staging loads whole aligned dwords (4 pixels) per lane and builds the 4
//    pixel pairs with v_perm from its dword and the next lane's (ds_bpermute),
//    one ds_write_b128 per lane: 1 VMEM instruction per 4 pairs instead of 8;
//  * LDS strides are compile-time (ds_read2 with immediate offsets);
//  * two window rows are processed per packed op: the J-I differences of a row
//    pair are packed to int16x2 (v_perm + v_pk_sub_i16) and multiplied into the
//    normal equations with one v_dot2_i32_i16 per sum (b1, b2, A11, A12, A22),
//    replacing two quarter-rate v_mul_lo_u32 per pixel and sum.
// All values fit int16 (|J - I| <= 8160, |Ix|, |Iy| <= 4080) and the per-lane
// int32 sums cannot overflow (at most 16 rows x 8160 x 4080 < 2^31), so the sums
// are the same exact integers as before: bit-identical results.
#include "lk_device.hpp"

namespace svo {

namespace {

constexpr int ru4(int v) { return (v + 3) & ~3; }
typedef const __attribute__((address_space(1))) u16a1* gu16u;  // unaligned 2-byte global loads

template <int WW, int WH>
struct Shape {
    static constexpr int G = 64 / WW;               // row groups of the strip map
    static constexpr int RPG = (WH + G - 1) / G;     // rows per group
    static constexpr bool FULL = G * RPG == WH;
    static constexpr int NP = (RPG + 1) / 2;        // packed row pairs per lane
    static constexpr int IPW = ru4(WW + 3), IPH = WH + 1;           // I pairs: entries x rows
    static constexpr int JRW = ru4(WW + 2 * JM + 3), JRH = WH + 1 + 2 * JM;
    static constexpr int IBYTES = IPW * IPH * 4, JBYTES = JRW * JRH * 4;
    static constexpr int WAVE_BYTES = IBYTES + JBYTES + 16;  // + a sink for the stager's spare lanes
};

// Exact wave sums of int32 values. A lane's b1, b2, A11, A12, A22 are bounded by
// RPG * 8160 * 4080 (RPG rows of |J - I| <= 8160 times |Ix| <= 4080): the first
// S32 DPP steps (2^S32-lane partial sums) run in int32 -- three where eight
// lanes' bound stays below 2^31 (strips of up to 8 rows: 11, 15 and 21 px), two
// for the 16-row strips of 31 x 31, whose eight lanes reach 4.26e9 (steps32) --
// then each partial is split into 16-bit halves for the remaining steps, all
// chains interleaved so that no DPP read waits on the write before it (no s_nop
// padding). The results are
// the FLT_SCALE'd floats: hi * 65536 is exact in float (|hi| < 2^24) and the one
// addition rounds the exact total once -- the same float as
// (float)(double)(int64 total), without the int64 / double detour.
__device__ __forceinline__ float halves_to_float(int hi_lane, int lo_lane) {
    const float h = (float)__builtin_amdgcn_readlane(hi_lane, 63);
    const float l = (float)__builtin_amdgcn_readlane(lo_lane, 63);
    return (h * 65536.f + l) * FLT_SCALE;
}

constexpr int steps32(int rpg) { return 8ll * rpg * 8160 * 4080 < (1ll << 31) ? 3 : 2; }

template <int S32>
__device__ __forceinline__ void wave_sum_f2(int x, int y, float& fx, float& fy) {
    static_assert(S32 == 2 || S32 == 3, "row_shr:4 in int32 or on the halves");
    x = dpp_add<0xb1, 0xf, true>(x);
    y = dpp_add<0xb1, 0xf, true>(y);
    x = dpp_add<0x4e, 0xf, true>(x);
    y = dpp_add<0x4e, 0xf, true>(y);
    if (S32 == 3) {
        x = dpp_add<0x114, 0xf, true>(x);
        y = dpp_add<0x114, 0xf, true>(y);
    }
    int xh = x >> 16, xl = x & 0xFFFF, yh = y >> 16, yl = y & 0xFFFF;
    if (S32 == 2) {
        xh = dpp_add<0x114, 0xf, true>(xh);
        xl = dpp_add<0x114, 0xf, true>(xl);
        yh = dpp_add<0x114, 0xf, true>(yh);
        yl = dpp_add<0x114, 0xf, true>(yl);
    }
    xh = dpp_add<0x118, 0xf, true>(xh);
    xl = dpp_add<0x118, 0xf, true>(xl);
    yh = dpp_add<0x118, 0xf, true>(yh);
    yl = dpp_add<0x118, 0xf, true>(yl);
    xh = dpp_add<0x142, 0xa, false>(xh);
    xl = dpp_add<0x142, 0xa, false>(xl);
    yh = dpp_add<0x142, 0xa, false>(yh);
    yl = dpp_add<0x142, 0xa, false>(yl);
    xh = dpp_add<0x143, 0xc, false>(xh);
    xl = dpp_add<0x143, 0xc, false>(xl);
    yh = dpp_add<0x143, 0xc, false>(yh);
    yl = dpp_add<0x143, 0xc, false>(yl);
    fx = halves_to_float(xh, xl);
    fy = halves_to_float(yh, yl);
}

// three chains: the normal matrix (A11, A12, A22) in one pass
template <int S32>
__device__ __forceinline__ void wave_sum_f3(int x, int y, int z, float& fx, float& fy, float& fz) {
    static_assert(S32 == 2 || S32 == 3, "row_shr:4 in int32 or on the halves");
    x = dpp_add<0xb1, 0xf, true>(x);
    y = dpp_add<0xb1, 0xf, true>(y);
    z = dpp_add<0xb1, 0xf, true>(z);
    x = dpp_add<0x4e, 0xf, true>(x);
    y = dpp_add<0x4e, 0xf, true>(y);
    z = dpp_add<0x4e, 0xf, true>(z);
    if (S32 == 3) {
        x = dpp_add<0x114, 0xf, true>(x);
        y = dpp_add<0x114, 0xf, true>(y);
        z = dpp_add<0x114, 0xf, true>(z);
    }
    int xh = x >> 16, xl = x & 0xFFFF, yh = y >> 16, yl = y & 0xFFFF, zh = z >> 16, zl = z & 0xFFFF;
    if (S32 == 2) {
        xh = dpp_add<0x114, 0xf, true>(xh);
        xl = dpp_add<0x114, 0xf, true>(xl);
        yh = dpp_add<0x114, 0xf, true>(yh);
        yl = dpp_add<0x114, 0xf, true>(yl);
        zh = dpp_add<0x114, 0xf, true>(zh);
        zl = dpp_add<0x114, 0xf, true>(zl);
    }
    xh = dpp_add<0x118, 0xf, true>(xh);
    xl = dpp_add<0x118, 0xf, true>(xl);
    yh = dpp_add<0x118, 0xf, true>(yh);
    yl = dpp_add<0x118, 0xf, true>(yl);
    zh = dpp_add<0x118, 0xf, true>(zh);
    zl = dpp_add<0x118, 0xf, true>(zl);
    xh = dpp_add<0x142, 0xa, false>(xh);
    xl = dpp_add<0x142, 0xa, false>(xl);
    yh = dpp_add<0x142, 0xa, false>(yh);
    yl = dpp_add<0x142, 0xa, false>(yl);
    zh = dpp_add<0x142, 0xa, false>(zh);
    zl = dpp_add<0x142, 0xa, false>(zl);
    xh = dpp_add<0x143, 0xc, false>(xh);
    xl = dpp_add<0x143, 0xc, false>(xl);
    yh = dpp_add<0x143, 0xc, false>(yh);
    yl = dpp_add<0x143, 0xc, false>(yl);
    zh = dpp_add<0x143, 0xc, false>(zh);
    zl = dpp_add<0x143, 0xc, false>(zl);
    fx = halves_to_float(xh, xl);
    fy = halves_to_float(yh, yl);
    fz = halves_to_float(zh, zl);
}

__device__ __forceinline__ unsigned pk_sub16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_bit_cast(s16x2, a) - __builtin_bit_cast(s16x2, b));
}

// Stage rows [0, H) x pair entries [0, W) of the region whose pixel origin is
// (xa, y0), xa a multiple of 4: entry (r, e) = L(xa+e, y0+r) | L(xa+e+1, y0+r) << 16.
// REFLECT_101 outside the image (slow path, border windows only).
// Branch-free inside the image (no exec-mask branches, which cost ~5 SALU
// each): every lane loads a valid dword (rows past the region re-read the last
// row, so they carry the same bytes as that row's owner; dword loads may run past
// the row end, never past the allocation: 256 B slack) and every lane writes:
// lanes without a complete set of pairs write to `sink`. A scheduling barrier
// per pass keeps the compiler from hoisting all loads (register pressure).
template <int W, int H>
__device__ __forceinline__ void stage_bf(unsigned* dst, unsigned* sink, const ImgLevel& L, int xa, int y0,
                                         int lane) {
    constexpr int LPR = W / 4 + 1, RPP = 64 / LPR, NP = (H + RPP - 1) / RPP;
    const int lr = lane / LPR, d = lane - lr * LPR;
    const bool inside = xa >= 0 && y0 >= 0 && xa + W + 1 <= L.w && y0 + H <= L.h;
    if (inside) {
        gu8 src = (gu8)L.data + xa + 4 * d;
        unsigned* dpl = (d < W / 4 && lr < RPP) ? dst + 4 * d : sink;
        const int dstride = (d < W / 4 && lr < RPP) ? W : 0;
#pragma unroll
        for (int q = 0; q < NP; q++) {
            int r = q * RPP + lr;
            r = r < H ? r : H - 1;
            const unsigned v = *(gu32)(src + (size_t)(y0 + r) * L.pitch);
            const unsigned nv = (unsigned)__builtin_amdgcn_ds_bpermute((lane + 1) << 2, (int)v);
            uint4 o;
            o.x = __builtin_amdgcn_perm(nv, v, 0x0c010c00u);
            o.y = __builtin_amdgcn_perm(nv, v, 0x0c020c01u);
            o.z = __builtin_amdgcn_perm(nv, v, 0x0c030c02u);
            o.w = __builtin_amdgcn_perm(nv, v, 0x0c040c03u);
            *reinterpret_cast<uint4*>(dpl + r * dstride) = o;
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        gu8 src = (gu8)L.data;
        for (int k = lane; k < W * H; k += 64) {
            const int r = k / W, e = k - r * W;
            gu8 row = src + (size_t)refl101(y0 + r, L.h) * L.pitch;
            dst[k] = (unsigned)row[refl101(xa + e, L.w)] | ((unsigned)row[refl101(xa + e + 1, L.w)] << 16);
        }
    }
}

// (launch bound: occupancy is limited by LDS (7 blocks/CU) and ~70 VGPRs alike;
// capping the VGPRs lower spills -- measured: launch bounds 6/7/8 waves all slower)
template <int WW, int WH>
__global__ __launch_bounds__(256, 1) void lk_fast_kernel(LKBatch B, LKDev p) {
    using S = Shape<WW, WH>;
    constexpr int RPG = S::RPG, NP = S::NP;
    constexpr int S32 = steps32(RPG);  // DPP steps of the wave sums that stay in int32
    static_assert((1ll << S32) * RPG * 8160 * 4080 < (1ll << 31), "2^S32 lanes' partial sums must fit int32");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int seq = blockIdx.y;
    const int n = B.counts ? B.counts[seq] : B.n;
    // a wave per feature; a grid smaller than the count (LKBatch::grid_hint) loops
    for (int pt = lk_first(B, seq) + blockIdx.x * 4 + wid; pt < n; pt += gridDim.x * 4) {
    const size_t base = (size_t)seq * B.cap;
    const float* __restrict__ prev_xy = B.prev_xy + 2 * base;
    float* __restrict__ next_xy = B.next_xy + 2 * base;
    // descriptors through the scalar cache (uniform per wave)
    const cpyr prev = (cpyr)B.prev + seq;
    const cpyr next = (cpyr)B.next + seq;
    const DerivDesc& dprev = B.dprev[seq];
    unsigned* ipair = reinterpret_cast<unsigned*>(lds + wid * S::WAVE_BYTES);
    unsigned* jreg = reinterpret_cast<unsigned*>(lds + wid * S::WAVE_BYTES + S::IBYTES);
    unsigned* sink = reinterpret_cast<unsigned*>(lds + wid * S::WAVE_BYTES + S::IBYTES + S::JBYTES);

    const int sc = lane % WW;
    const int sg = lane / WW;
    const bool strip = sg < S::G;
    // lanes outside the strip map (and rows past the window) run the same code on
    // in-range addresses; their derivatives are zeroed, so they add nothing
    const int r0 = (strip ? sg : 0) * RPG;
    const int rnd_i = 1 << (W_BITS - 6), rnd_d = 1 << (W_BITS + kDerShift - 1);

    constexpr float halfWx = (WW - 1) * 0.5f, halfWy = (WH - 1) * 0.5f;
    const float px = uni_f(prev_xy[2 * pt]), py = uni_f(prev_xy[2 * pt + 1]);
    float nx = 0.f, ny = 0.f;
    if (p.flags & SVO_LK_USE_INITIAL_FLOW) {
        nx = uni_f(next_xy[2 * pt]);
        ny = uni_f(next_xy[2 * pt + 1]);
    }
    int st = 1;
    float errv = 0.f;
    int itcount = 0;
    const int max_level = p.max_level;

    for (int level = max_level; level >= 0; level--) {
        const ImgLevel I{prev->lv[level].data, prev->lv[level].w, prev->lv[level].h, prev->lv[level].pitch};
        const ImgLevel J{next->lv[level].data, next->lv[level].w, next->lv[level].h, next->lv[level].pitch};
        const LevelStart start = level_start(px, py, nx, ny, level, max_level, p.flags, I.w, I.h, WW, WH);
        float nextx = start.nextx, nexty = start.nexty;
        nx = nextx;
        ny = nexty;
        if (!start.inb) {
            if (level == 0) {
                st = 0;
                errv = 0.f;
            }
            continue;
        }
        const int ipx = uni_i(start.ipx), ipy = uni_i(start.ipy);
        const BiW iw = bilinear_weights(start.a, start.b);
        const unsigned IW0 = iw.W0, IW1 = iw.W1;

        const int ixa = ipx & ~3;
        int jx0 = uni_i(ufloor(nextx - halfWx)) - JM, jy0 = uni_i(ufloor(nexty - halfWy)) - JM;
        int jxa = jx0 & ~3;
        // every top-left position of the staged region passes the image-bound test
        bool jsafe;
        const auto stage_next = [&] {
            jxa = jx0 & ~3;
            jsafe = jx0 >= -WW && jx0 + 2 * JM < J.w && jy0 >= -WH && jy0 + 2 * JM < J.h;
            stage_bf<S::JRW, S::JRH>(jreg, sink, J, jxa, jy0, lane);
        };
        // window (and its +1 bilinear row/column) inside the level: I pairs and
        // derivative pairs come straight from HBM; else REFLECT_101 staging / zeros
        const bool full_in = ipx >= 0 && ipy >= 0 && ipx + WW < I.w && ipy + WH < I.h;
        stage_next();
        unsigned P[RPG + 1];   // I(x, y) | I(x + 1, y) << 16 at the lane's column, rows r0 .. r0 + RPG
        u32x2a4 dv[RPG + 1];   // (Ix|Iy) at columns X, X+1 of each row: one dwordx2 load
        {
            const int dpitch = dprev.pitch[level];
            gu32 dsrc = (gu32)dprev.data[level];
            const int X = ipx + sc;
            if (full_in) {
                gu8 ib = (gu8)I.data + (size_t)(ipy + r0) * I.pitch + X;
                gu32 q = dsrc + (size_t)(ipy + r0) * dpitch + X;
#pragma unroll
                for (int k = 0; k <= RPG; k++) {
                    const int kk = (S::FULL || r0 + k <= WH) ? k : 0;  // stay inside the window
                    const unsigned v = *(gu16u)(ib + (size_t)kk * I.pitch);
                    P[k] = __builtin_amdgcn_perm(0u, v, 0x0c010c00u);
                    dv[k] = *(const __attribute__((address_space(1))) u32x2a4*)(q + (size_t)kk * dpitch);
                }
            } else {
                stage_bf<S::IPW, S::IPH>(ipair, sink, I, ixa, ipy, lane);
                const bool c0 = X >= 0 && X < I.w, c1 = X + 1 >= 0 && X + 1 < I.w;
#pragma unroll
                for (int k = 0; k <= RPG; k++) {
                    dv[k] = u32x2a4{0u, 0u};
                    const int Y = ipy + r0 + k;
                    if ((S::FULL || r0 + k <= WH) && Y >= 0 && Y < I.h) {
                        gu32 q = dsrc + (size_t)Y * dpitch + X;
                        if (c0) dv[k].x = q[0];
                        if (c1) dv[k].y = q[1];
                    }
                }
                wave_lds_sync();
                const unsigned* ip = ipair + r0 * S::IPW + (ipx - ixa) + sc;
#pragma unroll
                for (int k = 0; k <= RPG; k++) P[k] = ip[(S::FULL || r0 + k <= WH ? k : 0) * S::IPW];
            }
        }
        wave_lds_sync();

        // ---- I (x32), Ix, Iy at the lane's RPG window pixels, packed by row pairs ----
        // Lanes outside the strip map get zero derivative weights (their Ix, Iy
        // come out 0: rnd_d >> (W_BITS + kDerShift) == 0), so no branch per row.
        unsigned I2[NP], GX2[NP], GY2[NP];
        int a11 = 0, a12 = 0, a22 = 0;
        {
            const unsigned GW0 = strip ? IW0 : 0u, GW1 = strip ? IW1 : 0u;
            int iv[2 * NP], gx[2 * NP], gy[2 * NP];
#pragma unroll
            for (int j = 0; j < 2 * NP; j++) iv[j] = gx[j] = gy[j] = 0;
#pragma unroll
            for (int j = 0; j < RPG; j++) {
                iv[j] = sdot2(P[j], IW0, sdot2_r(P[j + 1], IW1, rnd_i)) >> (W_BITS - 5);
                const unsigned X0 = __builtin_amdgcn_perm(dv[j].y, dv[j].x, 0x05040100u);
                const unsigned X1 = __builtin_amdgcn_perm(dv[j + 1].y, dv[j + 1].x, 0x05040100u);
                const unsigned Y0 = __builtin_amdgcn_perm(dv[j].y, dv[j].x, 0x07060302u);
                const unsigned Y1 = __builtin_amdgcn_perm(dv[j + 1].y, dv[j + 1].x, 0x07060302u);
                const int gxr = sdot2(X0, GW0, sdot2_r(X1, GW1, rnd_d)) >> (W_BITS + kDerShift);
                const int gyr = sdot2(Y0, GW0, sdot2_r(Y1, GW1, rnd_d)) >> (W_BITS + kDerShift);
                if (S::FULL) {
                    gx[j] = gxr;
                    gy[j] = gyr;
                } else {
                    const int keep = -(int)(r0 + j < WH);
                    gx[j] = gxr & keep;
                    gy[j] = gyr & keep;
                }
            }
#pragma unroll
            for (int m = 0; m < NP; m++) {
                I2[m] = lo16x2(iv[2 * m], iv[2 * m + 1]);
                GX2[m] = lo16x2(gx[2 * m], gx[2 * m + 1]);
                GY2[m] = lo16x2(gy[2 * m], gy[2 * m + 1]);
                a11 = sdot2(GX2[m], GX2[m], a11);
                a12 = sdot2(GX2[m], GY2[m], a12);
                a22 = sdot2(GY2[m], GY2[m], a22);
            }
        }
        float A11, A12, A22;
        wave_sum_f3<S32>(a11, a12, a22, A11, A12, A22);

        float D = A11 * A22 - A12 * A12;
        float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * WW * WH);
        if (p.want_err && (p.flags & SVO_LK_GET_MIN_EIGENVALS)) errv = minEig;
        if (minEig < p.min_eig || D < FLT_EPSILON) {
            if (level == 0) st = 0;
            wave_lds_sync();
            continue;
        }
        D = 1.f / D;

        nextx -= halfWx;
        nexty -= halfWy;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < p.max_count; j++) {
            const SubPix np = sub_pixel(nextx, nexty);
            const int inx = uni_i(np.ix), iny = uni_i(np.iy);
            if (!(jsafe && (unsigned)(inx - jx0) <= 2u * JM && (unsigned)(iny - jy0) <= 2u * JM)) {
                if (!window_in_bounds(inx, iny, J.w, J.h, WW, WH)) {
                    if (level == 0) st = 0;
                    break;
                }
                follow_region<JM>(inx, iny, jx0, jy0, stage_next);
            }
            itcount++;
            const unsigned W0 = np.w.W0, W1 = np.w.W1;
            int b1 = 0, b2 = 0;
            {
                const unsigned* jp = jreg + (iny - jy0 + r0) * S::JRW + (inx - jxa + sc);
                unsigned q[RPG + 1];
#pragma unroll
                for (int k = 0; k <= RPG; k++) q[k] = jp[k * S::JRW];
                int jv[2 * NP];
#pragma unroll
                for (int k = 0; k < 2 * NP; k++)
                    jv[k] = k < RPG ? sdot2(q[k], W0, sdot2_r(q[k + 1], W1, rnd_i)) >> (W_BITS - 5) : 0;
#pragma unroll
                for (int m = 0; m < NP; m++) {
                    const unsigned d2 = pk_sub16(lo16x2(jv[2 * m], jv[2 * m + 1]), I2[m]);
                    b1 = sdot2(d2, GX2[m], b1);
                    b2 = sdot2(d2, GY2[m], b2);
                }
            }
            float fb1, fb2;
            wave_sum_f2<S32>(b1, b2, fb1, fb2);
            const float dx = (A12 * fb2 - A22 * fb1) * D;
            const float dy = (A12 * fb1 - A11 * fb2) * D;
            nextx += dx;
            nexty += dy;
            nx = nextx + halfWx;
            ny = nexty + halfWy;
            if (converged(dx, dy, p.eps2_lo, p.eps2_hi, p.eps2)) break;
            if (j > 0 && below_001(dx + pdx) && below_001(dy + pdy)) {
                nx -= dx * 0.5f;
                ny -= dy * 0.5f;
                break;
            }
            pdx = dx;
            pdy = dy;
        }

        if (st && p.want_err && level == 0 && !(p.flags & SVO_LK_GET_MIN_EIGENVALS)) {
            const bool in = sad_error<JM>(nx, ny, J.w, J.h, WW, WH, jx0, jy0, stage_next, [&](int x, int y, BiW w) {
                int sad = 0;
                const unsigned* jp = jreg + (y - jy0 + r0) * S::JRW + (x - jxa + sc);
#pragma unroll
                for (int k = 0; k < RPG; k++) {
                    const int jv = sdot2(jp[k * S::JRW], w.W0, sdot2_r(jp[(k + 1) * S::JRW], w.W1, rnd_i)) >>
                                   (W_BITS - 5);
                    const unsigned pr = I2[k >> 1];
                    const int iv = (k & 1) ? ((int)pr >> 16) : (int)(short)(pr & 0xFFFFu);
                    const int diff = jv - iv;
                    if (strip && (S::FULL || r0 + k < WH)) sad += diff < 0 ? -diff : diff;
                }
                return sad;
            }, errv);
            if (!in) {
                st = 0;
                continue;
            }
        }
        wave_lds_sync();
    }
    if (lane == 0) store_track(B, next_xy, base, pt, nx, ny, st, errv, itcount);
    }  // features of this wave
}

template <int WW, int WH>
hipError_t launch_fast(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st) {
    const int gn = b.grid_hint > 0 && b.grid_hint < max_n ? b.grid_hint : max_n;
    dim3 grid((gn + 3) / 4, nseq);
    constexpr int lds_bytes = 4 * Shape<WW, WH>::WAVE_BYTES;
    hipLaunchKernelGGL((lk_fast_kernel<WW, WH>), grid, dim3(256), lds_bytes, st, b, lk_dev(lp));
    return hipGetLastError();
}

}  // namespace

hipError_t launch_lk_fast(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st) {
    if (lp.win_w == 21 && lp.win_h == 21) return launch_fast<21, 21>(b, nseq, max_n, lp, st);
    if (lp.win_w == 11 && lp.win_h == 11) return launch_fast<11, 11>(b, nseq, max_n, lp, st);
    if (lp.win_w == 15 && lp.win_h == 15) return launch_fast<15, 15>(b, nseq, max_n, lp, st);
    if (lp.win_w == 31 && lp.win_h == 31) return launch_fast<31, 31>(b, nseq, max_n, lp, st);
    return hipErrorInvalidValue;
}

}  // namespace svo
