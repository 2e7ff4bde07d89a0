// lk_multi_kernel: four features per wave, the kernel of the two product calls
// (temporal 21 x 21 with the min-eigenvalue error, stereo 11 x 11 without error).
// The shape and staging of the groups' next-image regions are lk_quad.hpp's.
#include "lk_quad.hpp"
#include "lk_strip_map.hpp"
#include "xcd_tile.hpp"

namespace svo {

namespace {

// high halves packed: floor(lo / 2^16) | floor(hi / 2^16) << 16, one v_perm
__device__ __forceinline__ unsigned hi16x2(int lo, int hi) {
    return __builtin_amdgcn_perm((unsigned)hi, (unsigned)lo, 0x07060302u);
}
__device__ __forceinline__ int swz16_add(int v) {  // + lane ^ 16 (within 32-lane groups)
    return v + __builtin_amdgcn_ds_swizzle(v, 0x401f);
}
// float of the exact h * 2^16 + l (one rounding: the product is exact), NOT scaled by
// FLT_SCALE -- the callers apply it (A) or fold it into 1 / det (b)
__device__ __forceinline__ float halves_lane_float(int h, int l) { return __builtin_fmaf((float)h, 65536.f, (float)l); }

// NR rows of one strip: I (x32) / Ix / Iy at the strip's pixels packed by row pairs
// (NR / 2 pairs), accumulated into the A sums and into per-lane c1 += I.Ix,
// c2 += I.Iy (sum (J - I) G = sum J G - sum I G exactly -- int32 wrap-around
// arithmetic, the per-lane total is the same bounded value -- so an iteration starts
// its b sums at (-c1, -c2) and needs no J - I subtraction). An odd NR leaves a last
// row: with ODD = false it is closed by a zero row (one more pair, half empty); with
// ODD = true its raw sums are returned (li, lx, ly) for odd_pair_setup, which pairs
// the last rows of two strips.
__device__ __forceinline__ void pair_setup(unsigned I2, unsigned GXm, unsigned GYm, int& a11, int& a12, int& a22,
                                           int& c1, int& c2) {
    a11 = sdot2(GXm, GXm, a11);
    a12 = sdot2(GXm, GYm, a12);
    a22 = sdot2(GYm, GYm, a22);
    c1 = sdot2(I2, GXm, c1);
    c2 = sdot2(I2, GYm, c2);
}
template <int NR, bool ODD>
__device__ __forceinline__ void strip_setup_c(const unsigned* P, const u32x2a4* D, unsigned IW0, unsigned IW1,
                                              unsigned GW0, unsigned GW1, unsigned* GX, unsigned* GY, int& a11,
                                              int& a12, int& a22, int& c1, int& c2, int& li, int& lx, int& ly) {
    constexpr int NP = ODD ? NR / 2 : (NR + 1) / 2;
    const int rnd_i = 1 << (W_BITS - 6), rnd_d = 1 << (W_BITS + kDerShift - 1);
    int iv[NR + 1], gx[NR + 1], gy[NR + 1];
    iv[NR] = gx[NR] = gy[NR] = 0;
#pragma unroll
    for (int j = 0; j < NR; j++) {
        iv[j] = sdot2(P[j], IW0, sdot2_r(P[j + 1], IW1, rnd_i)) >> (W_BITS - 5);
        const unsigned X0 = __builtin_amdgcn_perm(D[j].y, D[j].x, 0x05040100u);
        const unsigned X1 = __builtin_amdgcn_perm(D[j + 1].y, D[j + 1].x, 0x05040100u);
        const unsigned Y0 = __builtin_amdgcn_perm(D[j].y, D[j].x, 0x07060302u);
        const unsigned Y1 = __builtin_amdgcn_perm(D[j + 1].y, D[j + 1].x, 0x07060302u);
        gx[j] = sdot2(X0, GW0, sdot2_r(X1, GW1, rnd_d));  // CV_DESCALE(., W_BITS) in bits 16..31
        gy[j] = sdot2(Y0, GW0, sdot2_r(Y1, GW1, rnd_d));
    }
    static_assert(W_BITS + kDerShift == 16, "derivative sums must carry their descaled value in bits 16..31");
#pragma unroll
    for (int m = 0; m < NP; m++) {
        GX[m] = hi16x2(gx[2 * m], gx[2 * m + 1]);
        GY[m] = hi16x2(gy[2 * m], gy[2 * m + 1]);
        pair_setup(lo16x2(iv[2 * m], iv[2 * m + 1]), GX[m], GY[m], a11, a12, a22, c1, c2);
    }
    if constexpr (ODD) {
        li = iv[NR - 1];
        lx = gx[NR - 1];
        ly = gy[NR - 1];
    }
}
// the last rows of strips k (i0 ..) and k + 1 (i1 ..) as one pair
__device__ __forceinline__ void odd_pair_setup(int i0, int x0, int y0, int i1, int x1, int y1, unsigned& GXm,
                                               unsigned& GYm, int& a11, int& a12, int& a22, int& c1, int& c2) {
    GXm = hi16x2(x0, x1);
    GYm = hi16x2(y0, y1);
    pair_setup(lo16x2(i0, i1), GXm, GYm, a11, a12, a22, c1, c2);
}

// Exact sums over the LPF lanes of each group (every lane receives its group's
// total), as floats of the exact integers (one rounding): int32 DPP steps while
// the partial sums provably fit (STEPS32), then 16-bit halves.
template <int LPF, int STEPS32>
__device__ __forceinline__ int group_add_step(int v, int step) {
    switch (step) {
        case 0: return dpp_row_add<0xb1>(v);   // quad_perm 1,0,3,2
        case 1: return dpp_row_add<0x4e>(v);   // quad_perm 2,3,0,1
        case 2: return dpp_row_add<0x124>(v);  // row_ror:4
        case 3: return dpp_row_add<0x128>(v);  // row_ror:8
        default: return swz16_add(v);          // lane ^ 16
    }
}
template <int LPF, int STEPS32, int NV>
__device__ __forceinline__ void group_sum_f(int (&v)[NV], float (&f)[NV]) {
    constexpr int STEPS = LPF == 16 ? 4 : 5;
    static_assert(LPF == 16 || LPF == 32, "groups of 16 or 32 lanes");
#pragma unroll
    for (int s = 0; s < STEPS32; s++)
#pragma unroll
        for (int i = 0; i < NV; i++) v[i] = group_add_step<LPF, STEPS32>(v[i], s);
    int h[NV], lo[NV];
#pragma unroll
    for (int i = 0; i < NV; i++) {
        h[i] = v[i] >> 16;
        lo[i] = v[i] & 0xFFFF;
    }
#pragma unroll
    for (int s = STEPS32; s < STEPS; s++)
#pragma unroll
        for (int i = 0; i < NV; i++) {
            h[i] = group_add_step<LPF, STEPS32>(h[i], s);
            lo[i] = group_add_step<LPF, STEPS32>(lo[i], s);
        }
#pragma unroll
    for (int i = 0; i < NV; i++) f[i] = halves_lane_float(h[i], lo[i]);
}
// the same group reduction stopped before the float: every lane receives its group's
// exact total as 16-bit-half sums (h, lo), total = h 2^16 + lo
template <int LPF, int STEPS32>
__device__ __forceinline__ void group_halves(int v, int& h, int& lo) {
    constexpr int STEPS = LPF == 16 ? 4 : 5;
#pragma unroll
    for (int s = 0; s < STEPS32; s++) v = group_add_step<LPF, STEPS32>(v, s);
    h = v >> 16;
    lo = v & 0xFFFF;
#pragma unroll
    for (int s = STEPS32; s < STEPS; s++) {
        h = group_add_step<LPF, STEPS32>(h, s);
        lo = group_add_step<LPF, STEPS32>(lo, s);
    }
}
// exact 64-lane totals of two int32 partials (|v| < 2^31 / 8 per lane) as half sums in
// scalars: three int32 DPP steps (8-lane partials), then the halves
__device__ __forceinline__ void wave_halves2(int x, int y, int& xh, int& xl, int& yh, int& yl) {
    x = dpp_add<0xb1, 0xf, true>(x);
    y = dpp_add<0xb1, 0xf, true>(y);
    x = dpp_add<0x4e, 0xf, true>(x);
    y = dpp_add<0x4e, 0xf, true>(y);
    x = dpp_add<0x114, 0xf, true>(x);
    y = dpp_add<0x114, 0xf, true>(y);
    int ah = x >> 16, al = x & 0xFFFF, bh = y >> 16, bl = y & 0xFFFF;
    ah = dpp_add<0x118, 0xf, true>(ah);
    al = dpp_add<0x118, 0xf, true>(al);
    bh = dpp_add<0x118, 0xf, true>(bh);
    bl = dpp_add<0x118, 0xf, true>(bl);
    ah = dpp_add<0x142, 0xa, false>(ah);
    al = dpp_add<0x142, 0xa, false>(al);
    bh = dpp_add<0x142, 0xa, false>(bh);
    bl = dpp_add<0x142, 0xa, false>(bl);
    ah = dpp_add<0x143, 0xc, false>(ah);
    al = dpp_add<0x143, 0xc, false>(al);
    bh = dpp_add<0x143, 0xc, false>(bh);
    bl = dpp_add<0x143, 0xc, false>(bl);
    xh = __builtin_amdgcn_readlane(ah, 63);
    xl = __builtin_amdgcn_readlane(al, 63);
    yh = __builtin_amdgcn_readlane(bh, 63);
    yl = __builtin_amdgcn_readlane(bl, 63);
}
__device__ __forceinline__ float rl_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// LOOP (the stereo call): the grid covers LKBatch::grid_hint features per sequence
// (the expected count) and a block whose sequence holds more takes the tiles
// gridDim.x, 2 gridDim.x, ... further on; without it (the temporal call) a block
// owns one tile and blocks past a sequence's count return at once. The stereo
// call's bound is the feature budget (~2,100 per sequence) while the speculative
// count is ~100: sized to the bound, 131k of its 134k waves per launch only read a
// count and exited, dispatched beside LK.
template <int FPW, int QJM, int MINW, int KKS = 2, int WW = 21, int WH = 21, int NR = 7, bool LOOP = false>
__global__ __launch_bounds__(64, MINW) void lk_multi_kernel(LKBatch B, LKDev p) {
    using Q = MultiShape<QJM, WW, WH, FPW>;
    static_assert(WH % NR == 0, "whole strips");
    static_assert(WW + QJM + 3 <= kPyrPad && WW + 1 <= kDerPad, "padding too small for the window");
    constexpr int JRW = Q::JRW, JRH = Q::JRH;
    constexpr int NSTRIP = WW * (WH / NR);
    constexpr int LPF = 64 / FPW;                 // lanes per feature
    constexpr int K = (NSTRIP + LPF - 1) / LPF;   // strips per lane
    using SM = StripMap<WW, WH / NR, LPF>;        // which strips (lk_strip_map.hpp)
    static_assert(SM::K == K && SM::valid(), "strip map");
    // triples: a lane's strips 0, 1, 2 from one dword (4 prev pixels) and one 16-byte
    // load (4 derivative records) per row, its strip 3 loaded as a single strip
    constexpr bool TRI = SM::TRIPLES;
    static_assert(!TRI || K == 4, "a triple and a single per lane");
    // A prev window starts at x in [-WW, w), y in [-WH, h) (window_in_bounds). A
    // strip at column c reads pixels and records c, c + 1 of rows y .. y + WH; a
    // triple's wide loads at column c <= WW - 3 read c .. c + 3, the columns its
    // three strips read one by one -- under either map columns x .. x + WW and no
    // further (SM::valid(): every strip a window column), inside the padded levels:
    static_assert(WW + 1 <= kPyrPad && WH + 1 <= kPyrPad && WW + 1 <= kDerPad && WH + 1 <= kDerPad,
                  "padding too small for the prev window's loads");
    // an odd strip height pairs the last rows of strips 2i and 2i + 1 (ODD; K even),
    // otherwise the last row is closed by a zero row
    constexpr bool ODD = NR % 2 == 1 && K % 2 == 0;
    constexpr int NP = ODD ? NR / 2 : (NR + 1) / 2;  // full row pairs per strip
    constexpr int NO = ODD ? K / 2 : 1;              // odd-row pairs per lane
    // int32 partial sums: a lane holds <= NR K products |diff * g| <= 8160 * 4080
    // (A sums: 4080^2); steps while 2^steps * NR K * 8160 * 4080 < 2^31
    constexpr long long kProd = (long long)NR * K * 8160 * 4080;
    constexpr int STEPS32 = 4 * kProd < (1ll << 31) ? 2 : 2 * kProd < (1ll << 31) ? 1 : 0;
    static_assert(kProd < (1ll << 31), "a lane's partial sums must fit int32");
    // the single-group tail (below): the 21 x 21 temporal shape, four strips per lane
    constexpr bool TAIL = !LOOP && FPW == 4 && K == 4 && ODD && NP == 3 && NO == 2;
    // a tail lane's b partial: NP full row pairs + one odd pair, 8160 * 4080 each
    static_assert(!TAIL || 8ll * (2 * NP + 2) * 8160 * 4080 < (1ll << 31), "tail partials: 3 int32 DPP steps");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63;
    const int g = lane / LPF, l = lane % LPF;
    // in XCD order the blocks one XCD runs are consecutive features of one sequence
    // (neighbouring windows: shared L2 lines) instead of every 8th block
    const XcdTile tile = xcd_tile();
    const int seq = tile.y;
    const int n = B.counts ? B.counts[seq] : B.n;
    const int first = lk_first(B, seq);
    int tx = tile.x;
next_tile:  // (LOOP: the block's next tile, gridDim.x further on)
    const int pt0 = first + tx * FPW;
    if (pt0 >= n) return;
    const int pt = pt0 + g;
    const bool live = pt < n;
    const int ptc = live ? pt : n - 1;  // an idle group shadows a real feature, writes nothing
    const size_t base = (size_t)seq * B.cap;
    const float* __restrict__ prev_xy = B.prev_xy + 2 * base;
    float* __restrict__ next_xy = B.next_xy + 2 * base;
    const cpyr prev = (cpyr)B.prev + seq;
    const cpyr next = (cpyr)B.next + seq;
    const DerivDesc& dprev = B.dprev[seq];
    unsigned* jregs = reinterpret_cast<unsigned*>(lds);
    const unsigned* jmine = jregs + g * (Q::JSTRIDE / 4);
    const StageGeom<JRW, JRH> sg(lane);

    // the lane's strips: column, first row; dummy slots carry zero weights
    int scol[K], srow[K];
    bool sreal[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const Strip s = SM::at(l, k);
        sreal[k] = s.real;
        scol[k] = s.col;
        srow[k] = s.band * NR;
    }
    constexpr float halfWx = (WW - 1) * 0.5f, halfWy = (WH - 1) * 0.5f;
    const int rnd_j = 1 << (W_BITS - 6 + kJShift);

    const float px = prev_xy[2 * ptc], py = prev_xy[2 * ptc + 1];
    float nx = 0.f, ny = 0.f;
    if (p.flags & SVO_LK_USE_INITIAL_FLOW) {
        nx = next_xy[2 * ptc];
        ny = next_xy[2 * ptc + 1];
    }
    int st = live ? 1 : 0;
    float errv = 0.f;
    // iterations per feature, counted from the active-lane ballot: wave-uniform, so
    // scalar registers (a per-lane counter is the first VGPR spilled under MINW = 4)
    int itc[FPW];
#pragma unroll
    for (int f = 0; f < FPW; f++) itc[f] = 0;
    const int max_level = p.max_level;

    for (int level = max_level; level >= 0; level--) {
        const ImgLevel I{prev->lv[level].data, prev->lv[level].w, prev->lv[level].h, prev->lv[level].pitch};
        const ImgLevel J{next->lv[level].data, next->lv[level].w, next->lv[level].h, next->lv[level].pitch};
        const LevelStart start = level_start(px, py, nx, ny, level, max_level, p.flags, I.w, I.h, WW, WH);
        float nextx = start.nextx, nexty = start.nexty;
        nx = nextx;
        ny = nexty;
        const int ipx = start.ipx, ipy = start.ipy;
        const bool inb = start.inb;
        if (!inb && level == 0 && live) {
            st = 0;
            errv = 0.f;
        }
        bool lact = live && inb;
        const BiW iw = bilinear_weights(start.a, start.b);
        const unsigned IW0 = iw.W0, IW1 = iw.W1;

        int jx0 = ufloor(nextx - halfWx) - QJM, jy0 = ufloor(nexty - halfWy) - QJM;
        int jxa = jx0 & ~3;
        int jbase = jy0 * JRW + jxa;  // the region origin as an entry offset (iny * JRW + inx - jbase)
        unsigned GX[K][NP], GY[K][NP], GXO[NO], GYO[NO];
        int li[K], lx[K], ly[K];  // (ODD) the strips' last rows until paired
        int asum[3] = {0, 0, 0};
        int csum[2] = {0, 0};  // sum I.Ix, I.Iy over the lane's strips
        {
            // branch-free reads (padded levels); an inactive group (or one whose
            // region lies beyond the padding: its first bounds test deactivates
            // it) stages and reads at the level origin, results unused
            using SL = StageGeom<JRW, JRH>;
            int xs[FPW], ys[FPW];
#pragma unroll
            for (int f = 0; f < FPW; f++) {
                const int xa = __builtin_amdgcn_readlane(jxa, LPF * f), y0 = __builtin_amdgcn_readlane(jy0, LPF * f);
                const bool ok = __builtin_amdgcn_readlane((int)lact, LPF * f) && region_in_pad<JRW, JRH>(J, xa, y0);
                xs[f] = ok ? xa : 0;
                ys[f] = ok ? y0 : 0;
            }
            unsigned sv[FPW][SL::NPS];
            // wave-uniform row bases (scalar adds) + one per-lane offset for every
            // feature: 4d + (the lane's pass-0 row) * pitch; the last pass's rows are
            // clamped to the region (per lane)
            const gu8 jbase = pad_origin(J.data, J.pitch, kPyrPad, 1) + (size_t)kPyrPad * (J.pitch + 1);
            const unsigned ol = 4u * (unsigned)sg.d + (unsigned)sg.row(0) * (unsigned)J.pitch;
            const unsigned olast = 4u * (unsigned)sg.d + (unsigned)sg.row(SL::NPS - 1) * (unsigned)J.pitch;
#pragma unroll
            for (int f = 0; f < FPW; f++) {
                const gu8 fb = jbase + xs[f] + (ptrdiff_t)ys[f] * J.pitch;
#pragma unroll
                for (int q = 0; q < SL::NPS; q++)
                    sv[f][q] = q + 1 < SL::NPS ? ldg_off<unsigned>(fb + (size_t)q * SL::RPP * J.pitch, ol)
                                               : ldg_off<unsigned>(fb, olast);
            }
            const int dpitch = dprev.pitch[level];
            const gu8 ibase = pad_origin(I.data, I.pitch, kPyrPad, 1);
            const gu8 dbase = pad_origin((const uint8_t*)dprev.data[level], dpitch, kDerPad, 4);
            const int sx = inb ? ipx : 0, sy = inb ? ipy : 0;
            const auto write_staging = [&] {
#pragma unroll
                for (int f = 0; f < FPW; f++)
#pragma unroll
                    for (int q = 0; q < SL::NPS; q++) sg.write(jregs + f * (Q::JSTRIDE / 4), sg.row(q), sv[f][q]);
            };
            const auto load_strip = [&](int k, unsigned* P, u32x2a4* Dv) {
                // per-lane offsets of the strip's first row; the rows by wave-uniform bases
                const int x = sx + scol[k], y = sy + srow[k];
                const unsigned oi = (unsigned)(x + kPyrPad) + (unsigned)(y + kPyrPad) * (unsigned)I.pitch;
                const unsigned od = 4u * ((unsigned)(x + kDerPad) + (unsigned)(y + kDerPad) * (unsigned)dpitch);
#pragma unroll
                for (int r = 0; r <= NR; r++) {
                    P[r] = __builtin_amdgcn_perm(0u, (unsigned)ldg_off<u16a1>(ibase + (size_t)r * I.pitch, oi),
                                                 0x0c010c00u);
                    Dv[r] = ldg_off<u32x2a4>(dbase + (size_t)r * 4 * dpitch, od);
                }
            };
            const auto setup_strip = [&](int k, const unsigned* P, const u32x2a4* Dv) {
                strip_setup_c<NR, ODD>(P, Dv, IW0, IW1, sreal[k] ? IW0 : 0u, sreal[k] ? IW1 : 0u, GX[k], GY[k], asum[0],
                                       asum[1], asum[2], csum[0], csum[1], li[k], lx[k], ly[k]);
                if (ODD && (k & 1))
                    odd_pair_setup(li[k - 1], lx[k - 1], ly[k - 1], li[k], lx[k], ly[k], GXO[k / 2], GYO[k / 2],
                                   asum[0], asum[1], asum[2], csum[0], csum[1]);
            };
            if constexpr (TRI) {
                // the rows of strips 0, 1, 2 (columns c, c + 1, c + 2) in one dword -- pixels
                // c .. c + 3, at any byte address -- and one 16-byte load -- records c .. c + 3
                // -- each; the single strip 3's narrow loads go out once strips 0 and 1
                // have freed their registers
                unsigned M[NR + 1];
                u32x4a4 Dm[NR + 1];
                {
                    const int x = sx + scol[0], y = sy + srow[0];
                    const unsigned oi = (unsigned)(x + kPyrPad) + (unsigned)(y + kPyrPad) * (unsigned)I.pitch;
                    const unsigned od = 4u * ((unsigned)(x + kDerPad) + (unsigned)(y + kDerPad) * (unsigned)dpitch);
#pragma unroll
                    for (int r = 0; r <= NR; r++) {
                        M[r] = ldg_off<u32a1>(ibase + (size_t)r * I.pitch, oi);
                        Dm[r] = ldg_off<u32x4a4>(dbase + (size_t)r * 4 * dpitch, od);
                    }
                }
                write_staging();
                unsigned P[NR + 1], Ps[NR + 1];
                u32x2a4 Dv[NR + 1], Ds[NR + 1];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    if (k == 2) load_strip(3, Ps, Ds);
#pragma unroll
                    for (int r = 0; r <= NR; r++) {
                        P[r] = __builtin_amdgcn_perm(0u, M[r], k == 0 ? 0x0c010c00u : k == 1 ? 0x0c020c01u : 0x0c030c02u);
                        Dv[r] = k == 0   ? u32x2a4{Dm[r].x, Dm[r].y}
                                : k == 1 ? u32x2a4{Dm[r].y, Dm[r].z}
                                         : u32x2a4{Dm[r].z, Dm[r].w};
                    }
                    setup_strip(k, P, Dv);
                }
                setup_strip(3, Ps, Ds);
            } else {
                // strips KKS at a time: loads of a group in flight together
                static_assert(KKS >= 1, "strips loaded per setup group");
#pragma unroll
                for (int k0 = 0; k0 < K; k0 += KKS) {
                    constexpr int KK = K >= KKS ? KKS : 1;
                    unsigned P[KK][NR + 1];
                    u32x2a4 Dv[KK][NR + 1];
#pragma unroll
                    for (int kk = 0; kk < KK; kk++) load_strip(k0 + kk, P[kk], Dv[kk]);
                    if (k0 == 0) write_staging();
#pragma unroll
                    for (int kk = 0; kk < KK; kk++) setup_strip(k0 + kk, P[kk], Dv[kk]);
                }
            }
        }
        wave_lds_sync();
        float A[3];
        group_sum_f<LPF, STEPS32>(asum, A);
        const float A11 = A[0] * FLT_SCALE, A12 = A[1] * FLT_SCALE, A22 = A[2] * FLT_SCALE;

        float D = A11 * A22 - A12 * A12;
        const float minEig =
            (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * WW * WH);
        if (lact && p.want_err && (p.flags & SVO_LK_GET_MIN_EIGENVALS)) errv = minEig;
        if (lact && (minEig < p.min_eig || D < FLT_EPSILON)) {
            if (level == 0) st = 0;
            lact = false;
        }
        D = 1.f / D;
        // the b sums arrive unscaled: (A12 b2 s - A22 b1 s) D == (A12 b2 - A22 b1) (s D)
        // exactly for s = FLT_SCALE (a power of two commutes with every rounding here)
        const float Ds = D * FLT_SCALE;

        nextx -= halfWx;
        nexty -= halfWy;
        float pdx = 0.f, pdy = 0.f;
        int tail_j = -1;
        for (int j = 0; j < p.max_count; j++) {
            const unsigned long long act0 = __builtin_amdgcn_ballot_w64(lact);
            if (act0 == 0) break;
            if constexpr (TAIL) {
                // one feature left: its iterations go to all 64 lanes (below)
                const unsigned long long gm = act0 & 0x0001000100010001ull;
                if ((gm & (gm - 1)) == 0) {
                    tail_j = j;
                    break;
                }
            }
            const float fnx = __builtin_floorf(nextx), fny = __builtin_floorf(nexty);
            const int inx = (int)fnx, iny = (int)fny;
            if (lact && !window_in_bounds(inx, iny, J.w, J.h, WW, WH)) {
                if (level == 0) st = 0;
                lact = false;
            }
            const bool need = lact && ((unsigned)(inx - jx0) > 2u * QJM || (unsigned)(iny - jy0) > 2u * QJM);
            unsigned long long nb = __builtin_amdgcn_ballot_w64(need && l == 0);
            if (nb) {  // (rare: the region's origin moves only inside this branch)
                if (need) {
                    jx0 = inx - QJM;
                    jy0 = iny - QJM;
                    jxa = jx0 & ~3;
                    jbase = jy0 * JRW + jxa;
                }
                wave_lds_sync();
                while (nb) {
                    const int f = (int)(__builtin_ctzll(nb) / LPF);
                    nb &= nb - 1;
                    stage_padded<JRW, JRH>(jregs + f * (Q::JSTRIDE / 4), J,
                                           __builtin_amdgcn_readlane(jxa, LPF * f),
                                           __builtin_amdgcn_readlane(jy0, LPF * f), sg);
                }
                wave_lds_sync();
            }
            {
                const unsigned long long act = __builtin_amdgcn_ballot_w64(lact);
#pragma unroll
                for (int f = 0; f < FPW; f++) itc[f] += (int)((act >> (LPF * f)) & 1ull);
            }
            const BiW w = bilinear_weights(nextx - fnx, nexty - fny);
            const unsigned W0 = w.W0, W1 = w.W1;
            int bsum[2] = {-csum[0], -csum[1]};
            {
                // (iny - jy0) JRW + (inx - jxa) as one 24-bit multiply-add against the
                // region origin's offset; an inactive group reads inside its own region
                // (results unused)
                const int off = lact ? __mul24(iny, JRW) + inx - jbase : 0;
                const unsigned* jb = jmine + off;
                int jlast = 0;  // (ODD) the even strip's last row
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const unsigned* js = jb + srow[k] * JRW + scol[k];
                    unsigned q[NR + 1];
#pragma unroll
                    for (int r = 0; r <= NR; r++) q[r] = js[r * JRW];
                    int jv[NR + 1];
                    jv[NR] = 0;
#pragma unroll
                    for (int r = 0; r < NR; r++)  // J x 2^kJShift: descaled value in bits 16..31
                        jv[r] = sdot2(q[r], W0, sdot2_r(q[r + 1], W1, rnd_j));
#pragma unroll
                    for (int m = 0; m < NP; m++) {
                        const unsigned jj = hi16x2(jv[2 * m], jv[2 * m + 1]);  // J; the I part is in csum
                        bsum[0] = sdot2(jj, GX[k][m], bsum[0]);
                        bsum[1] = sdot2(jj, GY[k][m], bsum[1]);
                    }
                    if constexpr (ODD) {
                        if (k & 1) {
                            const unsigned jj = hi16x2(jlast, jv[NR - 1]);
                            bsum[0] = sdot2(jj, GXO[k / 2], bsum[0]);
                            bsum[1] = sdot2(jj, GYO[k / 2], bsum[1]);
                        } else {
                            jlast = jv[NR - 1];
                        }
                    }
                }
            }
            float fb[2];
            group_sum_f<LPF, STEPS32>(bsum, fb);
            // materialised here, ahead of the lane-divergent update below: sunk into
            // it, the last DPP step splits into v_mov_dpp + a separate add per value
            asm volatile("" : "+v"(fb[0]), "+v"(fb[1]));
            const float fb1 = fb[0], fb2 = fb[1];
            const float dx = (A12 * fb2 - A22 * fb1) * Ds;
            const float dy = (A12 * fb1 - A11 * fb2) * Ds;
            if (lact) {
                nextx += dx;
                nexty += dy;
                nx = nextx + halfWx;
                ny = nexty + halfWy;
                if (converged(dx, dy, p.eps2_lo, p.eps2_hi, p.eps2)) {
                    lact = false;
                } else if (j > 0 && below_001(dx + pdx) && below_001(dy + pdy)) {
                    nx -= dx * 0.5f;
                    ny -= dy * 0.5f;
                    lact = false;
                } else {
                    pdx = dx;
                    pdy = dy;
                }
            }
        }
        if constexpr (TAIL) {
            if (tail_j >= 0) {
                // The single-group tail. One feature (group fs) is still iterating and
                // the wave's other groups are done with this level, so its iterations
                // run on all 64 lanes, one strip per lane instead of four: lane t takes
                // strip (l, k) = ((t >> 1) & 15, 2 (t >> 5) + (t & 1)) of the group's map
                // -- strips 2i and 2i + 1 of a group lane on neighbouring lanes, so the
                // odd-row pair that joins their last rows is one DPP move away. The
                // feature's G pairs move to LDS once (the region of a finished group:
                // it is not read again this level), its state to scalars. The b sums
                // stay exact integers: sum J G over the 64 lanes as 16-bit halves minus
                // the group's sum I G (its csum lanes, halves), rounded to float once
                // -- the same float as the group path, whatever the distribution.
                const int fs = (int)(__builtin_ctzll(__builtin_amdgcn_ballot_w64(lact)) / LPF);
                const int ls = fs * LPF;
                unsigned* const gst = jregs + ((fs + 1) & (FPW - 1)) * (Q::JSTRIDE / 4);
                unsigned* const jstar = jregs + fs * (Q::JSTRIDE / 4);
                if (g == fs) {
#pragma unroll
                    for (int k = 0; k < K; k++) {
                        const int t = ((k >> 1) << 5) | (l << 1) | (k & 1);
                        const unsigned ox = (k & 1) ? GXO[k >> 1] : 0u, oy = (k & 1) ? GYO[k >> 1] : 0u;
                        *reinterpret_cast<uint4*>(gst + 8 * t) = uint4{GX[k][0], GX[k][1], GX[k][2], GY[k][0]};
                        *reinterpret_cast<uint4*>(gst + 8 * t + 4) = uint4{GY[k][1], GY[k][2], ox, oy};
                    }
                }
                int ch0, cl0, ch1, cl1;
                group_halves<LPF, STEPS32>(csum[0], ch0, cl0);
                group_halves<LPF, STEPS32>(csum[1], ch1, cl1);
                ch0 = __builtin_amdgcn_readlane(ch0, ls);
                cl0 = __builtin_amdgcn_readlane(cl0, ls);
                ch1 = __builtin_amdgcn_readlane(ch1, ls);
                cl1 = __builtin_amdgcn_readlane(cl1, ls);
                wave_lds_sync();
                const uint4 ga = *reinterpret_cast<const uint4*>(gst + 8 * lane);
                const uint4 gb = *reinterpret_cast<const uint4*>(gst + 8 * lane + 4);
                const unsigned TX[NP] = {ga.x, ga.y, ga.z}, TY[NP] = {ga.w, gb.x, gb.y};
                const unsigned TXO = gb.z, TYO = gb.w;
                int soff;
                {
                    const Strip s = SM::at((lane >> 1) & (LPF - 1), ((lane >> 5) << 1) | (lane & 1));
                    soff = s.band * NR * JRW + s.col;
                }
                float tnx = rl_f(nextx, ls), tny = rl_f(nexty, ls), tpdx = rl_f(pdx, ls), tpdy = rl_f(pdy, ls);
                float tox = rl_f(nx, ls), toy = rl_f(ny, ls);
                const float tA11 = rl_f(A11, ls), tA12 = rl_f(A12, ls), tA22 = rl_f(A22, ls), tDs = rl_f(Ds, ls);
                int tjx0 = __builtin_amdgcn_readlane(jx0, ls), tjy0 = __builtin_amdgcn_readlane(jy0, ls);
                int tjbase = __builtin_amdgcn_readlane(jbase, ls);
                int tst = __builtin_amdgcn_readlane(st, ls);
                int titc = 0;
                for (int j = tail_j; j < p.max_count; j++) {
                    const float fnx = __builtin_floorf(tnx), fny = __builtin_floorf(tny);
                    const int inx = (int)fnx, iny = (int)fny;
                    if (!window_in_bounds(inx, iny, J.w, J.h, WW, WH)) {
                        if (level == 0) tst = 0;
                        break;
                    }
                    if ((unsigned)(inx - tjx0) > 2u * QJM || (unsigned)(iny - tjy0) > 2u * QJM) {
                        tjx0 = inx - QJM;
                        tjy0 = iny - QJM;
                        tjbase = tjy0 * JRW + (tjx0 & ~3);
                        wave_lds_sync();
                        stage_padded<JRW, JRH>(jstar, J, tjx0 & ~3, tjy0, sg);
                        wave_lds_sync();
                    }
                    titc++;
                    const BiW w = bilinear_weights(tnx - fnx, tny - fny);
                    const unsigned* js = jstar + (__mul24(iny, JRW) + inx - tjbase) + soff;
                    unsigned q[NR + 1];
#pragma unroll
                    for (int r = 0; r <= NR; r++) q[r] = js[r * JRW];
                    int jv[NR];
#pragma unroll
                    for (int r = 0; r < NR; r++) jv[r] = sdot2(q[r], w.W0, sdot2_r(q[r + 1], w.W1, rnd_j));
                    int b0 = 0, b1 = 0;
#pragma unroll
                    for (int m = 0; m < NP; m++) {
                        const unsigned jj = hi16x2(jv[2 * m], jv[2 * m + 1]);
                        b0 = sdot2(jj, TX[m], b0);
                        b1 = sdot2(jj, TY[m], b1);
                    }
                    {
                        // the even strip's last row from the neighbouring lane (quad_perm
                        // 1,0,3,2); even lanes hold zero odd-pair G
                        const int jp = __builtin_amdgcn_update_dpp(0, jv[NR - 1], 0xb1, 0xf, 0xf, true);
                        const unsigned jj = hi16x2(jp, jv[NR - 1]);
                        b0 = sdot2(jj, TXO, b0);
                        b1 = sdot2(jj, TYO, b1);
                    }
                    int h0, l0, h1, l1;
                    wave_halves2(b0, b1, h0, l0, h1, l1);
                    const float fb1 = __builtin_fmaf((float)(h0 - ch0), 65536.f, (float)(l0 - cl0));
                    const float fb2 = __builtin_fmaf((float)(h1 - ch1), 65536.f, (float)(l1 - cl1));
                    const float dx = (tA12 * fb2 - tA22 * fb1) * tDs;
                    const float dy = (tA12 * fb1 - tA11 * fb2) * tDs;
                    tnx += dx;
                    tny += dy;
                    tox = tnx + halfWx;
                    toy = tny + halfWy;
                    if (converged(dx, dy, p.eps2_lo, p.eps2_hi, p.eps2)) break;
                    if (j > 0 && below_001(dx + tpdx) && below_001(dy + tpdy)) {
                        tox -= dx * 0.5f;
                        toy -= dy * 0.5f;
                        break;
                    }
                    tpdx = dx;
                    tpdy = dy;
                }
                if (g == fs) {
                    nx = tox;
                    ny = toy;
                    st = tst;
                }
#pragma unroll
                for (int f = 0; f < FPW; f++) itc[f] += f == fs ? titc : 0;
            }
        }
        wave_lds_sync();
    }
    if (l == 0 && live) {
        next_xy[2 * pt] = nx;
        next_xy[2 * pt + 1] = ny;
        B.status[base + pt] = (uint8_t)st;
        if (B.err) B.err[base + pt] = errv;
        if (B.iters) {
            int itcount = itc[0];
#pragma unroll
            for (int f = 1; f < FPW; f++) itcount = g == f ? itc[f] : itcount;
            B.iters[base + pt] = itcount;
        }
    }
    if constexpr (LOOP) {
        tx += gridDim.x;
        goto next_tile;
    }
}

template <int FPW, int QJM, int MINW, int KKS, int WW, int WH, int NR, bool LOOP>
hipError_t launch_multi(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st) {
    const int gn = LOOP && b.grid_hint > 0 && b.grid_hint < max_n ? b.grid_hint : max_n;
    dim3 grid((gn + FPW - 1) / FPW, nseq);
    constexpr int lds_bytes = FPW * MultiShape<QJM, WW, WH, FPW>::JSTRIDE;
    hipLaunchKernelGGL((lk_multi_kernel<FPW, QJM, MINW, KKS, WW, WH, NR, LOOP>), grid, dim3(64), lds_bytes, st, b,
                       lk_dev(lp));
    return hipGetLastError();
}

}  // namespace

// four features per wave, 1-px staging margin (re-staged when the
// estimate leaves it; measured 2.7 % faster alone than a 2-px margin
// and than 3 px; two features per wave (lk_dual_kernel, another lane
// map) measured slower and is gone; 4 waves/SIMD, 8 features per wave
// and one strip ahead in the setup measured slower: DESIGN.md section 5).
// Launch bound 3 waves per SIMD (the kernel compiles to 122 VGPRs and runs 4).
// The level setup was bound by the texture addresser, which a load costs the same
// at any width and with any lanes active: a lane's strips 0, 1, 2 are three neighbouring columns read by one
// dword and one 16-byte load per row, strip 3 a single column (lk_strip_map.hpp;
// KKS, the strips per load group of the dealt map, is unused by it) -- 32 strip
// loads per level and wave where the dealt map issued 64
// (profiles/lk_pair_loads.txt).
hipError_t launch_lk_multi_temporal(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st) {
    return launch_multi<4, 1, 3, 2, 21, 21, 7, false>(b, nseq, max_n, lp, st);
}

// the stereo call's 11 x 11 (findLeftFeaturesInRight, no err): four
// features per wave too, one 11-row strip per lane (11 of 16 lanes). Capped
// at 80 VGPRs (6 waves per SIMD; a few spills in the per-tile / per-level
// code, none in the trip loop) so its waves fit beside the temporal kernel's three
// per SIMD: +1.7 % frames/s over 91 VGPRs
// (profiles/r06/e_setprio_stereo_minw_ab.txt)
hipError_t launch_lk_multi_stereo(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st) {
    return launch_multi<4, 1, 6, 1, 11, 11, 11, true>(b, nseq, max_n, lp, st);
}

}  // namespace svo
