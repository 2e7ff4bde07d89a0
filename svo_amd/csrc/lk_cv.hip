// lk_cv_kernel: OpenCV's own float accumulation order (SVO_LK_OPENCV_ORDER), one
// feature per wave, any window: the normal equations summed exactly as
// LKTrackerInvoker's SSE build sums them (lkpyramid.cpp, the CV_SIMD128 paths;
// oracle/lk.c:109-157, 186-238 ACC_SSE):
//  * A11 / A12 / A22: four float lanes over the columns x < se4 (lane x & 3,
//    rows in order, columns in order within a row), a scalar float chain over
//    the rest (row by row), then sA + ((q0 + q2) + (q1 + q3));
//  * b1 / b2 per iteration: four float lanes per sum over x < se8, each adding
//    float(d[x] G[x] + d[x+4] G[x+4]) for the 8-column blocks in order
//    (x & 3 = lane), a scalar chain over the rest, then
//    sb + ((c0 + c2 + 0) + (c1 + c3 + 0)).
// Every term is an integer, so a float chain equals the exact integer sum
// whenever the sum of the |terms| of the whole window stays <= 2^24 (every
// partial sum, and every combination of them, is then an exactly representable
// integer): the wave computes that bound beside the exact sums and runs the
// ordered float chains (one lane per chain, the terms staged in LDS in chain
// order) only when the bound fails. One feature per wave, the strip lane map,
// staging and sampling of lk_kernel (lk_strip.hpp); all else (solve, exits, err) as
// lk_kernel.
// The chains' term layout in LDS (per quantity, n = win_w * win_h ints):
//   A (3 quantities): lane k < 4 at k*win_h*M4 + y*M4 + m (x = 4m + k),
//                     scalar at 4*win_h*M4 + y*(win_w - se4) + (x - se4);
//   b (2 quantities): lane t < 4 at t*win_h*2*B8 + y*2*B8 + 2*blk + h
//                     (x = 8blk + t + 4h), scalar at win_h*se8 + y*(win_w - se8) + (x - se8).
#include "lk_strip.hpp"

namespace svo {

namespace {

struct CvOrder {
    int se4, se8;    // OpenCV's SIMD column ends: 4-wide covariance, 8-wide b loop
    int term_off;    // byte offset of the chain terms in the wave's LDS
};

__device__ __forceinline__ float lane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
constexpr int kExact24 = 1 << 24;

template <int RPG, bool FULL>
__global__ __launch_bounds__(64) void lk_cv_kernel(LKBatch B, LKDev p, CvOrder co) {
    static_assert((long long)RPG * 8160 * 4080 < (1ll << 31), "a lane's partial sums must fit int32");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x;
    const int seq = blockIdx.y;
    const int n = B.counts ? B.counts[seq] : B.n;
    const int pt = lk_first(B, seq) + blockIdx.x;
    if (pt >= n) return;
    const size_t base = (size_t)seq * B.cap;
    const float* __restrict__ prev_xy = B.prev_xy + 2 * base;
    float* __restrict__ next_xy = B.next_xy + 2 * base;
    const PyrDesc& prev = B.prev[seq];
    const PyrDesc& next = B.next[seq];
    const DerivDesc& dprev = B.dprev[seq];
    const StripLane m = strip_lane<RPG>(lane, p, lds);
    int* terms = reinterpret_cast<int*>(lds + co.term_off);

    const int win_w = p.win_w, win_h = p.win_h;
    const int npx = win_w * win_h;
    const int sc = m.sc, r0 = m.r0;
    const bool strip = m.strip;

    // this lane's column in the chain layouts (slot of row y = base + y * stride)
    const int se4 = co.se4, se8 = co.se8, M4 = se4 >> 2, B8 = se8 >> 3;
    int a_base, a_stride, b_base, b_stride;
    if (sc < se4) {
        a_base = (sc & 3) * win_h * M4 + (sc >> 2);
        a_stride = M4;
    } else {
        a_base = 4 * win_h * M4 + (sc - se4);
        a_stride = win_w - se4;
    }
    if (sc < se8) {
        b_base = (sc & 3) * win_h * 2 * B8 + 2 * (sc >> 3) + ((sc >> 2) & 1);
        b_stride = 2 * B8;
    } else {
        b_base = win_h * se8 + (sc - se8);
        b_stride = win_w - se8;
    }
    // chain lanes: A: lane = 5q + k (q: A11, A12, A22; k < 4 SIMD lane, 4 scalar);
    // b: lane = 5q + k (q: b1, b2)
    const int cq = lane / 5, ck = lane - 5 * (lane / 5);
    const int a_len = ck < 4 ? win_h * M4 : win_h * (win_w - se4);
    const int* a_src = terms + cq * npx + (ck < 4 ? ck * win_h * M4 : 4 * win_h * M4);
    const int b_len = ck < 4 ? win_h * B8 : win_h * (win_w - se8);
    const int* b_src = terms + cq * npx + (ck < 4 ? ck * win_h * 2 * B8 : win_h * se8);

    const float halfWx = (win_w - 1) * 0.5f, halfWy = (win_h - 1) * 0.5f;
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
        const ImgLevel I = prev.lv[level];
        const ImgLevel J = next.lv[level];
        const LevelStart start = level_start(px, py, nx, ny, level, max_level, p.flags, I.w, I.h, win_w, win_h);
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
        int jx0 = uni_i(ufloor(nextx - halfWx)) - JM, jy0 = uni_i(ufloor(nexty - halfWy)) - JM;
        const StripSamples<RPG> w = strip_setup<RPG, FULL>(m, p, I, J, dprev, level, ipx, ipy, jx0, jy0,
                                                           bilinear_weights(start.a, start.b));
        const auto& ival = w.ival;
        const auto& gix = w.gix;
        const auto& giy = w.giy;
        const int a11 = w.a11, a12 = w.a12, a22 = w.a22;
        const double e11 = wave_sum_exact(a11), e12 = wave_sum_exact(a12), e22 = wave_sum_exact(a22);
        float A11, A12, A22;
        // sum |Ix Iy| <= (sum Ix^2 + sum Iy^2) / 2: every chain exact under these bounds
        if (e11 <= kExact24 && e22 <= kExact24 && e11 + e22 <= 2.0 * kExact24) {
            A11 = (float)e11 * FLT_SCALE;
            A12 = (float)e12 * FLT_SCALE;
            A22 = (float)e22 * FLT_SCALE;
        } else {
            if (strip) {
#pragma unroll
                for (int j = 0; j < RPG; j++) {
                    if (FULL || r0 + j < win_h) {
                        const int s = a_base + (r0 + j) * a_stride;
                        terms[s] = gix[j] * gix[j];
                        terms[npx + s] = gix[j] * giy[j];
                        terms[2 * npx + s] = giy[j] * giy[j];
                    }
                }
            }
            wave_lds_sync();
            float acc = 0.f;
            if (lane < 15)
                for (int i = 0; i < a_len; i++) acc += (float)a_src[i];
            wave_lds_sync();
            A11 = (lane_f(acc, 4) + ((lane_f(acc, 0) + lane_f(acc, 2)) + (lane_f(acc, 1) + lane_f(acc, 3)))) *
                  FLT_SCALE;
            A12 = (lane_f(acc, 9) + ((lane_f(acc, 5) + lane_f(acc, 7)) + (lane_f(acc, 6) + lane_f(acc, 8)))) *
                  FLT_SCALE;
            A22 = (lane_f(acc, 14) + ((lane_f(acc, 10) + lane_f(acc, 12)) + (lane_f(acc, 11) + lane_f(acc, 13)))) *
                  FLT_SCALE;
        }

        float D = A11 * A22 - A12 * A12;
        float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) /
                       (float)(2 * win_w * win_h);
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
            const int inx = uni_i(ufloor(nextx)), iny = uni_i(ufloor(nexty));
            if (!window_in_bounds(inx, iny, J.w, J.h, win_w, win_h)) {
                if (level == 0) st = 0;
                break;
            }
            itcount++;
            follow_region<JM>(inx, iny, jx0, jy0, [&] { stage_next(m, p, J, jx0, jy0); });
            int b1 = 0, b2 = 0, babs = 0;
            int pb1[RPG], pb2[RPG];
#pragma unroll
            for (int k = 0; k < RPG; k++) pb1[k] = pb2[k] = 0;
            const BiW jw = bilinear_weights(nextx - inx, nexty - iny);
            for_next_rows<RPG, FULL>(m, p, inx, iny, jx0, jy0, jw, [&](int k, int jv) {
                const int diff = jv - ival[k];
                pb1[k] = diff * gix[k];
                pb2[k] = diff * giy[k];
                b1 += pb1[k];
                b2 += pb2[k];
                // |terms| <= 8160 * 4080 < 2^25: capped per lane so 64 lanes cannot overflow
                babs = min(babs + abs(pb1[k]) + abs(pb2[k]), kExact24 + 1);
            });
            float fb1, fb2;
            if (dpp_sum(babs) <= kExact24) {
                fb1 = (float)wave_sum_exact(b1) * FLT_SCALE;
                fb2 = (float)wave_sum_exact(b2) * FLT_SCALE;
            } else {
                if (strip) {
#pragma unroll
                    for (int k = 0; k < RPG; k++) {
                        if (FULL || r0 + k < win_h) {
                            const int s = b_base + (r0 + k) * b_stride;
                            terms[s] = pb1[k];
                            terms[npx + s] = pb2[k];
                        }
                    }
                }
                wave_lds_sync();
                float acc = 0.f;
                // (two loops: the SIMD-lane chains add a pair per term, the scalar
                // chain single terms; one loop with a per-term branch on the step cost
                // ~10 instructions per term and ran max(len) times for both kinds)
                if (lane < 10) {
                    if (ck < 4) {
#pragma unroll 6
                        for (int i = 0; i < b_len; i++) acc += (float)(b_src[2 * i] + b_src[2 * i + 1]);
                    } else {
#pragma unroll 8
                        for (int i = 0; i < b_len; i++) acc += (float)b_src[i];
                    }
                }
                wave_lds_sync();
                fb1 = (lane_f(acc, 4) + (((lane_f(acc, 0) + lane_f(acc, 2)) + 0.f) +
                                         ((lane_f(acc, 1) + lane_f(acc, 3)) + 0.f))) * FLT_SCALE;
                fb2 = (lane_f(acc, 9) + (((lane_f(acc, 5) + lane_f(acc, 7)) + 0.f) +
                                         ((lane_f(acc, 6) + lane_f(acc, 8)) + 0.f))) * FLT_SCALE;
            }
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
            pdx = uni_f(dx);  // (wave-uniform: kept in scalar registers)
            pdy = uni_f(dy);
        }

        if (st && p.want_err && level == 0 && !(p.flags & SVO_LK_GET_MIN_EIGENVALS)) {
            // SAD: sum |diff| <= 2048 * 8160 < 2^24, exact in any order
            if (!strip_sad_error<RPG, FULL>(m, p, J, nx, ny, jx0, jy0, ival, errv)) {
                st = 0;
                continue;
            }
        }
        wave_lds_sync();
    }
    if (lane == 0) store_track(B, next_xy, base, pt, nx, ny, st, errv, itcount);
}

template <int RPG>
hipError_t launch_cv_rpg(const LKBatch& b, int nseq, int max_n, const LKDev& d, hipStream_t st) {
    CvOrder co;
    co.se4 = d.win_w >= 4 ? ((d.win_w - 4) / 4 + 1) * 4 : 0;
    co.se8 = d.win_w >= 8 ? ((d.win_w - 8) / 8 + 1) * 8 : 0;
    co.term_off = (d.lds_wave + 15) & ~15;
    const int lds = co.term_off + 3 * d.win_w * d.win_h * 4;
    dim3 grid(max_n, nseq);
    if (d.groups * RPG == d.win_h)
        hipLaunchKernelGGL((lk_cv_kernel<RPG, true>), grid, dim3(64), lds, st, b, d, co);
    else
        hipLaunchKernelGGL((lk_cv_kernel<RPG, false>), grid, dim3(64), lds, st, b, d, co);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_lk_cv(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st) {
    const LKDev d = lk_dev(lp);
    const int rpg = (d.win_h + d.groups - 1) / d.groups;
#define SVO_LK_CV_CASE(R) \
    case R: return launch_cv_rpg<R>(b, nseq, max_n, d, st);
    switch (rpg) {
        SVO_LK_CV_CASE(1) SVO_LK_CV_CASE(2) SVO_LK_CV_CASE(3) SVO_LK_CV_CASE(4) SVO_LK_CV_CASE(5)
        SVO_LK_CV_CASE(6) SVO_LK_CV_CASE(7) SVO_LK_CV_CASE(8) SVO_LK_CV_CASE(11) SVO_LK_CV_CASE(16)
        default:
            break;
    }
#undef SVO_LK_CV_CASE
    if (rpg <= 16) return launch_cv_rpg<16>(b, nseq, max_n, d, st);
    if (rpg <= 32) return launch_cv_rpg<32>(b, nseq, max_n, d, st);
    if (rpg <= 48) return launch_cv_rpg<48>(b, nseq, max_n, d, st);
    return launch_cv_rpg<64>(b, nseq, max_n, d, st);
}

}  // namespace svo
