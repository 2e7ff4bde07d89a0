// lk_kernel: one wave64 per feature, any window lk_supported() admits, run-time
// window sizes (SVO_LK_GENERIC=1, or a window no specialised kernel covers). The
// lane map, staging and sampling are lk_strip.hpp's.
//  * The normal-equation sums are integer products; they are summed EXACTLY
//    (per-lane int32, wave sum by DPP on 16-bit halves, int64 total) and then
//    rounded to float once, so the result is order-independent and bit-exact
//    against the oracle's EXACT mode (OpenCV's own float accumulation order
//    differs only by rounding of the sums).
#include "lk_strip.hpp"

namespace svo {

namespace {

template <int RPG, bool FULL>
__global__ __launch_bounds__(256) void lk_kernel(LKBatch B, LKDev p) {
    static_assert((long long)RPG * 8160 * 4080 < (1ll << 31), "a lane's partial sums must fit int32");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int seq = blockIdx.y;
    const int n = B.counts ? B.counts[seq] : B.n;
    const int pt = lk_first(B, seq) + blockIdx.x * 4 + wid;
    if (pt >= n) return;
    const size_t base = (size_t)seq * B.cap;
    const float* __restrict__ prev_xy = B.prev_xy + 2 * base;
    float* __restrict__ next_xy = B.next_xy + 2 * base;
    const PyrDesc& prev = B.prev[seq];
    const PyrDesc& next = B.next[seq];
    const DerivDesc& dprev = B.dprev[seq];
    const StripLane m = strip_lane<RPG>(lane, p, lds + wid * p.lds_wave);

    const int win_w = p.win_w, win_h = p.win_h;
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
        const float A11 = (float)wave_sum_exact(a11) * FLT_SCALE;
        const float A12 = (float)wave_sum_exact(a12) * FLT_SCALE;
        const float A22 = (float)wave_sum_exact(a22) * FLT_SCALE;

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
            int b1 = 0, b2 = 0;
            const BiW jw = bilinear_weights(nextx - inx, nexty - iny);
            for_next_rows<RPG, FULL>(m, p, inx, iny, jx0, jy0, jw, [&](int k, int jv) {
                const int diff = jv - ival[k];
                b1 += diff * gix[k];
                b2 += diff * giy[k];
            });
            const float fb1 = (float)wave_sum_exact(b1) * FLT_SCALE;
            const float fb2 = (float)wave_sum_exact(b2) * FLT_SCALE;
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
            if (!strip_sad_error<RPG, FULL>(m, p, J, nx, ny, jx0, jy0, ival, errv)) {
                st = 0;
                continue;
            }
        }
        wave_lds_sync();  // this level's LDS reads finish before the next level's staging
    }
    if (lane == 0) store_track(B, next_xy, base, pt, nx, ny, st, errv, itcount);
}

template <int RPG>
hipError_t launch_rpg(const LKBatch& b, int nseq, int max_n, const LKDev& d, hipStream_t st) {
    dim3 grid((max_n + 3) / 4, nseq);
    if (d.groups * RPG == d.win_h)
        hipLaunchKernelGGL((lk_kernel<RPG, true>), grid, dim3(256), 4 * d.lds_wave, st, b, d);
    else
        hipLaunchKernelGGL((lk_kernel<RPG, false>), grid, dim3(256), 4 * d.lds_wave, st, b, d);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_lk_generic(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st) {
    const LKDev d = lk_dev(lp);
    const int rpg = (d.win_h + d.groups - 1) / d.groups;
#define SVO_LK_CASE(R) \
    case R: return launch_rpg<R>(b, nseq, max_n, d, st);
    switch (rpg) {
        SVO_LK_CASE(1) SVO_LK_CASE(2) SVO_LK_CASE(3) SVO_LK_CASE(4) SVO_LK_CASE(5) SVO_LK_CASE(6)
        SVO_LK_CASE(7) SVO_LK_CASE(8) SVO_LK_CASE(9) SVO_LK_CASE(10) SVO_LK_CASE(11) SVO_LK_CASE(12)
        SVO_LK_CASE(14) SVO_LK_CASE(16)
        default:
            break;
    }
#undef SVO_LK_CASE
    // uncommon strip heights: round up to the next instantiated size
    if (rpg <= 13) return launch_rpg<14>(b, nseq, max_n, d, st);
    if (rpg <= 16) return launch_rpg<16>(b, nseq, max_n, d, st);
    if (rpg <= 32) return launch_rpg<32>(b, nseq, max_n, d, st);
    // windows wider than 32 px: one strip per column, the window's height
    if (rpg <= 48) return launch_rpg<48>(b, nseq, max_n, d, st);
    return launch_rpg<64>(b, nseq, max_n, d, st);
}

}  // namespace svo
