// Row SAD: the stereo match of a rectified pair as a bounded 1-D search along the
// left point's own row (svo_stereo_match_rows; the rule: include/svo_gpu.h and
// DESIGN.md section 3c). Integer costs throughout, so a numpy restatement pins
// every output bit for bit (tests/stereo_rows_reference.py).
//
// One wave per feature, a block of one wave (the barriers below are the wave's
// own). Per feature:
//   1. the right strip -- (2r+1) rows of the ncand + 2r bytes the search can touch
//      -- is staged into LDS with aligned dword loads (the level's kPyrPad border
//      covers the up to 7 + 3 bytes outside the image), the left patch beside it,
//      its rows cut to 2r+1 bytes by a dword mask and padded with zeros;
//   2. lane l costs the candidates l, l + 64, l + 128, l + 192 (candidate c is the
//      disparity dlo + c): per patch row, the window's 2r+1 bytes as up to four
//      dwords from five aligned LDS dwords (v_alignbyte_b32), the last one masked
//      like the left row (no branch per lane), and one v_sad_u8 per dword into
//      the running cost;
//   3. cost << 16 | c (cost <= 15 * 15 * 255 = 57375 fits 16 bits, c 8) reduced
//      with an unsigned minimum over the wave: the least cost, the lowest
//      disparity among equals; the second minimum (|c - c*| >= 2) the same way;
//   4. lane 0 applies the tests, the parabola and writes the outputs.
// No atomics: a run's outputs depend on its inputs alone.
//
// The guided entry (svo_stereo_match_rows_guided: a point searches its prior +-
// guide) adds stereo_rows_guided_kernel, four points per wave on 16-lane rows, the
// full-range body again for the points without a prior
// (stereo_rows_noprior_kernel), and row_priors_kernel (svo_stereo_row_priors);
// each has its comment below.
#include "common.hpp"

namespace svo {
namespace {

constexpr int kRowsMaxR = 7;
constexpr int kRowsMaxCand = 256;
// strip row: 3 (alignment) + 256 + 14 bytes = 69 dwords; the window's fifth
// dword may be one past the row's last staged one (read, never used)
constexpr int kStripDw = 70;
constexpr int kStripRows = 2 * kRowsMaxR + 1;

struct RowsShared {
    uint32_t strip[kStripRows * kStripDw + 2];
    uint32_t left[kStripRows * 4];
    int cost[kRowsMaxCand];
};

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}

// SKIP (the guided entry's second launch): the points that have a prior belong to
// stereo_rows_guided_kernel, and their waves leave at once.
template <bool SKIP>
__device__ __forceinline__ void rows_wave_body(const StereoRowsBatch& B, const svo_stereo_rows_params& P,
                                               const int* __restrict__ d_prior) {
    __shared__ RowsShared sh;
    const int lane = threadIdx.x;
    const int seq = blockIdx.y;
    const int n = B.counts ? B.counts[seq] : B.n;
    const size_t base = (size_t)seq * B.cap;
    const ImgLevel L = B.left[seq].lv[0];
    const ImgLevel R = B.right[seq].lv[0];
    const int w = L.w, h = L.h;
    const int r = P.radius;
    const int side = 2 * r + 1;
    const int nd = (side + 3) >> 2;  // dwords per patch row
    // the last dword's live bytes (side & 3 of them; side is odd, so 1 or 3)
    const uint32_t last_mask = (side & 3) == 1 ? 0xffu : 0xffffffu;

    // a wave per feature; a grid smaller than the count (grid_hint) loops
    for (int pt = blockIdx.x; pt < n; pt += gridDim.x) {
        if (SKIP && d_prior[base + pt] != SVO_STEREO_NO_PRIOR) continue;
        const float x = B.prev_xy[2 * (base + pt)], y = B.prev_xy[2 * (base + pt) + 1];
        // cvRound: round half to even; the range test on the rounded floats, so a
        // coordinate no int holds (NaN included) is outside
        const float rx = __builtin_rintf(x), ry = __builtin_rintf(y);
        const bool inside = rx >= 0.f && rx <= (float)(w - 1) && ry >= 0.f && ry <= (float)(h - 1);
        const int xi = inside ? (int)rx : 0, yi = inside ? (int)ry : 0;
        const int dlo = max(P.d_min, xi - (w - 1)), dhi = min(P.d_max, xi);
        const int ncand = dhi - dlo + 1;
        bool ok = inside && ncand >= 3;  // uniform over the wave
        int best_c = 0, c0 = 0;
        float delta = 0.f;
        if (ok) {
            // strip: columns [xi - dhi - r, xi - dlo + r] of rows yi - r .. yi + r,
            // from the aligned dword at or below its first byte
            const int col0 = xi - dhi - r;
            const uint8_t* rrow = R.data + (ptrdiff_t)(yi - r) * R.pitch + col0;
            const int mis = (int)((uintptr_t)rrow & 3);
            const int rowdw = (mis + ncand + 2 * r + 3) >> 2;  // <= 69
            rrow -= mis;
            for (int k = lane; k < side * rowdw; k += 64) {
                const int i = k / rowdw, j = k - i * rowdw;
                sh.strip[i * kStripDw + j] = *(const uint32_t*)(rrow + (ptrdiff_t)i * R.pitch + 4 * j);
            }
            // left patch: rows of 2r+1 bytes from (xi - r, yi - r), byte loads (its
            // column has no alignment to speak of, and it is 15 x 15 at the most)
            if (lane < side * nd) {
                const int i = lane / nd, q = lane - i * nd;
                const uint8_t* lp = L.data + (ptrdiff_t)(yi - r + i) * L.pitch + (xi - r + 4 * q);
                uint32_t v = 0;
                const int nb = min(4, side - 4 * q);
                for (int b = 0; b < nb; b++) v |= (uint32_t)lp[b] << (8 * b);
                sh.left[i * 4 + q] = v;
            }
            __syncthreads();
            uint32_t key = 0xffffffffu;
            for (int g = 0; g * 64 < ncand; g++) {
                const int c = lane + 64 * g;
                if (c < ncand) {
                    // the window of disparity dlo + c starts at column xi - (dlo + c) - r
                    const int s = mis + (dhi - dlo - c);
                    const int sdw = s >> 2;
                    const uint32_t sh8 = (uint32_t)(s & 3);
                    uint32_t acc = 0;
                    for (int i = 0; i < side; i++) {
                        const uint32_t* sr = sh.strip + i * kStripDw + sdw;
                        const uint32_t* lr = sh.left + i * 4;
                        uint32_t lo = sr[0];
                        for (int q = 0; q < nd; q++) {
                            const uint32_t hi = sr[q + 1];
                            uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, sh8);
                            v &= q == nd - 1 ? last_mask : 0xffffffffu;
                            acc = __builtin_amdgcn_sad_u8(v, lr[q], acc);
                            lo = hi;
                        }
                    }
                    sh.cost[c] = (int)acc;
                    const uint32_t kc = (acc << 16) | (uint32_t)c;
                    key = kc < key ? kc : key;
                }
            }
            key = wave_min_u32(key);
            best_c = (int)(key & 0xffffu);
            c0 = (int)(key >> 16);
            __syncthreads();
            // the runner-up: the least cost at two or more disparities from the best
            uint32_t sec = 0xffffffffu;
            for (int c = lane; c < ncand; c += 64) {
                const uint32_t v = (uint32_t)sh.cost[c];
                if ((c <= best_c - 2 || c >= best_c + 2) && v < sec) sec = v;
            }
            sec = wave_min_u32(sec);
            if (best_c == 0 || best_c == ncand - 1) ok = false;  // no bracket
            if (ok && P.max_cost > 0 && c0 > P.max_cost) ok = false;
            if (ok && P.uniq_pct > 0 && sec != 0xffffffffu &&
                !((uint32_t)c0 * 100u < (uint32_t)P.uniq_pct * sec))
                ok = false;
            if (ok) {
                const int cm = sh.cost[best_c - 1], cp = sh.cost[best_c + 1];
                const int den = cm + cp - 2 * c0;
                delta = den == 0 ? 0.f : __fdiv_rn((float)(cm - cp), (float)(2 * den));
            }
            __syncthreads();  // the next feature restages
        }
        if (lane == 0) {
            const int d = dlo + best_c;
            float xr = x;
            if (ok) {
                const float off = __fadd_rn((float)d, delta);
                xr = __fsub_rn(x, off);
            }
            B.next_xy[2 * (base + pt)] = xr;
            B.next_xy[2 * (base + pt) + 1] = y;
            B.status[base + pt] = ok ? 1 : 0;
            if (B.disparity) B.disparity[base + pt] = ok ? d : 0;
            if (B.cost) B.cost[base + pt] = ok ? c0 : 0;
        }
    }
}

__global__ __launch_bounds__(64) void stereo_rows_kernel(const StereoRowsBatch B, const svo_stereo_rows_params P) {
    rows_wave_body<false>(B, P, nullptr);
}

// the guided entry's points without a prior: the full range, a wave per point
__global__ __launch_bounds__(64) void stereo_rows_noprior_kernel(const StereoRowsBatch B, const svo_stereo_rows_params P,
                                                                 const int* __restrict__ d_prior) {
    rows_wave_body<true>(B, P, d_prior);
}

// Guided row SAD (svo_stereo_match_rows_guided): a point with a prior searches
// prior +- guide, at most 31 candidates, so a 16-lane row serves it and four points
// share a wave (a block of one wave; the barriers are the wave's own and stand
// outside every per-point branch). Per point the same steps as above on its own
// LDS slice: the strip is (2r+1) rows of at most 3 + 31 + 14 bytes = 12 dwords,
// lane l of the row costs the candidates l and l + 16, the keys are reduced over
// the row's 16 lanes, the row's first lane writes. Points without a prior are
// stereo_rows_noprior_kernel's.
constexpr int kGuideMax = 15;
constexpr int kGuidedCand = 2 * kGuideMax + 1;
constexpr int kGStripDw = 13;  // 12 staged dwords and the window's fifth (read, never used)

struct GuidedShared {
    uint32_t strip[kStripRows * kGStripDw + 3];
    uint32_t left[kStripRows * 4];
    int cost[kGuidedCand + 1];
};

__device__ __forceinline__ uint32_t row16_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 16);
        v = t < v ? t : v;
    }
    return v;
}

__global__ __launch_bounds__(64) void stereo_rows_guided_kernel(const StereoRowsBatch B, const svo_stereo_rows_params P,
                                                                const int* __restrict__ d_prior, const int guide) {
    __shared__ GuidedShared shg[4];
    const int grp = threadIdx.x >> 4, sl = threadIdx.x & 15;
    GuidedShared& sh = shg[grp];
    const int seq = blockIdx.y;
    const int n = B.counts ? B.counts[seq] : B.n;
    const size_t base = (size_t)seq * B.cap;
    const ImgLevel L = B.left[seq].lv[0];
    const ImgLevel R = B.right[seq].lv[0];
    const int w = L.w, h = L.h;
    const int r = P.radius;
    const int side = 2 * r + 1;
    const int nd = (side + 3) >> 2;
    const uint32_t last_mask = (side & 3) == 1 ? 0xffu : 0xffffffu;

    // four points per wave; the loop is the wave's, the point is the row's
    for (int pt0 = 4 * blockIdx.x; pt0 < n; pt0 += 4 * gridDim.x) {
        const int pt = pt0 + grp;
        const int prior = pt < n ? d_prior[base + pt] : SVO_STEREO_NO_PRIOR;
        const bool mine = prior != SVO_STEREO_NO_PRIOR;
        float x = 0.f, y = 0.f;
        if (mine) {
            x = B.prev_xy[2 * (base + pt)];
            y = B.prev_xy[2 * (base + pt) + 1];
        }
        const float rx = __builtin_rintf(x), ry = __builtin_rintf(y);
        const bool inside = mine && rx >= 0.f && rx <= (float)(w - 1) && ry >= 0.f && ry <= (float)(h - 1);
        const int xi = inside ? (int)rx : 0, yi = inside ? (int)ry : 0;
        // prior +- guide cut to the parameters' range: a prior clamped to [-64, 320]
        // gives the same intersection with [d_min, d_max] (inside [-16, 255]; guide
        // <= 15) as the prior itself, and cannot overflow
        const int pc = min(max(prior, -64), 320);
        const int glo = max(P.d_min, pc - guide), ghi = min(P.d_max, pc + guide);
        const int dlo = max(glo, xi - (w - 1)), dhi = min(ghi, xi);
        const int ncand = dhi - dlo + 1;  // <= 31
        bool ok = inside && ncand >= 3;   // uniform over the row
        int best_c = 0, c0 = 0;
        float delta = 0.f;
        int mis = 0;
        if (ok) {
            const int col0 = xi - dhi - r;
            const uint8_t* rrow = R.data + (ptrdiff_t)(yi - r) * R.pitch + col0;
            mis = (int)((uintptr_t)rrow & 3);
            const int rowdw = (mis + ncand + 2 * r + 3) >> 2;  // <= 12
            rrow -= mis;
            for (int k = sl; k < side * rowdw; k += 16) {
                const int i = k / rowdw, j = k - i * rowdw;
                sh.strip[i * kGStripDw + j] = *(const uint32_t*)(rrow + (ptrdiff_t)i * R.pitch + 4 * j);
            }
            for (int k = sl; k < side * nd; k += 16) {
                const int i = k / nd, q = k - i * nd;
                const uint8_t* lp = L.data + (ptrdiff_t)(yi - r + i) * L.pitch + (xi - r + 4 * q);
                uint32_t v = 0;
                const int nb = min(4, side - 4 * q);
                for (int b = 0; b < nb; b++) v |= (uint32_t)lp[b] << (8 * b);
                sh.left[i * 4 + q] = v;
            }
        }
        __syncthreads();
        uint32_t key = 0xffffffffu;
        if (ok) {
            for (int c = sl; c < ncand; c += 16) {
                const int s = mis + (dhi - dlo - c);
                const int sdw = s >> 2;
                const uint32_t sh8 = (uint32_t)(s & 3);
                uint32_t acc = 0;
                for (int i = 0; i < side; i++) {
                    const uint32_t* sr = sh.strip + i * kGStripDw + sdw;
                    const uint32_t* lr = sh.left + i * 4;
                    uint32_t lo = sr[0];
                    for (int q = 0; q < nd; q++) {
                        const uint32_t hi = sr[q + 1];
                        uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, sh8);
                        v &= q == nd - 1 ? last_mask : 0xffffffffu;
                        acc = __builtin_amdgcn_sad_u8(v, lr[q], acc);
                        lo = hi;
                    }
                }
                sh.cost[c] = (int)acc;
                const uint32_t kc = (acc << 16) | (uint32_t)c;
                key = kc < key ? kc : key;
            }
        }
        key = row16_min_u32(key);
        __syncthreads();
        uint32_t sec = 0xffffffffu;
        if (ok) {
            best_c = (int)(key & 0xffffu);
            c0 = (int)(key >> 16);
            for (int c = sl; c < ncand; c += 16) {
                const uint32_t v = (uint32_t)sh.cost[c];
                if ((c <= best_c - 2 || c >= best_c + 2) && v < sec) sec = v;
            }
        }
        sec = row16_min_u32(sec);
        if (ok) {
            if (best_c == 0 || best_c == ncand - 1) ok = false;  // no bracket: the prior was wrong
            if (ok && P.max_cost > 0 && c0 > P.max_cost) ok = false;
            if (ok && P.uniq_pct > 0 && sec != 0xffffffffu &&
                !((uint32_t)c0 * 100u < (uint32_t)P.uniq_pct * sec))
                ok = false;
            if (ok) {
                const int cm = sh.cost[best_c - 1], cp = sh.cost[best_c + 1];
                const int den = cm + cp - 2 * c0;
                delta = den == 0 ? 0.f : __fdiv_rn((float)(cm - cp), (float)(2 * den));
            }
        }
        __syncthreads();  // the next four points restage
        if (mine && sl == 0) {
            const int d = dlo + best_c;
            float xr = x;
            if (ok) {
                const float off = __fadd_rn((float)d, delta);
                xr = __fsub_rn(x, off);
            }
            B.next_xy[2 * (base + pt)] = xr;
            B.next_xy[2 * (base + pt) + 1] = y;
            B.status[base + pt] = ok ? 1 : 0;
            if (B.disparity) B.disparity[base + pt] = ok ? d : 0;
            if (B.cost) B.cost[base + pt] = ok ? c0 : 0;
        }
    }
}

// The prior of svo_stereo_row_priors: a thread per feature, its id looked up in
// the previous frame's sorted list.
__global__ __launch_bounds__(256) void row_priors_kernel(const RowPriorsBatch B) {
    const int s = blockIdx.y;
    int n = B.counts ? B.counts[s] : B.n;
    if (B.sub) n -= max(B.sub[s], 0);
    n = min(max(n, 0), B.cap);
    if (B.n_out && blockIdx.x == 0 && threadIdx.x == 0) B.n_out[s] = n;
    int pn = 0;
    if (B.prev_mid) {
        pn = B.prev_n ? B.prev_n[(size_t)s * B.prev_n_stride] : B.prev_n_host;
        if (B.prev_epoch && B.prev_epoch[(size_t)s * B.prev_n_stride] != B.cur_epoch[s]) pn = 0;
        pn = min(max(pn, 0), B.prev_cap);
    }
    const size_t base = (size_t)s * B.cap, pbase = (size_t)s * B.prev_stride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int id = B.mid[base + i];
        int lo = 0, hi = pn;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (B.prev_mid[pbase + m] < id)
                lo = m + 1;
            else
                hi = m;
        }
        int out = SVO_STEREO_NO_PRIOR;
        if (lo < pn && B.prev_mid[pbase + lo] == id) {
            const float ur = B.prev_ur[pbase + lo];
            if (ur >= 0.f) {
                const float d = __builtin_rintf(__fsub_rn(B.prev_xy[2 * (pbase + lo)], ur));
                if (d >= -32767.f && d <= 32767.f) out = (int)d;  // (a NaN fails both)
            }
        }
        B.d_prior[base + i] = out;
    }
}

}  // namespace

hipError_t launch_row_priors(const RowPriorsBatch& b, int nseq, int max_n, hipStream_t st) {
    if (nseq <= 0) return hipSuccess;
    const int gx = std::max(1, (std::min(std::max(max_n, 0), b.cap) + 255) / 256);
    hipLaunchKernelGGL(row_priors_kernel, dim3(gx, nseq), dim3(256), 0, st, b);
    return hipGetLastError();
}

bool stereo_rows_params_ok(const svo_stereo_rows_params& p) {
    if (p.radius < 1 || p.radius > kRowsMaxR) return false;
    if (p.d_min < -16 || p.d_max > 255) return false;
    const long span = (long)p.d_max - (long)p.d_min + 1;
    if (span < 3 || span > kRowsMaxCand) return false;
    if (p.uniq_pct < 0 || p.uniq_pct > 100 || p.max_cost < 0) return false;
    return true;
}

hipError_t launch_stereo_rows(const StereoRowsBatch& b, int nseq, int max_n, const svo_stereo_rows_params& p,
                              hipStream_t st) {
    if (!stereo_rows_params_ok(p)) return hipErrorInvalidValue;
    const int gn = b.grid_hint > 0 && b.grid_hint < max_n ? b.grid_hint : max_n;
    if (gn <= 0 || nseq <= 0) return hipSuccess;
    hipLaunchKernelGGL(stereo_rows_kernel, dim3(gn, nseq), dim3(64), 0, st, b, p);
    return hipGetLastError();
}

hipError_t launch_stereo_rows_guided(const StereoRowsBatch& b, int nseq, int max_n, const svo_stereo_rows_params& p,
                                     const int* d_prior, int guide, int full_grid, hipStream_t st) {
    if (!stereo_rows_params_ok(p) || !d_prior || guide < 1 || guide > kGuideMax) return hipErrorInvalidValue;
    if (max_n <= 0 || nseq <= 0) return hipSuccess;
    // two launches that each skip the other's points: four guided points per wave,
    // then the points without a prior, a wave each (waves loop over a smaller grid)
    hipLaunchKernelGGL(stereo_rows_guided_kernel, dim3((max_n + 3) / 4, nseq), dim3(64), 0, st, b, p, d_prior, guide);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int gf = full_grid > 0 && full_grid < max_n ? full_grid : max_n;
    hipLaunchKernelGGL(stereo_rows_noprior_kernel, dim3(gf, nseq), dim3(64), 0, st, b, p, d_prior);
    return hipGetLastError();
}

}  // namespace svo
