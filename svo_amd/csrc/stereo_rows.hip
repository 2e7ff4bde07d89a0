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

__global__ __launch_bounds__(64) void stereo_rows_kernel(const StereoRowsBatch B, const svo_stereo_rows_params P) {
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

}  // namespace

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

}  // namespace svo
