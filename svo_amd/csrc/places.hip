// Kernels of the batched front end's place memory (places.hpp; the rules:
// DESIGN.md section 3e). The descriptor is section 3d's, by the device code the
// one-image kernels use (orb_device.hpp), over [sequence][feature] lists with one
// frame per sequence; the records are ordered compactions of the valid entries.
#include "orb_device.hpp"
#include "places.hpp"

namespace svo {

namespace {

// orb_blur_kernel's tile scheme with blockIdx.z as the sequence: level 0 of every
// frame into its own plane of `out`.
__global__ void __launch_bounds__(256) places_blur_kernel(const PyrDesc* __restrict__ frames, uint8_t* __restrict__ out,
                                                          size_t seq_stride, int pitch) {
    const ImgLevel L = frames[blockIdx.z].lv[0];
    const int x0 = blockIdx.x * kBlurTW, y0 = blockIdx.y * kBlurTH;
    if (x0 >= L.w || y0 >= L.h) return;  // block-uniform
    orb_blur_tile(L, x0, y0, out + (size_t)blockIdx.z * seq_stride, pitch);
}

// One wave per feature, grid (cap / 4, sequences): the level pixel and the validity
// test, orb_angle_kernel's moments and direction, orb_brief_kernel's 256 tests.
// Every lane holds the reduced moments, so every lane derives the same (c, s).
__global__ void __launch_bounds__(256) places_describe_kernel(
    const PyrDesc* __restrict__ frames, const uint8_t* __restrict__ blurred, size_t seq_stride, int pitch,
    const float2* __restrict__ xy, const int* __restrict__ n_p, int cap, int hp, OrbUmax um, int reach,
    const int8_t* __restrict__ pattern, unsigned long long* __restrict__ desc, uint8_t* __restrict__ valid) {
    __shared__ char2 s_pat[kOrbPatternPoints];
    reinterpret_cast<uint32_t*>(s_pat)[threadIdx.x] = reinterpret_cast<const uint32_t*>(pattern)[threadIdx.x];
    __syncthreads();
    const int s = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= min(n_p[s], cap)) return;  // wave-uniform
    const ImgLevel L = frames[s].lv[0];
    const size_t at = (size_t)s * cap + k;
    const float2 p = xy[at];
    const int cx = __float2int_rn(p.x), cy = __float2int_rn(p.y);  // cvRound at lscale 1 (NaN: 0, never valid)
    const bool ok = cx >= reach && cx <= L.w - 1 - reach && cy >= reach && cy <= L.h - 1 - reach;
    unsigned long long word = 0;  // lane r < 4 keeps the ballot of round r
    if (ok) {                     // wave-uniform
        int m10, m01;
        orb_moments(L, cx, cy, hp, um, lane, m10, m01);
        const OrbDirection d = orb_direction(m10, m01);
        const ImgLevel B{blurred + (size_t)s * seq_stride, L.w, L.h, pitch};
        word = orb_brief_words(B, cx, cy, d.c, d.s, s_pat, reach, lane);
    }
    if (lane < 4) desc[at * 4 + lane] = word;
    if (lane == 0) valid[at] = ok ? 1 : 0;
}

constexpr int kCompactThreads = 256;

// One block per sequence; the list goes by in chunks of 256, one entry per thread.
// A wave's ballot places its valid entries among the wave's, the waves' counts go
// through LDS, `base` carries the chunks before: list order is kept.
__global__ void __launch_bounds__(kCompactThreads) places_compact_kernel(PlacesCompact c) {
    __shared__ int s_wave[kCompactThreads / 64];
    const int s = blockIdx.x;
    const int n = min(c.n[s], c.cap);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t in0 = (size_t)s * c.cap, out0 = (size_t)s * c.out_stride;
    int base = 0;
    for (int k0 = 0; k0 < n; k0 += kCompactThreads) {  // block-uniform trip count
        const int k = k0 + threadIdx.x;
        const bool keep = k < n && c.valid[in0 + k] != 0;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int before = base, total = base;
        for (int w = 0; w < kCompactThreads / 64; w++) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (keep) {
            const int at = before + __popcll(b & ((1ull << lane) - 1));  // < n <= cap
            const size_t j = out0 + at;
            const uint4* src = reinterpret_cast<const uint4*>(c.desc + (in0 + k) * SVO_ORB_DESC_BYTES);
            uint4* dst = reinterpret_cast<uint4*>(c.desc_out + j * SVO_ORB_DESC_BYTES);
            dst[0] = src[0];
            dst[1] = src[1];
            reinterpret_cast<float2*>(c.xy_out)[j] = reinterpret_cast<const float2*>(c.xy)[in0 + k];
            if (c.mid) c.mid_out[in0 + at] = c.mid[in0 + k];
        }
        base = total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (threadIdx.x == 0) c.n_out[(size_t)s * c.n_stride] = base;
}

__global__ void __launch_bounds__(256) places_gather_xyz_kernel(const int* __restrict__ mid, int cap,
                                                                const int* __restrict__ n, int n_stride,
                                                                const double* __restrict__ map, int map_cap,
                                                                double* __restrict__ xyz_out, size_t out_stride) {
    const int s = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(n[(size_t)s * n_stride], cap)) return;
    const int id = mid[(size_t)s * cap + i];
    double* o = xyz_out + 3 * ((size_t)s * out_stride + i);
    if (id < 0 || id >= map_cap) {  // (never: the ids are the step's own)
        o[0] = o[1] = o[2] = 0.0;
        return;
    }
    const double* m = map + 3 * ((size_t)s * map_cap + id);
    o[0] = m[0];
    o[1] = m[1];
    o[2] = m[2];
}

__global__ void __launch_bounds__(256) places_gather_pairs_kernel(const int2* __restrict__ pairs,
                                                                  const int* __restrict__ n_pairs,
                                                                  const int* __restrict__ prob,
                                                                  const int* __restrict__ q_set,
                                                                  const int* __restrict__ rec_set, int cap,
                                                                  const float2* __restrict__ q_xy,
                                                                  const double* __restrict__ rec_xyz,
                                                                  double* __restrict__ obj, float2* __restrict__ img) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int p = prob[k];
    if (i >= min(n_pairs[p], cap)) return;
    const int2 qr = pairs[(size_t)p * cap + i];
    const size_t o = (size_t)k * cap + i;
    if (qr.x < 0 || qr.x >= cap || qr.y < 0 || qr.y >= cap) {  // (never: the filter's own pairs)
        obj[3 * o] = obj[3 * o + 1] = obj[3 * o + 2] = 0.0;
        img[o] = make_float2(0.f, 0.f);
        return;
    }
    const double* X = rec_xyz + 3 * ((size_t)rec_set[k] * cap + qr.y);
    obj[3 * o] = X[0];
    obj[3 * o + 1] = X[1];
    obj[3 * o + 2] = X[2];
    img[o] = q_xy[(size_t)q_set[k] * cap + qr.x];
}

}  // namespace

hipError_t launch_places_blur(const PyrDesc* frames, int nseq, int w, int h, uint8_t* out, size_t seq_stride,
                              int pitch, hipStream_t st) {
    if (nseq <= 0 || w <= 0 || h <= 0) return hipSuccess;
    dim3 grid((w + kBlurTW - 1) / kBlurTW, (h + kBlurTH - 1) / kBlurTH, nseq);
    hipLaunchKernelGGL(places_blur_kernel, grid, dim3(256), 0, st, frames, out, seq_stride, pitch);
    return hipGetLastError();
}

hipError_t launch_places_describe(const PyrDesc* frames, const uint8_t* blurred, size_t seq_stride, int pitch,
                                  const float* xy, const int* n, int cap, int nseq, int hp, const int* umax,
                                  int reach, const int8_t* pattern, uint8_t* desc, uint8_t* valid,
                                  hipStream_t st) {
    if (nseq <= 0 || cap <= 0) return hipSuccess;
    if (hp < 1 || hp > 15) return hipErrorInvalidValue;
    OrbUmax um{};
    for (int v = 0; v <= hp; v++) um.u[v] = umax[v];
    hipLaunchKernelGGL(places_describe_kernel, dim3((cap + 3) / 4, nseq), dim3(256), 0, st, frames, blurred,
                       seq_stride, pitch, reinterpret_cast<const float2*>(xy), n, cap, hp, um, reach, pattern,
                       reinterpret_cast<unsigned long long*>(desc), valid);
    return hipGetLastError();
}

hipError_t launch_places_compact(const PlacesCompact& c, int nseq, hipStream_t st) {
    if (nseq <= 0) return hipSuccess;
    hipLaunchKernelGGL(places_compact_kernel, dim3(nseq), dim3(kCompactThreads), 0, st, c);
    return hipGetLastError();
}

hipError_t launch_places_gather_xyz(const int* mid, int cap, const int* n, int n_stride, const double* map,
                                    int map_cap, double* xyz_out, size_t out_stride, int nseq, hipStream_t st) {
    if (nseq <= 0 || cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(places_gather_xyz_kernel, dim3((cap + 255) / 256, nseq), dim3(256), 0, st, mid, cap, n,
                       n_stride, map, map_cap, xyz_out, out_stride);
    return hipGetLastError();
}

hipError_t launch_places_gather_pairs(const int* pairs, const int* n_pairs, const int* prob, const int* q_set,
                                      const int* rec_set, int n_sel, int cap, const float* q_xy,
                                      const double* rec_xyz, double* obj, float* img, hipStream_t st) {
    if (n_sel <= 0 || cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(places_gather_pairs_kernel, dim3((cap + 255) / 256, n_sel), dim3(256), 0, st,
                       reinterpret_cast<const int2*>(pairs), n_pairs, prob, q_set, rec_set, cap,
                       reinterpret_cast<const float2*>(q_xy), rec_xyz, obj, reinterpret_cast<float2*>(img));
    return hipGetLastError();
}

}  // namespace svo
