// svo_match_projected on the device (the rules: DESIGN.md section 3f;
// include/svo_gpu.h): where ORBmatcher::SearchByProjection would stand in a port.
// Three kernels: the frame's keypoints binned into a cell grid, every map point
// projected and matched inside its window, the bids resolved into pairs. Every
// result is a minimum over keys (distance << 20 | index), so it depends neither
// on the cell size, nor on the order inside a cell, nor on the launch shape.
#include "match_projected.hpp"

#include <hip/hip_runtime.h>

#include "block_compact.hpp"

namespace svo {

namespace {

constexpr int kProjThreads = 256;

// The cell of a keypoint, or -1 for one that is not usable (outside the frame, NaN).
__device__ __forceinline__ int proj_cell(float2 k, float wf, float hf, const ProjGrid& g) {
    if (!(k.x >= 0.f && k.x < wf && k.y >= 0.f && k.y < hf)) return -1;
    // (min: a width above 2^24 can round up as a float)
    return min((int)k.y >> g.shift, g.gh - 1) * g.gw + min((int)k.x >> g.shift, g.gw - 1);
}

// One block per problem. Pass 1 counts the usable keypoints per cell in LDS and
// clears the claim words; the counts are scanned (a thread sums a run of cells,
// the 256 sums are scanned by doubling); pass 2 places every keypoint's index at
// its cell's cursor. LDS integer atomics: the order inside a cell is free.
__global__ void __launch_bounds__(kProjThreads) proj_bin_kernel(ProjMatch m) {
    __shared__ int s_cnt[kProjMaxCells];
    __shared__ int s_part[kProjThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int ks = m.k_set ? m.k_set[p] : p;
    const int nk = max(min(m.n_kp[ks], m.k_stride), 0);  // (never past a set's rows)
    const float2* kp = reinterpret_cast<const float2*>(m.kxy) + (size_t)ks * m.k_stride;
    const int ncell = m.grid.cells();  // <= kProjMaxCells
    const float wf = (float)m.w, hf = (float)m.h;
    int* cs = m.scr.cell_start + (size_t)p * (ncell + 1);
    int* sorted = m.scr.sorted + (size_t)p * m.k_stride;
    uint32_t* claim = m.scr.claim + (size_t)p * m.k_stride;
    for (int c = tid; c < ncell; c += kProjThreads) s_cnt[c] = 0;
    __syncthreads();
    for (int j = tid; j < nk; j += kProjThreads) {
        claim[j] = kProjNoKey;
        const int c = proj_cell(kp[j], wf, hf, m.grid);
        if (c >= 0) atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    const int per = (ncell + kProjThreads - 1) / kProjThreads, c0 = tid * per;
    int sum = 0;
    for (int k = 0; k < per; k++)
        if (c0 + k < ncell) sum += s_cnt[c0 + k];
    s_part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kProjThreads; off <<= 1) {
        const int v = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int run = s_part[tid] - sum;
    for (int k = 0; k < per; k++)
        if (c0 + k < ncell) {
            const int cnt = s_cnt[c0 + k];
            cs[c0 + k] = run;
            s_cnt[c0 + k] = run;  // the cell's cursor
            run += cnt;
        }
    if (tid == kProjThreads - 1) cs[ncell] = s_part[tid];
    __syncthreads();
    for (int j = tid; j < nk; j += kProjThreads) {
        const int c = proj_cell(kp[j], wf, hf, m.grid);
        if (c >= 0) sorted[atomicAdd(&s_cnt[c], 1)] = j;  // < the usable count <= nk <= k_stride
    }
}

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// grid (point tiles, problems), kLanes lanes per point (1, or 16: a quarter wave):
// the projection in f64, the cells the window touches row by row (a row's cells
// are one run of the sorted list, which the point's lanes stride over), the window
// test in f32 on the keypoint itself, the two smallest keys (merged across the
// point's lanes by shuffles: minima of distinct keys, so the split changes
// nothing), the outputs, and the bid: an atomicMin of (distance << 20 | point) on
// the keypoint's claim word. The points of a wave are neighbours in the list, not
// in the image: their walks diverge, and the outputs stay in list order.
template <int kLanes>
__global__ void __launch_bounds__(kProjThreads) proj_match_kernel(ProjMatch m) {
    const int p = blockIdx.y;
    const int ps = m.p_set ? m.p_set[p] : p, ks = m.k_set ? m.k_set[p] : p;
    const int np = min(m.n_pts[ps], m.p_stride);
    const int sub = threadIdx.x % kLanes;
    const int i = blockIdx.x * (kProjThreads / kLanes) + threadIdx.x / kLanes;
    if (i >= np) return;  // (no barrier below; the lanes of a point leave together)
    const double* T = m.poses + 12 * (size_t)p;
    const double* X = m.xyz + 3 * ((size_t)ps * m.p_stride + i);
    const double x = X[0], y = X[1], z = X[2];
    const double px = T[0] * x + T[1] * y + T[2] * z + T[9];
    const double py = T[3] * x + T[4] * y + T[5] * z + T[10];
    const double pz = T[6] * x + T[7] * y + T[8] * z + T[11];
    const bool front = pz > 0;
    const double iz = 1.0 / pz;
    const double u = m.fx * (px * iz) + m.cx, v = m.fy * (py * iz) + m.cy;
    const float uf = (float)u, vf = (float)v;
    const bool visible = front && uf >= 0.f && uf < (float)m.w && vf >= 0.f && vf < (float)m.h;
    uint32_t k1 = kProjNoKey, k2 = kProjNoKey;
    if (visible) {
        const float r = m.radius;
        // The cells that can hold a candidate: the window's pixels, widened by more
        // than the rounding of kx - uf in f32, in f64 and cut to the frame first.
        const double mg = 1.0 + (double)r * 1.2e-7;
        const double xm = (double)(m.w - 1), ym = (double)(m.h - 1);
        const int cx0 = (int)fmin(fmax(floor((double)uf - r - mg), 0.0), xm) >> m.grid.shift;
        const int cx1 = (int)fmin(fmax(floor((double)uf + r + mg), 0.0), xm) >> m.grid.shift;
        const int cy0 = (int)fmin(fmax(floor((double)vf - r - mg), 0.0), ym) >> m.grid.shift;
        const int cy1 = (int)fmin(fmax(floor((double)vf + r + mg), 0.0), ym) >> m.grid.shift;
        const int ncell = m.grid.cells();
        const int* cs = m.scr.cell_start + (size_t)p * (ncell + 1);
        const int* sorted = m.scr.sorted + (size_t)p * m.k_stride;
        const float2* kp = reinterpret_cast<const float2*>(m.kxy) + (size_t)ks * m.k_stride;
        const uint4* kd = reinterpret_cast<const uint4*>(m.kdesc) + 2 * (size_t)ks * m.k_stride;
        const uint4* pd = reinterpret_cast<const uint4*>(m.pdesc) + 2 * ((size_t)ps * m.p_stride + i);
        const uint4 a0 = pd[0], a1 = pd[1];
        for (int cy = cy0; cy <= cy1; cy++) {
            const int e1 = cs[cy * m.grid.gw + cx1 + 1];  // (<= cs[ncell]: the usable count)
            for (int e = cs[cy * m.grid.gw + cx0] + sub; e < e1; e += kLanes) {
                const int j = sorted[e];
                const float2 k = kp[j];
                if (!(fabsf(k.x - uf) <= r && fabsf(k.y - vf) <= r)) continue;
                const uint32_t key = ((uint32_t)hamming256(a0, a1, kd[2 * (size_t)j], kd[2 * (size_t)j + 1]) << 20) |
                                     (uint32_t)j;
                if (key < k1) {
                    k2 = k1;
                    k1 = key;
                } else if (key < k2) {
                    k2 = key;
                }
            }
        }
    }
    for (int off = kLanes / 2; off > 0; off >>= 1) {  // (every lane of the point is here, visible or not)
        const uint32_t o1 = (uint32_t)__shfl_xor((int)k1, off, kLanes), o2 = (uint32_t)__shfl_xor((int)k2, off, kLanes);
        k2 = min(max(k1, o1), min(k2, o2));
        k1 = min(k1, o1);
    }
    if (sub != 0) return;
    const int j1 = k1 == kProjNoKey ? -1 : (int)(k1 & (kProjMaxStride - 1));
    const int j2 = k2 == kProjNoKey ? -1 : (int)(k2 & (kProjMaxStride - 1));
    const int d1 = k1 == kProjNoKey ? 257 : (int)(k1 >> 20), d2 = k2 == kProjNoKey ? 257 : (int)(k2 >> 20);
    const size_t o = (size_t)p * m.p_stride + i;
    if (m.idx) reinterpret_cast<int2*>(m.idx)[o] = make_int2(j1, j2);
    if (m.dist) reinterpret_cast<int2*>(m.dist)[o] = make_int2(d1, d2);
    if (m.proj) reinterpret_cast<float2*>(m.proj)[o] = front ? make_float2(uf, vf) : make_float2(-1.f, -1.f);
    if (m.pairs && j1 >= 0 && d1 <= m.max_dist &&
        (m.ratio_pct == 0 || j2 < 0 || (long long)d1 * 100 < (long long)m.ratio_pct * d2))
        atomicMin(m.scr.claim + (size_t)p * m.k_stride + j1, ((uint32_t)d1 << 20) | (uint32_t)i);
}

// One block per problem: the keypoints some point bid for, in ascending index,
// each with the point of its smallest bid (block_compact_row, as match_filter_kernel).
__global__ void __launch_bounds__(kProjThreads) proj_pairs_kernel(ProjMatch m) {
    __shared__ int s_wave[kProjThreads / 64];
    const int p = blockIdx.x;
    const int nk = max(min(m.n_kp[m.k_set ? m.k_set[p] : p], m.k_stride), 0);
    const uint32_t* claim = m.scr.claim + (size_t)p * m.k_stride;
    int2* out = reinterpret_cast<int2*>(m.pairs) + (size_t)p * m.k_stride;
    int base = 0;
    for (int j0 = 0; j0 < nk; j0 += kProjThreads) {  // block-uniform trip count
        const int j = j0 + threadIdx.x;
        const uint32_t c = j < nk ? claim[j] : kProjNoKey;
        const bool keep = c != kProjNoKey;
        const int row = block_compact_row<kProjThreads>(keep, base, s_wave);
        if (keep) out[row] = make_int2(j, (int)(c & (kProjMaxStride - 1)));  // row < nk <= k_stride
    }
    if (threadIdx.x == 0) m.n_pairs[p] = base;
}

}  // namespace

hipError_t launch_proj_bin(const ProjMatch& m, int n_problems, hipStream_t st) {
    if (n_problems <= 0) return hipSuccess;
    hipLaunchKernelGGL(proj_bin_kernel, dim3(n_problems), dim3(kProjThreads), 0, st, m);
    return hipGetLastError();
}

hipError_t launch_proj_match(const ProjMatch& m, int n_problems, int max_pts, hipStream_t st) {
    if (n_problems <= 0 || max_pts <= 0) return hipSuccess;
    if (m.lanes == 16) {
        constexpr int per = kProjThreads / 16;
        hipLaunchKernelGGL(proj_match_kernel<16>, dim3((max_pts + per - 1) / per, n_problems), dim3(kProjThreads), 0,
                           st, m);
    } else {
        hipLaunchKernelGGL(proj_match_kernel<1>, dim3((max_pts + kProjThreads - 1) / kProjThreads, n_problems),
                           dim3(kProjThreads), 0, st, m);
    }
    return hipGetLastError();
}

hipError_t launch_proj_pairs(const ProjMatch& m, int n_problems, hipStream_t st) {
    if (n_problems <= 0 || !m.pairs) return hipSuccess;
    hipLaunchKernelGGL(proj_pairs_kernel, dim3(n_problems), dim3(kProjThreads), 0, st, m);
    return hipGetLastError();
}

}  // namespace svo
