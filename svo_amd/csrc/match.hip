// Hamming nearest and second-nearest neighbour of 256-bit descriptors
// (svo_match_hamming; the rule: DESIGN.md section 3d): cv::BFMatcher(NORM_HAMMING)
// ::knnMatch(k = 2) with ties to the lowest train index.
#include "orb.hpp"

namespace svo {

namespace {

constexpr int kMatchQ = 256;  // queries per block, one per thread
constexpr int kMatchT = 256;  // train descriptors per LDS tile (8 KiB)

// grid (query tiles, problems). A thread keeps its query in 8 dwords; the block
// stages the train descriptors through LDS a tile at a time and every thread
// reads train descriptor j at the same address (a broadcast: no bank conflict).
// Per pair 8 xor + 8 accumulating popcounts; (d1, i1, d2, i2) under strict <
// while the train index rises, so ties go to the lowest index. q_set / t_set
// (nullable: problem p uses sets p) name the query and the train set of a problem
// -- descriptors at set * stride, count nq_p[set] / nt_p[set] -- so problems that
// share a set read it in place; the outputs are the problem's own rows.
__global__ void __launch_bounds__(kMatchQ) hamming_knn2_kernel(const uint32_t* __restrict__ q,
                                                               const uint32_t* __restrict__ t,
                                                               const int* __restrict__ nq_p,
                                                               const int* __restrict__ nt_p, int q_stride,
                                                               int t_stride, int2* __restrict__ idx,
                                                               int2* __restrict__ dist,
                                                               const int* __restrict__ q_set,
                                                               const int* __restrict__ t_set) {
    __shared__ uint4 s_t[kMatchT][2];
    const int p = blockIdx.y;
    const int qs = q_set ? q_set[p] : p, ts = t_set ? t_set[p] : p;
    const int nq = min(nq_p[qs], q_stride), nt = min(nt_p[ts], t_stride);  // (never past a set's rows)
    if ((int)blockIdx.x * kMatchQ >= nq) return;  // block-uniform
    const int qi = blockIdx.x * kMatchQ + threadIdx.x;
    const bool live = qi < nq;
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (live) {
        const uint4* qp = reinterpret_cast<const uint4*>(q + ((size_t)qs * q_stride + qi) * 8);
        a0 = qp[0];
        a1 = qp[1];
    }
    const uint4* tp = reinterpret_cast<const uint4*>(t + (size_t)ts * t_stride * 8);
    int d1 = 257, i1 = -1, d2 = 257, i2 = -1;
    for (int base = 0; base < nt; base += kMatchT) {
        const int cnt = min(kMatchT, nt - base);
        if ((int)threadIdx.x < cnt) {  // never past this problem's count
            s_t[threadIdx.x][0] = tp[(size_t)(base + threadIdx.x) * 2];
            s_t[threadIdx.x][1] = tp[(size_t)(base + threadIdx.x) * 2 + 1];
        }
        __syncthreads();
        for (int j = 0; j < cnt; j++) {
            const uint4 b0 = s_t[j][0], b1 = s_t[j][1];
            const int d = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
                          __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
            if (d < d1) {
                d2 = d1;
                i2 = i1;
                d1 = d;
                i1 = base + j;
            } else if (d < d2) {
                d2 = d;
                i2 = base + j;
            }
        }
        __syncthreads();
    }
    if (live) {
        const size_t o = (size_t)p * q_stride + qi;
        idx[o] = make_int2(i1, i2);
        dist[o] = make_int2(d1, d2);
    }
}

}  // namespace

hipError_t launch_hamming_knn2(const uint32_t* q, const uint32_t* t, const int* nq, const int* nt, int q_stride,
                               int t_stride, int n_problems, int max_nq, int* idx, int* dist, hipStream_t st,
                               const int* q_set, const int* t_set) {
    if (n_problems <= 0 || max_nq <= 0) return hipSuccess;
    dim3 grid((max_nq + kMatchQ - 1) / kMatchQ, n_problems);
    hipLaunchKernelGGL(hamming_knn2_kernel, grid, dim3(kMatchQ), 0, st, q, t, nq, nt, q_stride, t_stride,
                       reinterpret_cast<int2*>(idx), reinterpret_cast<int2*>(dist), q_set, t_set);
    return hipGetLastError();
}

}  // namespace svo
