// svo_match_filter for many problems at once (svo_match_filter_batch, and the
// place memory's query): the ratio test and the cross-check on the rows
// hamming_knn2_kernel wrote, integers only, then the kept pairs compacted in
// ascending query index. The order is part of the result: it decides the draws
// of the RANSAC that takes the pairs.
#include "block_compact.hpp"
#include "orb.hpp"

namespace svo {

namespace {

constexpr int kFilterThreads = 256;

// One block per problem. Queries go by in chunks of 256, one per thread: keep is
// svo_match_filter's rule; block_compact_row places the kept ones in order.
__global__ void __launch_bounds__(kFilterThreads) match_filter_kernel(
    const int2* __restrict__ idx_qt, const int2* __restrict__ dist_qt, const int2* __restrict__ idx_tq,
    const int* __restrict__ nq_p, const int* __restrict__ nt_p, int q_stride, int t_stride, int ratio_pct,
    int2* __restrict__ pairs, int* __restrict__ n_pairs, const int* __restrict__ q_set,
    const int* __restrict__ t_set) {
    __shared__ int s_wave[kFilterThreads / 64];
    const int p = blockIdx.x;
    const int nq = min(nq_p[q_set ? q_set[p] : p], q_stride);
    const int nt = min(nt_p[t_set ? t_set[p] : p], t_stride);
    const int2* iq = idx_qt + (size_t)p * q_stride;
    const int2* dq = dist_qt + (size_t)p * q_stride;
    const int2* it = idx_tq ? idx_tq + (size_t)p * t_stride : nullptr;
    int2* out = pairs + (size_t)p * q_stride;
    int base = 0;
    for (int q0 = 0; q0 < nq; q0 += kFilterThreads) {  // block-uniform trip count
        const int q = q0 + threadIdx.x;
        bool keep = false;
        int i1 = -1;
        if (q < nq) {
            const int2 i = iq[q], d = dq[q];
            i1 = i.x;
            keep = i1 >= 0 && i1 < nt;
            if (keep && ratio_pct != 0)
                keep = i.y >= 0 && (long long)d.x * 100 < (long long)ratio_pct * d.y;
            if (keep && it) keep = it[i1].x == q;
        }
        const int row = block_compact_row<kFilterThreads>(keep, base, s_wave);
        if (keep) out[row] = make_int2(q, i1);  // < nq <= q_stride
    }
    if (threadIdx.x == 0) n_pairs[p] = base;
}

}  // namespace

hipError_t launch_match_filter(const int* idx_qt, const int* dist_qt, const int* idx_tq, const int* nq,
                               const int* nt, int q_stride, int t_stride, int n_problems, int ratio_pct, int* pairs,
                               int* n_pairs, hipStream_t st, const int* q_set, const int* t_set) {
    if (n_problems <= 0) return hipSuccess;
    hipLaunchKernelGGL(match_filter_kernel, dim3(n_problems), dim3(kFilterThreads), 0, st,
                       reinterpret_cast<const int2*>(idx_qt), reinterpret_cast<const int2*>(dist_qt),
                       reinterpret_cast<const int2*>(idx_tq), nq, nt, q_stride, t_stride, ratio_pct,
                       reinterpret_cast<int2*>(pairs), n_pairs, q_set, t_set);
    return hipGetLastError();
}

}  // namespace svo
