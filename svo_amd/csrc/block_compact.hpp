// A block's stable compaction step, stated once (match_filter.hip,
// match_projected.hip): the threads of a block go over a list in chunks of
// kThreads, one entry per thread, and the kept entries leave in list order.
#pragma once

#include <hip/hip_runtime.h>

namespace svo {

// One chunk. Every thread of the block calls it (two barriers inside). A wave's
// ballot gives each kept entry its place among the wave's (the popcount of the
// lower lanes' bits), the waves' counts go through s_wave (kThreads / 64 ints of
// LDS) for the waves in front, and `base` carries the chunks before: on return it
// holds the kept entries so far, the same in every thread. Returns the output
// row of this thread's entry (meaningful where keep).
template <int kThreads>
__device__ __forceinline__ int block_compact_row(bool keep, int& base, int* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int before = base, total = base;
    for (int w = 0; w < kThreads / 64; w++) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    base = total;
    __syncthreads();  // s_wave is rewritten by the next chunk
    return before + __popcll(b & ((1ull << lane) - 1));
}

}  // namespace svo
