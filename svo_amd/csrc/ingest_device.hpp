// Device helpers the level-0 writers share (ingest.hip, rectify.hip).
#pragma once

#include "common.hpp"

namespace svo {

// OpenCV's CV_8U RGB2Gray, exact integer arithmetic (ingest.hip has the constants' origin)
__device__ __forceinline__ uint32_t gray_of(uint32_t b, uint32_t g, uint32_t r) {
    return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14;
}

// loads at any byte address (global memory allows them): the staging block mirrors
// host rows that need not be aligned (1241, 3723 B)
typedef uint32_t u32a1 __attribute__((aligned(1)));
typedef uint16_t u16a1 __attribute__((aligned(1)));

}  // namespace svo
