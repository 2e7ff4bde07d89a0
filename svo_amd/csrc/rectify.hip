// Rectifying ingest: level 0 of the device pyramid from a RAW camera frame, i.e.
// cv::remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) of 8-bit grey
// with OpenCV's fixed-point maps (initUndistortRectifyMap(..., CV_16SC2, ...) /
// convertMaps): map1 int16 (sx, sy) per output pixel, map2 uint16 < 1024 holding
// the fractions a = map2 & 31 (x) and b = map2 >> 5 (y) in 1/32 pixel.
//
//   tap(i, j) = src[sy + i][sx + j] inside the raw image, else 0
//   out = ((32-a)(32-b) tap(0,0) + a(32-b) tap(0,1) + (32-a)b tap(1,0) + ab tap(1,1) + 512) >> 10
//
// OpenCV's remapBilinear holds these four products times 32 in a 15-bit table and
// casts with (v + 16384) >> 15: the same integer (at a = b = 0 its one saturated
// weight 32767 still returns tap(0,0)). Pure integer, exact, like gray_of. BGR
// input: every tap is gray_of(B, G, R) first = cvtColor(BGR2GRAY), then remap.
//
// The same stage as ingest_batched_kernel (ingest.hip) with a gather in front:
// the staging block mirrors the host frames byte for byte, grid (quads / 256, h,
// S), one thread makes four pixels and stores one dword; one map pair per eye
// serves all S sequences (it stays in L2 / the Infinity Cache).
//
// Address safety: no load leaves a source row of the staging block. The two taps
// of a source row are adjacent, so they travel as one unaligned pair load at
// column cx = clamp(sx, 0, raw_w - 2) of row clamp(sy + i, 0, raw_h - 1), and
// selects pick the bytes: in place (sx == cx), shifted by one at either edge (sx ==
// -1: tap(.,1) is the pair's first byte; sx == raw_w - 1: tap(.,0) is its second),
// zero otherwise. A naive pair load at sx leaves the allocation at sx = -1 on the
// first row of sequence 0 and at sx = raw_w - 1 on the last row of the last
// sequence when stride == raw_w.
#include "ingest_device.hpp"

namespace svo {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
// the maps' rows are w elements apart (any w): a quad's map1 is 4-byte, its map2 2-byte aligned
typedef u32x4 u32x4a4 __attribute__((aligned(4)));
typedef u32x2 u32x2a2 __attribute__((aligned(2)));

// the grey values of columns c and c + 1 of a source row (p: the row's byte at column c)
template <bool BGR>
__device__ __forceinline__ void rect_pair(const uint8_t* p, uint32_t& p0, uint32_t& p1) {
    if (BGR) {
        const uint32_t lo = *reinterpret_cast<const u32a1*>(p);      // B0 G0 R0 B1
        const uint32_t hi = *reinterpret_cast<const u16a1*>(p + 4);  // G1 R1
        p0 = gray_of(lo & 255, (lo >> 8) & 255, (lo >> 16) & 255);
        p1 = gray_of(lo >> 24, hi & 255, hi >> 8);
    } else {
        const uint32_t v = *reinterpret_cast<const u16a1*>(p);
        p0 = v & 255;
        p1 = v >> 8;
    }
}

// one output pixel; src: the sequence's raw frame, m1 = sx | sy << 16, m2 = a | b << 5
template <bool BGR>
__device__ __forceinline__ uint32_t rect_pixel(const uint8_t* __restrict__ src, int spitch, int raw_w, int raw_h,
                                               uint32_t m1, uint32_t m2) {
    const int sx = (int16_t)(m1 & 0xFFFFu), sy = (int16_t)(m1 >> 16);
    const uint32_t a = m2 & 31u, b = m2 >> 5;
    const int cx = min(max(sx, 0), raw_w - 2);
    const int dx = sx - cx;  // 0: in place; -1 / 1: one column off at the left / right edge; else outside
    uint32_t acc = 512u;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int ry = sy + i;
        const int cy = min(max(ry, 0), raw_h - 1);
        uint32_t p0, p1;
        rect_pair<BGR>(src + (size_t)cy * spitch + (size_t)cx * (BGR ? 3 : 1), p0, p1);
        uint32_t t0 = dx == 0 ? p0 : dx == 1 ? p1 : 0u;
        uint32_t t1 = dx == 0 ? p1 : dx == -1 ? p0 : 0u;
        t0 = ry == cy ? t0 : 0u;
        t1 = ry == cy ? t1 : 0u;
        acc += (i ? b : 32u - b) * ((32u - a) * t0 + a * t1);
    }
    return acc >> 10;
}

// stage: [S][raw_h][spitch] raw frames, sequences seq_stride apart; map1 as one
// dword per output pixel, rows w apart; each sequence's level 0 from the
// descriptor array (w x h; its borders are the pyramid chain's to write).
template <bool BGR>
__global__ void __launch_bounds__(256) rectify_batched_kernel(const uint8_t* __restrict__ stage, size_t seq_stride,
                                                              int spitch, int raw_w, int raw_h,
                                                              const uint32_t* __restrict__ map1,
                                                              const uint16_t* __restrict__ map2,
                                                              const PyrDesc* __restrict__ descs, int w, int h) {
    const int s = blockIdx.z, y = blockIdx.y;
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= w) return;
    const ImgLevel L = descs[s].lv[0];
    const uint8_t* src = stage + (size_t)s * seq_stride;
    uint8_t* d = const_cast<uint8_t*>(L.data) + (size_t)y * L.pitch + x;
    const size_t p = (size_t)y * w + x;
    if (x + 4 <= w) {
        const u32x4 m1 = *reinterpret_cast<const u32x4a4*>(map1 + p);
        const u32x2 m2 = *reinterpret_cast<const u32x2a2*>(map2 + p);
        const uint32_t out = rect_pixel<BGR>(src, spitch, raw_w, raw_h, m1.x, m2.x & 0xFFFFu) |
                             rect_pixel<BGR>(src, spitch, raw_w, raw_h, m1.y, m2.x >> 16) << 8 |
                             rect_pixel<BGR>(src, spitch, raw_w, raw_h, m1.z, m2.y & 0xFFFFu) << 16 |
                             rect_pixel<BGR>(src, spitch, raw_w, raw_h, m1.w, m2.y >> 16) << 24;
        *reinterpret_cast<uint32_t*>(d) = out;  // (level 0 rows are 64-byte aligned at x = 0)
    } else {
        for (int i = 0; x + i < w; i++)
            d[i] = (uint8_t)rect_pixel<BGR>(src, spitch, raw_w, raw_h, map1[p + i], map2[p + i]);
    }
}

hipError_t launch_rectify_batched(const uint8_t* stage, size_t seq_stride, int spitch, const RectMapsDev& m,
                                  const PyrDesc* descs, int S, bool bgr, hipStream_t st) {
    if (m.w <= 0 || m.h <= 0 || S <= 0 || m.raw_w < 2 || m.raw_h < 1 || !m.map1 || !m.map2 ||
        spitch < (bgr ? 3 : 1) * m.raw_w)
        return hipErrorInvalidValue;
    dim3 grid(((m.w + 3) / 4 + 255) / 256, m.h, S);
    const uint32_t* map1 = reinterpret_cast<const uint32_t*>(m.map1);
    if (bgr)
        hipLaunchKernelGGL(rectify_batched_kernel<true>, grid, dim3(256), 0, st, stage, seq_stride, spitch, m.raw_w,
                           m.raw_h, map1, m.map2, descs, m.w, m.h);
    else
        hipLaunchKernelGGL(rectify_batched_kernel<false>, grid, dim3(256), 0, st, stage, seq_stride, spitch, m.raw_w,
                           m.raw_h, map1, m.map2, descs, m.w, m.h);
    return hipGetLastError();
}

}  // namespace svo
