// Device code of the ORB descriptor rules, shared by the
// one-image kernels (orb_describe.hip) and the batched front end's place memory
// (places.hip): the 7-tap blur of one tile, a keypoint's moments and direction,
// and the steered BRIEF tests of one wave. Every value that decides a bit is an
// exact integer or one correctly rounded f64 operation.
#pragma once

#include "orb.hpp"

namespace svo {

// BORDER_REFLECT_101 into [0, n), reflected as often as a level narrower than the
// kernel needs; a one-pixel axis reads its only pixel
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

constexpr int kBlurR = 3;                  // 7 taps
constexpr int kBlurTW = 64, kBlurTH = 16;  // output tile
constexpr int kBlurSW = kBlurTW + 2 * kBlurR, kBlurSH = kBlurTH + 2 * kBlurR;
constexpr int kBlurSP = 72;                // source tile row pitch (bytes)

// Separable 7-tap blur, 8-bit weights {18, 34, 49, 54, 49, 34, 18} (sum 256):
// h = sum w p (<= 65280, u16), out = (sum w h + 32768) >> 16. The 64 x 16 tile at
// (x0, y0) of L by one block of 256 threads: the source tile with its reflected
// halo goes through LDS, then the row sums of its 22 rows, then the columns.
__device__ __forceinline__ void orb_blur_tile(const ImgLevel& L, int x0, int y0, uint8_t* out, int dp) {
    __shared__ uint8_t s_src[kBlurSH][kBlurSP];
    __shared__ uint16_t s_h[kBlurSH][kBlurTW];
    const int tid = threadIdx.x;
    for (int i = tid; i < kBlurSH * kBlurSW; i += 256) {
        const int r = i / kBlurSW, c = i - r * kBlurSW;
        const int y = reflect101(y0 - kBlurR + r, L.h), x = reflect101(x0 - kBlurR + c, L.w);
        s_src[r][c] = L.data[(size_t)y * L.pitch + x];
    }
    __syncthreads();
    for (int i = tid; i < kBlurSH * kBlurTW; i += 256) {
        const int r = i / kBlurTW, c = i - r * kBlurTW;
        const uint8_t* p = &s_src[r][c];
        s_h[r][c] = (uint16_t)(18 * (p[0] + p[6]) + 34 * (p[1] + p[5]) + 49 * (p[2] + p[4]) + 54 * p[3]);
    }
    __syncthreads();
    for (int i = tid; i < kBlurTH * kBlurTW; i += 256) {
        const int r = i / kBlurTW, c = i - r * kBlurTW;
        const int x = x0 + c, y = y0 + r;
        if (x >= L.w || y >= L.h) continue;
        const unsigned v = 18u * (s_h[r][c] + s_h[r + 6][c]) + 34u * (s_h[r + 1][c] + s_h[r + 5][c]) +
                           49u * (s_h[r + 2][c] + s_h[r + 4][c]) + 54u * s_h[r + 3][c];
        out[(size_t)y * dp + x] = (uint8_t)((v + 32768u) >> 16);
    }
}

struct OrbUmax {
    int u[16];  // hp <= 15
};

__device__ __forceinline__ int wave_sum(int v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// The moments of the circular patch around (cx, cy) of L, by one wave: lane
// j < 2 hp + 1 takes row v = j - hp: m10 += u I and the row sum, in int32
// (|m| <= 31 * 31 * 15 * 255); every lane returns the reduced sums.
__device__ __forceinline__ void orb_moments(const ImgLevel& L, int cx, int cy, int hp, const OrbUmax& um, int lane,
                                            int& m10, int& m01) {
    m10 = 0;
    m01 = 0;
    const int v = lane - hp;
    if (lane <= 2 * hp) {
        const int d = um.u[v < 0 ? -v : v];
        const uint8_t* row = L.data + (size_t)(cy + v) * L.pitch + cx;
        int rs = 0;
        for (int u = -d; u <= d; u++) {
            const int I = row[u];
            m10 += u * I;
            rs += I;
        }
        m01 = v * rs;
    }
    m10 = wave_sum(m10);
    m01 = wave_sum(m01);
}

// c = m10 / hyp, s = m01 / hyp in f64 ((1, 0) without a gradient)
__device__ __forceinline__ OrbDirection orb_direction(int m10, int m01) {
    const long long r2 = (long long)m10 * m10 + (long long)m01 * m01;  // < 2^53: exact as a double
    OrbDirection o{1.0, 0.0};
    if (r2 != 0) {
        const double hyp = sqrt((double)r2);
        o.c = (double)m10 / hyp;
        o.s = (double)m01 / hyp;
    }
    return o;
}

// The 256 tests of one keypoint by one wave, four rounds: in round r lane j owns
// test 64 r + j, i.e. pattern points 2 (64 r + j) and the next. It steers both by
// (c, s) in f64 (two exact products and one rounded addition per coordinate),
// gathers two bytes of the blurred level and compares; the ballot's 64 bits are
// descriptor bytes 8 r .. 8 r + 7 (bit j of byte i = test 8 i + j). Lane r < 4
// returns the ballot of round r.
__device__ __forceinline__ unsigned long long orb_brief_words(const ImgLevel& L, int cx, int cy, double c, double s,
                                                              const char2* s_pat, int reach, int lane) {
    const uint8_t* centre = L.data + (size_t)cy * L.pitch + cx;
    unsigned long long word = 0;
    for (int r = 0; r < 4; r++) {
        int smp[2];
        for (int e = 0; e < 2; e++) {
            const char2 p = s_pat[2 * (64 * r + lane) + e];
            const double px = (double)p.x, py = (double)p.y;
            int ix = __double2int_rn(px * c - py * s);
            int iy = __double2int_rn(px * s + py * c);
            // |(ix, iy)| <= rint(hp sqrt 2 (1 + 2^-52)) = reach for every supported hp: the
            // clamp never binds; it keeps a corrupt direction from reading outside the level
            ix = min(max(ix, -reach), reach);
            iy = min(max(iy, -reach), reach);
            smp[e] = centre[iy * L.pitch + ix];
        }
        const unsigned long long b = __ballot(smp[0] < smp[1]);
        if (lane == r) word = b;
    }
    return word;
}

}  // namespace svo
