// ORB descriptors on the levels svo_orb_detect builds (the rules: DESIGN.md
// section 3d, restated in tests/orb_describe_reference.py): the blurred copy of
// every level, the intensity-centroid direction of a keypoint, and the steered
// 256-test BRIEF bits. Every value that decides a bit is an exact integer or one
// correctly rounded f64 operation (sqrt, division, one addition of two exact
// products), so the bits do not depend on a maths library or on contraction.
#include "orb.hpp"

namespace svo {

namespace {

// BORDER_REFLECT_101 into [0, n), reflected as often as a level narrower than the
// kernel needs; a one-pixel axis reads its only pixel
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

constexpr int kBlurR = 3;                 // 7 taps
constexpr int kBlurTW = 64, kBlurTH = 16; // output tile
constexpr int kBlurSW = kBlurTW + 2 * kBlurR, kBlurSH = kBlurTH + 2 * kBlurR;
constexpr int kBlurSP = 72;               // source tile row pitch (bytes)

// Separable 7-tap blur, 8-bit weights {18, 34, 49, 54, 49, 34, 18} (sum 256):
// h = sum w p (<= 65280, u16), out = (sum w h + 32768) >> 16. One block per
// 64 x 16 tile of a level (blockIdx.z): the source tile with its reflected halo
// goes through LDS, then the row sums of its 22 rows, then the columns.
__global__ void __launch_bounds__(256) orb_blur_kernel(PyrDesc src, PyrDesc dst) {
    __shared__ uint8_t s_src[kBlurSH][kBlurSP];
    __shared__ uint16_t s_h[kBlurSH][kBlurTW];
    const ImgLevel L = src.lv[blockIdx.z];
    const int x0 = blockIdx.x * kBlurTW, y0 = blockIdx.y * kBlurTH;
    if (x0 >= L.w || y0 >= L.h) return;  // the grid is sized by the largest level
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
    uint8_t* out = const_cast<uint8_t*>(dst.lv[blockIdx.z].data);
    const int dp = dst.lv[blockIdx.z].pitch;
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

// One wave per keypoint. Lane j < 2 hp + 1 takes row v = j - hp of the circular
// patch: m10 += u I and the row sum, in int32 (|m| <= 31 * 31 * 15 * 255). Lane 0
// turns the reduced moments into (c, s) and the reported angle.
__global__ void __launch_bounds__(256) orb_angle_kernel(PyrDesc levels, const OrbDescKp* __restrict__ kps, int n,
                                                        int hp, OrbUmax um, OrbDirection* __restrict__ dir,
                                                        float* __restrict__ angle) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;  // wave-uniform
    const OrbDescKp kp = kps[k];
    if (kp.level < 0) {
        if (lane == 0) {
            dir[k] = OrbDirection{1.0, 0.0};
            angle[k] = -1.f;
        }
        return;
    }
    const ImgLevel L = levels.lv[kp.level];
    int m10 = 0, m01 = 0;
    const int v = lane - hp;
    if (lane <= 2 * hp) {
        const int d = um.u[v < 0 ? -v : v];
        const uint8_t* row = L.data + (size_t)(kp.cy + v) * L.pitch + kp.cx;
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
    if (lane == 0) {
        const long long r2 = (long long)m10 * m10 + (long long)m01 * m01;  // < 2^53: exact as a double
        OrbDirection o{1.0, 0.0};
        if (r2 != 0) {
            const double hyp = sqrt((double)r2);
            o.c = (double)m10 / hyp;
            o.s = (double)m01 / hyp;
        }
        dir[k] = o;
        double a = atan2((double)m01, (double)m10) * (180.0 / 3.14159265358979323846);
        if (a < 0) a += 360.0;
        angle[k] = (float)a;
    }
}

// One wave per keypoint, four rounds: in round r lane j owns test 64 r + j, i.e.
// pattern points 2 (64 r + j) and the next. It steers both by (c, s) in f64 (two
// exact products and one rounded addition per coordinate), gathers two bytes of
// the blurred level and compares; the ballot's 64 bits are descriptor bytes
// 8 r .. 8 r + 7 (bit j of byte i = test 8 i + j).
__global__ void __launch_bounds__(256) orb_brief_kernel(PyrDesc blurred, const OrbDescKp* __restrict__ kps, int n,
                                                        const int8_t* __restrict__ pattern,
                                                        const OrbDirection* __restrict__ dir, int reach,
                                                        unsigned long long* __restrict__ desc) {
    __shared__ char2 s_pat[kOrbPatternPoints];
    reinterpret_cast<uint32_t*>(s_pat)[threadIdx.x] = reinterpret_cast<const uint32_t*>(pattern)[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;  // wave-uniform
    const OrbDescKp kp = kps[k];
    unsigned long long word = 0;  // lane r < 4 keeps the ballot of round r
    if (kp.level >= 0) {
        const ImgLevel L = blurred.lv[kp.level];
        const uint8_t* centre = L.data + (size_t)kp.cy * L.pitch + kp.cx;
        const double c = dir[k].c, s = dir[k].s;
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
    }
    if (lane < 4) desc[(size_t)k * 4 + lane] = word;
}

}  // namespace

hipError_t launch_orb_blur(const PyrDesc& levels, const PyrDesc& blurred, hipStream_t st) {
    int mw = 0, mh = 0;
    for (int l = 0; l < levels.nlevels; l++) {
        mw = levels.lv[l].w > mw ? levels.lv[l].w : mw;
        mh = levels.lv[l].h > mh ? levels.lv[l].h : mh;
    }
    if (levels.nlevels <= 0 || mw <= 0 || mh <= 0) return hipSuccess;
    dim3 grid((mw + kBlurTW - 1) / kBlurTW, (mh + kBlurTH - 1) / kBlurTH, levels.nlevels);
    hipLaunchKernelGGL(orb_blur_kernel, grid, dim3(256), 0, st, levels, blurred);
    return hipGetLastError();
}

hipError_t launch_orb_angle(const PyrDesc& levels, const OrbDescKp* kp, int n, int hp, const int* umax,
                            OrbDirection* dir, float* angle, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (hp < 1 || hp > 15) return hipErrorInvalidValue;
    OrbUmax um{};
    for (int v = 0; v <= hp; v++) um.u[v] = umax[v];
    hipLaunchKernelGGL(orb_angle_kernel, dim3((n + 3) / 4), dim3(256), 0, st, levels, kp, n, hp, um, dir, angle);
    return hipGetLastError();
}

hipError_t launch_orb_brief(const PyrDesc& blurred, const OrbDescKp* kp, int n, const int8_t* pattern,
                            const OrbDirection* dir, int reach, uint8_t* desc, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(orb_brief_kernel, dim3((n + 3) / 4), dim3(256), 0, st, blurred, kp, n, pattern, dir, reach,
                       reinterpret_cast<unsigned long long*>(desc));
    return hipGetLastError();
}

}  // namespace svo
