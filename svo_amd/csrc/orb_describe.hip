// ORB descriptors on the levels svo_orb_detect builds (the rules: DESIGN.md
// section 3d, restated in tests/orb_describe_reference.py): the blurred copy of
// every level, the intensity-centroid direction of a keypoint, and the steered
// 256-test BRIEF bits. Every value that decides a bit is an exact integer or one
// correctly rounded f64 operation (sqrt, division, one addition of two exact
// products), so the bits do not depend on a maths library or on contraction.
#include "orb_device.hpp"

namespace svo {

namespace {

// One block per 64 x 16 tile of a level (blockIdx.z): orb_blur_tile.
__global__ void __launch_bounds__(256) orb_blur_kernel(PyrDesc src, PyrDesc dst) {
    const ImgLevel L = src.lv[blockIdx.z];
    const int x0 = blockIdx.x * kBlurTW, y0 = blockIdx.y * kBlurTH;
    if (x0 >= L.w || y0 >= L.h) return;  // the grid is sized by the largest level (block-uniform)
    orb_blur_tile(L, x0, y0, const_cast<uint8_t*>(dst.lv[blockIdx.z].data), dst.lv[blockIdx.z].pitch);
}

// One wave per keypoint (orb_moments). Lane 0 turns the reduced moments into
// (c, s) and the reported angle.
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
    int m10, m01;
    orb_moments(levels.lv[kp.level], kp.cx, kp.cy, hp, um, lane, m10, m01);
    if (lane == 0) {
        dir[k] = orb_direction(m10, m01);
        double a = atan2((double)m01, (double)m10) * (180.0 / 3.14159265358979323846);
        if (a < 0) a += 360.0;
        angle[k] = (float)a;
    }
}

// One wave per keypoint (orb_brief_words): lanes 0..3 store the four ballots.
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
    if (kp.level >= 0)
        word = orb_brief_words(blurred.lv[kp.level], kp.cx, kp.cy, dir[k].c, dir[k].s, s_pat, reach, lane);
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
