// svo_match_projected behind the C ABI (the rules: DESIGN.md section 3f;
// include/svo_gpu.h): the argument checks, the upload into the context's scratch,
// the three launches of match_projected.hip and the download of the live rows.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "linalg.hpp"
#include "match_projected.hpp"

using namespace svo;

const char* svo::proj_params_refused(int w, int h, const svo_proj_match_params* prm) {
    if (!prm) return "null params";
    if (w < 1 || h < 1) return "w or h < 1";
    if (!std::isfinite(prm->radius) || !(prm->radius > 0.f)) return "radius not finite or <= 0";
    if (prm->max_dist < 0 || prm->max_dist > 256) return "max_dist outside [0, 256]";
    if (prm->ratio_pct < 0) return "ratio_pct < 0";
    return nullptr;
}

namespace {

// svo_match_projected, and with time_reps > 0 svo_match_projected_time: each
// launch again `reps` times between events instead of the download
int proj_run(svo_ctx* ctx, int n_problems, const int* n_pts, const int* n_kp, int p_stride, int k_stride,
             const double* xyz, const uint8_t* pdesc, const float* kxy, const uint8_t* kdesc, const double* poses,
             const double* K4, int w, int h, const svo_proj_match_params* prm, int* idx, int* dist, float* proj,
             int* pairs, int* n_pairs, const char* who, int time_reps, double* time_ms) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_problems < 0 || n_problems > 65535 || p_stride < 0 || k_stride < 0 || p_stride > kProjMaxStride ||
        k_stride > kProjMaxStride)
        return set_error(ctx, SVO_ERR_ARG, "%s: problems outside [0, 65535] or a stride outside [0, 2^20]", who);
    if (const char* why = proj_params_refused(w, h, prm)) return set_error(ctx, SVO_ERR_ARG, "%s: %s", who, why);
    if (pairs && !n_pairs) return set_error(ctx, SVO_ERR_ARG, "%s: pairs without n_pairs", who);
    if (n_problems == 0) return SVO_OK;
    if (!n_pts || !n_kp) return set_error(ctx, SVO_ERR_ARG, "%s: null counts", who);
    int max_pts = 0, max_kp = 0;
    for (int p = 0; p < n_problems; p++) {
        if (n_pts[p] < 0 || n_pts[p] > p_stride || n_kp[p] < 0 || n_kp[p] > k_stride)
            return set_error(ctx, SVO_ERR_ARG, "%s: counts of problem %d outside [0, stride]", who, p);
        max_pts = n_pts[p] > max_pts ? n_pts[p] : max_pts;
        max_kp = n_kp[p] > max_kp ? n_kp[p] : max_kp;
    }
    if ((max_pts > 0 && (!xyz || !pdesc || !poses || !K4)) || (max_kp > 0 && (!kxy || !kdesc)))
        return set_error(ctx, SVO_ERR_ARG, "%s: null arrays", who);
    const size_t P = (size_t)n_problems, PS = (size_t)p_stride, KS = (size_t)k_stride;
    const bool want_pairs = pairs != nullptr || time_reps > 0;
    if (max_pts == 0 && max_kp == 0) {
        if (pairs) std::memset(n_pairs, 0, sizeof(int) * P);
        return SVO_OK;
    }
    hipStream_t st = ctx->stream;
    ProjMatch m{};
    double* dxyz;
    uint32_t *dpd, *dkd;
    float* dkxy;
    double* dposes;
    int *dnp, *dnk;
    m.grid = proj_grid(w, h);
    if (!carve_scratch(ctx, kScratchDescribe, [&](Carver& c) {
            dxyz = c.take<double>(3 * P * PS);
            dpd = c.take<uint32_t>(8 * P * PS);
            dkxy = c.take<float>(2 * P * KS);
            dkd = c.take<uint32_t>(8 * P * KS);
            dposes = c.take<double>(12 * P);
            dnp = c.take<int>(P);
            dnk = c.take<int>(P);
            proj_scratch_layout(c, m.scr, P, KS, m.grid);
            m.idx = c.take<int>(2 * P * PS);
            m.dist = c.take<int>(2 * P * PS);
            m.proj = c.take<float>(2 * P * PS);
            m.pairs = c.take<int>(2 * P * KS);
            m.n_pairs = c.take<int>(P);
        }))
        return set_error(ctx, SVO_ERR_HIP, "%s: workspace alloc failed", who);
    if (!want_pairs) m.pairs = nullptr;
    if (!time_reps) {  // an output the caller skips is not computed
        if (!idx) m.idx = nullptr;
        if (!dist) m.dist = nullptr;
        if (!proj) m.proj = nullptr;
    }
    // (with no point anywhere the point arrays may be null, and likewise the keypoints')
    if (max_pts > 0) {
        SVO_HIP(ctx, hipMemcpyAsync(dxyz, xyz, sizeof(double) * 3 * P * PS, hipMemcpyHostToDevice, st));
        SVO_HIP(ctx, hipMemcpyAsync(dpd, pdesc, SVO_ORB_DESC_BYTES * P * PS, hipMemcpyHostToDevice, st));
        SVO_HIP(ctx, hipMemcpyAsync(dposes, poses, sizeof(double) * 12 * P, hipMemcpyHostToDevice, st));
    }
    if (max_kp > 0) {
        SVO_HIP(ctx, hipMemcpyAsync(dkxy, kxy, sizeof(float) * 2 * P * KS, hipMemcpyHostToDevice, st));
        SVO_HIP(ctx, hipMemcpyAsync(dkd, kdesc, SVO_ORB_DESC_BYTES * P * KS, hipMemcpyHostToDevice, st));
    }
    SVO_HIP(ctx, hipMemcpyAsync(dnp, n_pts, sizeof(int) * P, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(dnk, n_kp, sizeof(int) * P, hipMemcpyHostToDevice, st));
    m.n_pts = dnp;
    m.n_kp = dnk;
    m.p_stride = p_stride;
    m.k_stride = k_stride;
    m.xyz = dxyz;
    m.pdesc = dpd;
    m.kxy = dkxy;
    m.kdesc = dkd;
    m.poses = dposes;
    if (max_pts > 0) {
        m.fx = K4[0];
        m.fy = K4[1];
        m.cx = K4[2];
        m.cy = K4[3];
    }
    m.w = w;
    m.h = h;
    m.radius = prm->radius;
    m.max_dist = prm->max_dist;
    m.ratio_pct = prm->ratio_pct;
    // A/B and test hook of the launch shape, read per call: SVO_PROJ_LANES=16 (a quarter wave per point)
    if (const char* e = std::getenv("SVO_PROJ_LANES")) m.lanes = std::atoi(e);
    SVO_HIP(ctx, launch_proj_bin(m, n_problems, st));
    SVO_HIP(ctx, launch_proj_match(m, n_problems, max_pts, st));
    SVO_HIP(ctx, launch_proj_pairs(m, n_problems, st));
    if (time_reps > 0) {
        hipEvent_t e[2] = {nullptr, nullptr};
        auto timed = [&](double* ms, auto&& launch) -> hipError_t {
            hipError_t r = hipEventRecord(e[0], st);
            for (int k = 0; k < time_reps && r == hipSuccess; k++) r = launch();
            if (r == hipSuccess) r = hipEventRecord(e[1], st);
            if (r == hipSuccess) r = hipEventSynchronize(e[1]);
            float t = 0.f;
            if (r == hipSuccess) r = hipEventElapsedTime(&t, e[0], e[1]);
            *ms = (double)t / time_reps;
            return r;
        };
        hipError_t r = hipEventCreate(&e[0]);
        if (r == hipSuccess) r = hipEventCreate(&e[1]);
        // (the match launch bids again for what it claimed: the same minima, the same pairs)
        if (r == hipSuccess) r = timed(&time_ms[0], [&] { return launch_proj_bin(m, n_problems, st); });
        if (r == hipSuccess) r = timed(&time_ms[1], [&] { return launch_proj_match(m, n_problems, max_pts, st); });
        if (r == hipSuccess) r = timed(&time_ms[2], [&] { return launch_proj_pairs(m, n_problems, st); });
        (void)hipStreamSynchronize(st);
        for (hipEvent_t ev : e)
            if (ev) (void)hipEventDestroy(ev);
        SVO_HIP(ctx, r);
        return SVO_OK;
    }
    // only the live rows reach the caller: the padding up to the strides stays as it was
    std::vector<int> hi(idx ? 2 * P * PS : 0), hd(dist ? 2 * P * PS : 0), hp(pairs ? 2 * P * KS : 0), hn(P, 0);
    std::vector<float> hj(proj ? 2 * P * PS : 0);
    if (!hi.empty()) SVO_HIP(ctx, hipMemcpyAsync(hi.data(), m.idx, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, st));
    if (!hd.empty()) SVO_HIP(ctx, hipMemcpyAsync(hd.data(), m.dist, sizeof(int) * hd.size(), hipMemcpyDeviceToHost, st));
    if (!hj.empty())
        SVO_HIP(ctx, hipMemcpyAsync(hj.data(), m.proj, sizeof(float) * hj.size(), hipMemcpyDeviceToHost, st));
    if (pairs) {
        if (!hp.empty())
            SVO_HIP(ctx, hipMemcpyAsync(hp.data(), m.pairs, sizeof(int) * hp.size(), hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipMemcpyAsync(hn.data(), m.n_pairs, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    }
    SVO_HIP(ctx, hipStreamSynchronize(st));
    for (size_t p = 0; p < P; p++) {
        const size_t at = 2 * p * PS, n = 2 * (size_t)n_pts[p];
        if (!hi.empty()) std::memcpy(idx + at, hi.data() + at, sizeof(int) * n);
        if (!hd.empty()) std::memcpy(dist + at, hd.data() + at, sizeof(int) * n);
        if (!hj.empty()) std::memcpy(proj + at, hj.data() + at, sizeof(float) * n);
        if (pairs) {
            n_pairs[p] = hn[p];
            if (hn[p] > 0) std::memcpy(pairs + 2 * p * KS, hp.data() + 2 * p * KS, sizeof(int) * 2 * hn[p]);
        }
    }
    return SVO_OK;
}

}  // namespace

extern "C" int svo_match_projected(svo_ctx* ctx, int n_problems, const int* n_pts, const int* n_kp, int p_stride,
                                   int k_stride, const double* xyz, const uint8_t* pdesc, const float* kxy,
                                   const uint8_t* kdesc, const double* poses, const double* K4, int w, int h,
                                   const svo_proj_match_params* params, int* idx, int* dist, float* proj, int* pairs,
                                   int* n_pairs) {
    return proj_run(ctx, n_problems, n_pts, n_kp, p_stride, k_stride, xyz, pdesc, kxy, kdesc, poses, K4, w, h, params,
                    idx, dist, proj, pairs, n_pairs, "svo_match_projected", 0, nullptr);
}

extern "C" int svo_match_projected_time(svo_ctx* ctx, int n_problems, const int* n_pts, const int* n_kp, int p_stride,
                                        int k_stride, const double* xyz, const uint8_t* pdesc, const float* kxy,
                                        const uint8_t* kdesc, const double* poses, const double* K4, int w, int h,
                                        const svo_proj_match_params* params, int reps, double ms[3]) {
    if (!ctx) return SVO_ERR_ARG;
    if (reps < 1 || !ms) return set_error(ctx, SVO_ERR_ARG, "svo_match_projected_time: bad arguments");
    ms[0] = ms[1] = ms[2] = 0.0;
    return proj_run(ctx, n_problems, n_pts, n_kp, p_stride, k_stride, xyz, pdesc, kxy, kdesc, poses, K4, w, h, params,
                    nullptr, nullptr, nullptr, nullptr, nullptr, "svo_match_projected_time", reps, ms);
}

extern "C" int svo_pose_from_rvec(const double rvec[3], const double tvec[3], double T[12]) {
    if (!rvec || !tvec || !T) return SVO_ERR_ARG;
    la::rodrigues(rvec, T);
    for (int k = 0; k < 3; k++) T[9 + k] = tvec[k];
    return SVO_OK;
}
