// ORB descriptors and the Hamming matcher behind the C ABI (the rules: DESIGN.md
// section 3d; include/svo_gpu.h): where cv::ORB::compute / detectAndCompute and
// cv::BFMatcher(NORM_HAMMING)::knnMatch(k = 2) would stand in a port. The levels
// are the ones svo_orb_detect builds (orb_build_levels); the kernels are in
// orb_describe.hip and match.hip; the tables, the argument checks and the match
// filter are host code.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "orb.hpp"
#include "pose.hpp"

using namespace svo;

namespace {

// patch_size odd in [5, 31]
bool patch_ok(int patch_size) { return patch_size >= 5 && patch_size <= 31 && (patch_size & 1); }

int orb_reach(int hp) { return (int)std::nearbyint(hp * std::sqrt(2.0)); }

// orb.cpp's umax: row |v| of the circular patch spans |u| <= umax[|v|]
void orb_umax(int hp, int* umax) {
    int u[18] = {0};
    const int vmax = (int)std::floor(hp * std::sqrt(2.0) / 2 + 1);
    const int vmin = (int)std::ceil(hp * std::sqrt(2.0) / 2);
    for (int v = 0; v <= vmax; v++) u[v] = (int)std::nearbyint(std::sqrt((double)hp * hp - (double)v * v));
    for (int v = hp, v0 = 0; v >= vmin; --v) {
        while (u[v0] == u[v0 + 1]) ++v0;
        u[v] = v0;
        ++v0;
    }
    for (int v = 0; v <= hp; v++) umax[v] = u[v];
}

// orb.cpp's makeRandomPattern: cv::RNG(0x34985739), x before y
void default_pattern(int hp, int8_t* xy) {
    Rng rng{0x34985739ull};
    for (int i = 0; i < kOrbPatternPoints; i++) {
        xy[2 * i] = (int8_t)rng.uniform(-hp, hp + 1);
        xy[2 * i + 1] = (int8_t)rng.uniform(-hp, hp + 1);
    }
}

// What the descriptor entry points reject beyond orb_geometry's checks; on
// success pat holds the pattern to use.
const char* check_describe(const svo_orb_params* prm, const int8_t* pattern_xy, int8_t* pat) {
    if (!patch_ok(prm->patch_size)) return "patch_size must be odd and in [5, 31]";
    if (prm->wta_k != 2) return "only wta_k = 2 is supported";
    if (prm->first_level != 0) return "first_level must be 0";
    const int hp = prm->patch_size / 2;
    if (!pattern_xy) {
        default_pattern(hp, pat);
        return nullptr;
    }
    for (int i = 0; i < 2 * kOrbPatternPoints; i++)
        if (pattern_xy[i] < -hp || pattern_xy[i] > hp) return "pattern entry outside [-hp, hp]";
    std::memcpy(pat, pattern_xy, 2 * kOrbPatternPoints);
    return nullptr;
}

}  // namespace

const char* svo::orb_describe_tables(int patch_size, const int8_t* pattern_xy, int8_t* pat, int* umax, int* reach) {
    svo_orb_params prm{};
    prm.patch_size = patch_size;
    prm.wta_k = 2;
    if (const char* why = check_describe(&prm, pattern_xy, pat)) return why;
    orb_umax(patch_size / 2, umax);
    *reach = orb_reach(patch_size / 2);
    return nullptr;
}

namespace {

// ms per launch of `reps` back-to-back launches between two HIP events (after the
// caller's own first launch as the warm-up); measurement entry points only
struct TimedLoop {
    svo_ctx* ctx;
    int reps;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    TimedLoop(svo_ctx* c, int r) : ctx(c), reps(r) {
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
    }
    ~TimedLoop() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    template <class F>
    hipError_t run(double* ms, F&& launch) {
        if (!e0 || !e1) return hipErrorOutOfMemory;
        hipError_t e = hipEventRecord(e0, ctx->stream);
        for (int r = 0; r < reps && e == hipSuccess; r++) e = launch();
        if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float t = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
        *ms = (double)t / reps;
        return e;
    }
};

struct DescWork {
    PyrDesc blurred;
    OrbDescKp* kp;
    OrbDirection* dir;
    float* angle;
    uint8_t* desc;
    int8_t* pat;
};

// Lays out the workspace for n keypoints on the levels of o and queues the blur.
int blur_levels(svo_ctx* ctx, const OrbLevels& o, int n, const char* who, DescWork& w) {
    const OrbGeometry& g = o.g;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    w.blurred = PyrDesc{};
    w.blurred.nlevels = g.nlev;
    if (!carve_scratch(ctx, kScratchDescribe, [&](Carver& c) {
            for (int l = 0; l < g.nlev; l++) {
                const int bp = (g.lw[l] + 63) & ~63;
                w.blurred.lv[l] = ImgLevel{c.take<uint8_t>((size_t)bp * g.lh[l]), g.lw[l], g.lh[l], bp};
            }
            w.kp = c.take<OrbDescKp>(nn);
            w.dir = c.take<OrbDirection>(nn);
            w.angle = c.take<float>(nn);
            w.desc = c.take<uint8_t>((size_t)SVO_ORB_DESC_BYTES * nn);
            w.pat = c.take<int8_t>(2 * kOrbPatternPoints);
        }))
        return set_error(ctx, SVO_ERR_HIP, "%s: workspace alloc failed", who);
    SVO_HIP(ctx, launch_orb_blur(o.lev, w.blurred, ctx->stream));
    return SVO_OK;
}

// The descriptor half: n keypoints (level-0 coordinates, octaves checked by the
// caller) on the levels of o. Synchronous.
int describe_levels(svo_ctx* ctx, const svo_orb_params* prm, const OrbLevels& o, const int8_t* pat,
                    const svo_keypoint* kp, const int* octave, int n, uint8_t* desc, float* angle, uint8_t* valid,
                    const char* who, int time_reps = 0, double* time_ms = nullptr) {
    if (n <= 0) return SVO_OK;
    const OrbGeometry& g = o.g;
    hipStream_t st = ctx->stream;
    const int hp = prm->patch_size / 2, reach = orb_reach(hp);
    int umax[16];
    orb_umax(hp, umax);
    std::vector<OrbDescKp> hk(n);
    std::vector<uint8_t> hv(n);
    for (int i = 0; i < n; i++) {
        const int l = octave[i];
        const float inv = 1.f / g.lscale[l];
        const int cx = (int)std::nearbyint(kp[i].x * inv), cy = (int)std::nearbyint(kp[i].y * inv);  // cvRound(float)
        const bool ok = cx >= reach && cx <= g.lw[l] - 1 - reach && cy >= reach && cy <= g.lh[l] - 1 - reach;
        hk[i] = OrbDescKp{cx, cy, ok ? l : -1, 0};
        hv[i] = ok ? 1 : 0;
    }
    DescWork w;
    const int rc = blur_levels(ctx, o, n, who, w);
    if (rc != SVO_OK) return rc;
    SVO_HIP(ctx, hipMemcpyAsync(w.kp, hk.data(), sizeof(OrbDescKp) * n, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(w.pat, pat, 2 * kOrbPatternPoints, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, launch_orb_angle(o.lev, w.kp, n, hp, umax, w.dir, w.angle, st));
    SVO_HIP(ctx, launch_orb_brief(w.blurred, w.kp, n, w.pat, w.dir, reach, w.desc, st));
    if (time_reps > 0) {  // svo_orb_describe_time: the three kernels again, each `reps` times between events
        TimedLoop tl(ctx, time_reps);
        SVO_HIP(ctx, tl.run(&time_ms[0], [&] { return launch_orb_blur(o.lev, w.blurred, st); }));
        SVO_HIP(ctx, tl.run(&time_ms[1],
                            [&] { return launch_orb_angle(o.lev, w.kp, n, hp, umax, w.dir, w.angle, st); }));
        SVO_HIP(ctx, tl.run(&time_ms[2],
                            [&] { return launch_orb_brief(w.blurred, w.kp, n, w.pat, w.dir, reach, w.desc, st); }));
    }
    std::vector<uint8_t> hd((size_t)SVO_ORB_DESC_BYTES * n);
    std::vector<float> ha(n);
    SVO_HIP(ctx, hipMemcpyAsync(hd.data(), w.desc, hd.size(), hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(ha.data(), w.angle, sizeof(float) * n, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));  // also: hk and pat have left the host
    std::memcpy(desc, hd.data(), hd.size());
    std::memcpy(valid, hv.data(), n);
    if (angle) std::memcpy(angle, ha.data(), sizeof(float) * n);
    return SVO_OK;
}

}  // namespace

extern "C" int svo_orb_default_pattern(int patch_size, int8_t pattern_xy[1024]) {
    if (!pattern_xy || !patch_ok(patch_size)) return SVO_ERR_ARG;
    default_pattern(patch_size / 2, pattern_xy);
    return SVO_OK;
}

extern "C" int svo_orb_umax(int patch_size, int* umax, int cap, int* n) {
    if (!patch_ok(patch_size) || cap < 0 || (!umax && cap > 0)) return SVO_ERR_ARG;
    const int hp = patch_size / 2;
    int u[16];
    orb_umax(hp, u);
    for (int v = 0; v <= hp && v < cap; v++) umax[v] = u[v];
    if (n) *n = hp + 1;
    return SVO_OK;
}

extern "C" int svo_orb_compute(svo_ctx* ctx, const svo_image* img, const svo_orb_params* prm, const int8_t* pattern_xy,
                               const svo_keypoint* kp, const int* octave, int n, uint8_t* desc, float* angle,
                               uint8_t* valid) {
    if (!ctx || !img || !prm || n < 0 || (n > 0 && (!kp || !octave || !desc || !valid)))
        return set_error(ctx, SVO_ERR_ARG, "svo_orb_compute: bad arguments");
    int8_t pat[2 * kOrbPatternPoints];
    if (const char* why = check_describe(prm, pattern_xy, pat))
        return set_error(ctx, SVO_ERR_ARG, "svo_orb_compute: %s", why);
    for (int i = 0; i < n; i++)
        if (octave[i] < 0 || octave[i] >= prm->nlevels)
            return set_error(ctx, SVO_ERR_ARG, "svo_orb_compute: octave %d of keypoint %d outside [0, nlevels)",
                             octave[i], i);
    OrbLevels o;
    const int rc = orb_build_levels(ctx, img, prm, nullptr, "svo_orb_compute", o);
    if (rc != SVO_OK) return rc;
    return describe_levels(ctx, prm, o, pat, kp, octave, n, desc, angle, valid, "svo_orb_compute");
}

extern "C" int svo_orb_detect_and_compute(svo_ctx* ctx, const svo_image* img, const svo_orb_params* prm,
                                          const uint8_t* mask, const int8_t* pattern_xy, svo_keypoint* kp, int* octave,
                                          uint8_t* desc, float* angle, uint8_t* valid, int cap, int* n_out) {
    if (!ctx || !img || !prm || cap < 0 || (cap > 0 && (!kp || !desc || !valid)))
        return set_error(ctx, SVO_ERR_ARG, "svo_orb_detect_and_compute: bad arguments");
    int8_t pat[2 * kOrbPatternPoints];
    if (const char* why = check_describe(prm, pattern_xy, pat))
        return set_error(ctx, SVO_ERR_ARG, "svo_orb_detect_and_compute: %s", why);
    OrbLevels o;
    int rc = orb_build_levels(ctx, img, prm, mask, "svo_orb_detect_and_compute", o);
    if (rc != SVO_OK) return rc;
    std::vector<int> own;  // the octaves, when the caller does not ask for them
    if (!octave) {
        own.resize(cap > 0 ? cap : 1);
        octave = own.data();
    }
    int n = 0;
    rc = orb_detect_levels(ctx, prm, o, kp, octave, cap, &n);
    if (rc != SVO_OK) return rc;
    if (n_out) *n_out = n;
    // the pyramid detection ran on is still in the workspace: describe from it
    return describe_levels(ctx, prm, o, pat, kp, octave, n < cap ? n : cap, desc, angle, valid,
                           "svo_orb_detect_and_compute");
}

extern "C" int svo_orb_blur_level(svo_ctx* ctx, const svo_image* img, const svo_orb_params* prm, int level,
                                  uint8_t* out, int* lw, int* lh) {
    if (!ctx || !img || !prm || !out) return set_error(ctx, SVO_ERR_ARG, "svo_orb_blur_level: bad arguments");
    if (level < 0 || level >= prm->nlevels) return set_error(ctx, SVO_ERR_ARG, "svo_orb_blur_level: no such level");
    OrbLevels o;
    int rc = orb_build_levels(ctx, img, prm, nullptr, "svo_orb_blur_level", o);
    if (rc != SVO_OK) return rc;
    DescWork w;
    rc = blur_levels(ctx, o, 0, "svo_orb_blur_level", w);
    if (rc != SVO_OK) return rc;
    const ImgLevel& L = w.blurred.lv[level];
    SVO_HIP(ctx, hipMemcpy2DAsync(out, L.w, L.data, L.pitch, L.w, L.h, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (lw) *lw = L.w;
    if (lh) *lh = L.h;
    return SVO_OK;
}

namespace {

// svo_match_hamming, and with time_reps > 0 svo_match_hamming_time: the launch
// again `reps` times between events instead of the download
int match_run(svo_ctx* ctx, int n_problems, const int* nq, const int* nt, int q_stride, int t_stride,
              const uint8_t* q, const uint8_t* t, int* idx, int* dist, const char* who, int time_reps, double* time_ms) {
    if (!ctx || n_problems < 0 || n_problems > 65535 || q_stride < 0 || t_stride < 0)
        return set_error(ctx, SVO_ERR_ARG, "%s: bad arguments", who);
    if (n_problems == 0) return SVO_OK;
    if (!nq || !nt) return set_error(ctx, SVO_ERR_ARG, "%s: null counts", who);
    int max_nq = 0;
    for (int p = 0; p < n_problems; p++) {
        if (nq[p] < 0 || nq[p] > q_stride || nt[p] < 0 || nt[p] > t_stride)
            return set_error(ctx, SVO_ERR_ARG, "%s: counts of problem %d outside [0, stride]", who, p);
        max_nq = nq[p] > max_nq ? nq[p] : max_nq;
    }
    if (max_nq == 0) return SVO_OK;
    if (!q || (!time_reps && (!idx || !dist)) || (!t && t_stride > 0))
        return set_error(ctx, SVO_ERR_ARG, "%s: null arrays", who);
    hipStream_t st = ctx->stream;
    const size_t P = (size_t)n_problems;
    const size_t qb = P * q_stride * SVO_ORB_DESC_BYTES, tb = P * t_stride * SVO_ORB_DESC_BYTES;
    const size_t ob = sizeof(int) * 2 * P * q_stride;
    uint32_t *dq, *dt;
    int *dnq, *dnt, *didx, *ddist;
    if (!carve_scratch(ctx, kScratchDescribe, [&](Carver& c) {
            dq = c.take<uint32_t>(qb / 4);
            dt = c.take<uint32_t>(tb / 4);
            dnq = c.take<int>(P);
            dnt = c.take<int>(P);
            didx = c.take<int>(2 * P * q_stride);
            ddist = c.take<int>(2 * P * q_stride);
        }))
        return set_error(ctx, SVO_ERR_HIP, "%s: workspace alloc failed", who);
    SVO_HIP(ctx, hipMemcpyAsync(dq, q, qb, hipMemcpyHostToDevice, st));
    if (tb) SVO_HIP(ctx, hipMemcpyAsync(dt, t, tb, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(dnq, nq, sizeof(int) * P, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(dnt, nt, sizeof(int) * P, hipMemcpyHostToDevice, st));
    auto launch = [&] {
        return launch_hamming_knn2(dq, dt, dnq, dnt, q_stride, t_stride, n_problems, max_nq, didx, ddist, st);
    };
    SVO_HIP(ctx, launch());
    if (time_reps > 0) {
        TimedLoop tl(ctx, time_reps);
        SVO_HIP(ctx, tl.run(time_ms, launch));
        SVO_HIP(ctx, hipStreamSynchronize(st));
        return SVO_OK;
    }
    // only the rows of live queries reach the caller: the padding up to the stride stays as it was
    std::vector<int> hi(2 * P * q_stride), hd(2 * P * q_stride);
    SVO_HIP(ctx, hipMemcpyAsync(hi.data(), didx, ob, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(hd.data(), ddist, ob, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    for (size_t p = 0; p < P; p++) {
        const size_t at = 2 * p * q_stride;
        std::memcpy(idx + at, hi.data() + at, sizeof(int) * 2 * nq[p]);
        std::memcpy(dist + at, hd.data() + at, sizeof(int) * 2 * nq[p]);
    }
    return SVO_OK;
}

}  // namespace

extern "C" int svo_match_hamming(svo_ctx* ctx, int n_problems, const int* nq, const int* nt, int q_stride,
                                 int t_stride, const uint8_t* q, const uint8_t* t, int* idx, int* dist) {
    return match_run(ctx, n_problems, nq, nt, q_stride, t_stride, q, t, idx, dist, "svo_match_hamming", 0, nullptr);
}

extern "C" int svo_match_hamming_time(svo_ctx* ctx, int n_problems, const int* nq, const int* nt, int q_stride,
                                      int t_stride, const uint8_t* q, const uint8_t* t, int reps, double* ms) {
    if (reps < 1 || !ms) return set_error(ctx, SVO_ERR_ARG, "svo_match_hamming_time: bad arguments");
    *ms = 0.0;
    return match_run(ctx, n_problems, nq, nt, q_stride, t_stride, q, t, nullptr, nullptr, "svo_match_hamming_time",
                     reps, ms);
}

extern "C" int svo_orb_describe_time(svo_ctx* ctx, const svo_image* img, const svo_orb_params* prm, int cap, int reps,
                                     double ms[3], int* n_kp) {
    if (!ctx || !img || !prm || cap < 1 || reps < 1 || !ms)
        return set_error(ctx, SVO_ERR_ARG, "svo_orb_describe_time: bad arguments");
    int8_t pat[2 * kOrbPatternPoints];
    if (const char* why = check_describe(prm, nullptr, pat))
        return set_error(ctx, SVO_ERR_ARG, "svo_orb_describe_time: %s", why);
    OrbLevels o;
    int rc = orb_build_levels(ctx, img, prm, nullptr, "svo_orb_describe_time", o);
    if (rc != SVO_OK) return rc;
    std::vector<svo_keypoint> kp(cap);
    std::vector<int> octave(cap);
    int n = 0;
    rc = orb_detect_levels(ctx, prm, o, kp.data(), octave.data(), cap, &n);
    if (rc != SVO_OK) return rc;
    n = n < cap ? n : cap;
    if (n_kp) *n_kp = n;
    ms[0] = ms[1] = ms[2] = 0.0;
    std::vector<uint8_t> desc((size_t)SVO_ORB_DESC_BYTES * (n > 0 ? n : 1)), valid(n > 0 ? n : 1);
    return describe_levels(ctx, prm, o, pat, kp.data(), octave.data(), n, desc.data(), nullptr, valid.data(),
                           "svo_orb_describe_time", reps, ms);
}

extern "C" int svo_match_filter(const int* idx_qt, const int* dist_qt, int nq, const int* idx_tq, int nt,
                                int ratio_pct, int* pairs, int cap, int* n_out) {
    if (nq < 0 || nt < 0 || cap < 0 || ratio_pct < 0 || (nq > 0 && (!idx_qt || !dist_qt)) || (!pairs && cap > 0))
        return SVO_ERR_ARG;
    for (int q = 0; q < nq; q++)  // nothing is written on a bad index
        if (idx_qt[2 * q] >= nt || idx_qt[2 * q + 1] >= nt) return SVO_ERR_ARG;
    int n = 0;
    for (int q = 0; q < nq; q++) {
        const int i1 = idx_qt[2 * q], i2 = idx_qt[2 * q + 1];
        if (i1 < 0) continue;
        if (ratio_pct != 0 &&
            !(i2 >= 0 && (long long)dist_qt[2 * q] * 100 < (long long)ratio_pct * dist_qt[2 * q + 1]))
            continue;
        if (idx_tq && idx_tq[2 * i1] != q) continue;
        if (n < cap) {
            pairs[2 * n] = q;
            pairs[2 * n + 1] = i1;
        }
        n++;
    }
    if (n_out) *n_out = n;
    return SVO_OK;
}

extern "C" int svo_match_filter_batch(svo_ctx* ctx, int n_problems, const int* nq, const int* nt, int q_stride,
                                      int t_stride, const int* idx_qt, const int* dist_qt, const int* idx_tq,
                                      int ratio_pct, int* pairs, int* n_pairs) {
    const char* who = "svo_match_filter_batch";
    if (!ctx || n_problems < 0 || n_problems > 65535 || q_stride < 0 || t_stride < 0 || ratio_pct < 0)
        return set_error(ctx, SVO_ERR_ARG, "%s: bad arguments", who);
    if (n_problems == 0) return SVO_OK;
    if (!nq || !nt || !n_pairs) return set_error(ctx, SVO_ERR_ARG, "%s: null counts", who);
    const size_t P = (size_t)n_problems;
    int max_nq = 0;
    for (size_t p = 0; p < P; p++) {
        if (nq[p] < 0 || nq[p] > q_stride || nt[p] < 0 || nt[p] > t_stride)
            return set_error(ctx, SVO_ERR_ARG, "%s: counts of problem %zu outside [0, stride]", who, p);
        max_nq = nq[p] > max_nq ? nq[p] : max_nq;
    }
    if (max_nq > 0 && (!idx_qt || !dist_qt || !pairs)) return set_error(ctx, SVO_ERR_ARG, "%s: null arrays", who);
    for (size_t p = 0; p < P; p++)  // nothing is written on a bad index
        for (int q = 0; q < nq[p]; q++) {
            const int* i = idx_qt + 2 * (p * q_stride + q);
            if (i[0] >= nt[p] || i[1] >= nt[p])
                return set_error(ctx, SVO_ERR_ARG, "%s: an index of problem %zu is not below its train count", who, p);
        }
    if (max_nq == 0) {
        std::memset(n_pairs, 0, sizeof(int) * P);
        return SVO_OK;
    }
    hipStream_t st = ctx->stream;
    const size_t qn = 2 * P * q_stride, tn = idx_tq ? 2 * P * t_stride : 0;
    int *dqt, *ddq, *dtq, *dnq, *dnt, *dpairs, *dnp;
    if (!carve_scratch(ctx, kScratchDescribe, [&](Carver& c) {
            dqt = c.take<int>(qn);
            ddq = c.take<int>(qn);
            dtq = c.take<int>(tn);
            dnq = c.take<int>(P);
            dnt = c.take<int>(P);
            dpairs = c.take<int>(qn);
            dnp = c.take<int>(P);
        }))
        return set_error(ctx, SVO_ERR_HIP, "%s: workspace alloc failed", who);
    SVO_HIP(ctx, hipMemcpyAsync(dqt, idx_qt, sizeof(int) * qn, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(ddq, dist_qt, sizeof(int) * qn, hipMemcpyHostToDevice, st));
    if (tn) SVO_HIP(ctx, hipMemcpyAsync(dtq, idx_tq, sizeof(int) * tn, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(dnq, nq, sizeof(int) * P, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(dnt, nt, sizeof(int) * P, hipMemcpyHostToDevice, st));
    // (t_stride 0 with a cross-check: every nt is 0 and nothing passes the index test)
    SVO_HIP(ctx, launch_match_filter(dqt, ddq, tn ? dtq : nullptr, dnq, dnt, q_stride, t_stride, n_problems,
                                     ratio_pct, dpairs, dnp, st));
    std::vector<int> hp(qn), hn(P);
    SVO_HIP(ctx, hipMemcpyAsync(hp.data(), dpairs, sizeof(int) * qn, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(hn.data(), dnp, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    // only the rows of kept pairs reach the caller: the padding up to the stride stays as it was
    for (size_t p = 0; p < P; p++) {
        n_pairs[p] = hn[p];
        std::memcpy(pairs + 2 * p * q_stride, hp.data() + 2 * p * q_stride, sizeof(int) * 2 * hn[p]);
    }
    return SVO_OK;
}
