// The rest of the batched front end's C ABI: synchronize and the readbacks, the
// observation window and its bundle adjustment, level readbacks, the timing
// probes and the phase-timing ring.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ba.hpp"
#include "frontend_state.hpp"
#include "pose_refine.hpp"

namespace svo {

// Phase timing: event pairs from a ring; a pair is folded into the totals once
// its end event has completed (work that runs into the next step is collected
// then), so timing never adds a synchronisation.
void ph_fold(svo_frontend* fe, bool wait) {
    std::vector<std::pair<int, int>> keep;
    for (auto& p : fe->pending) {
        if (wait) (void)hipEventSynchronize(fe->ev[p.second + 1]);
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, fe->ev[p.second], fe->ev[p.second + 1]);
        if (e == hipSuccess) {
            fe->phase_ms[p.first] += ms;
            fe->phase_n[p.first] += 1;
        } else if (e == hipErrorNotReady) {
            keep.push_back(p);
        }
    }
    fe->pending.swap(keep);
}

void ph_begin(svo_frontend* fe, int ph, hipStream_t st, int* slot) {
    *slot = -1;
    if (!fe->cfg.timing) return;
    // timing 2: only the big phases (each event pair costs a few us of host time)
    if (fe->cfg.timing == 2 && ph != PH_LK && ph != PH_PYR && ph != PH_FAST && ph != PH_STEREO && ph != PH_PYR_R)
        return;
    if (fe->cfg.timing == 3 && ph != PH_LK) return;  // timing 3: the LK launches only (the roofline's)
    const int sl = fe->ev_used;
    bool wrapped = false;  // ring wrapped onto a pair still in flight
    for (const auto& p : fe->pending) wrapped |= p.second == sl;
    if (wrapped) ph_fold(fe, true);
    fe->ev_used = (fe->ev_used + 2) % kEvRing;
    *slot = sl;
    (void)hipEventRecord(fe->ev[sl], st);
    fe->pending.push_back({ph, sl});
}

void ph_end(svo_frontend* fe, hipStream_t st, int slot) {
    if (slot >= 0) (void)hipEventRecord(fe->ev[slot + 1], st);
}

}  // namespace svo

using namespace svo;

// the recorded slots, oldest first
static WindowOrder fe_window_order(const svo_frontend* fe) {
    WindowOrder o{};
    o.n = std::min(fe->win.count, fe->win.slots);
    for (int i = 0; i < o.n; i++) o.slot[i] = (fe->win.count - o.n + i) % fe->win.slots;
    return o;
}

// one timed run of `launch` on the context stream: a warm-up, then reps launches
// between two events
template <class F>
static int fe_time_launches(svo_ctx* ctx, int reps, double* ms_per_launch, F launch) {
    hipEvent_t e0, e1;
    SVO_HIP(ctx, hipEventCreate(&e0));
    SVO_HIP(ctx, hipEventCreate(&e1));
    SVO_HIP(ctx, launch());  // untimed first (caches warm, identical contents)
    SVO_HIP(ctx, hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < reps; i++) SVO_HIP(ctx, launch());
    SVO_HIP(ctx, hipEventRecord(e1, ctx->stream));
    SVO_HIP(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    SVO_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_launch = ms / reps;
    return SVO_OK;
}

extern "C" {

int svo_frontend_synchronize(svo_frontend* fe) {
    if (!fe) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    int rq = fe_queue_stats(fe);
    if (rq) return rq;
    for (hipStream_t st : {fe->st_lk, fe->st_fast, fe->st_copy, ctx->stream}) SVO_HIP(ctx, hipStreamSynchronize(st));
    fe_finish_fits(fe);
    // the last keyframe's map points to the world frame (the next post-LK finds
    // nothing pending then)
    SVO_HIP(ctx, launch_finalize_map(fe_pending(fe), fe->S, ctx->stream));
    // (the place memory's newest record takes its points now: they are final)
    int rp = fe_places_flush(fe, ctx->stream);
    if (rp) return rp;
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

int svo_frontend_pose(svo_frontend* fe, int seq, double rvec[3], double tvec[3]) {
    if (!fe || seq < 0 || seq >= fe->S) return SVO_ERR_ARG;
    int rq = fe_queue_stats(fe);
    if (rq) return rq;
    fe_finish_fits(fe);
    std::memcpy(rvec, &fe->pose[6 * (size_t)seq], sizeof(double) * 3);
    std::memcpy(tvec, &fe->pose[6 * (size_t)seq + 3], sizeof(double) * 3);
    return SVO_OK;
}

int svo_frontend_features(svo_frontend* fe, int seq, float* xy, int cap, int* n) {
    if (!fe || seq < 0 || seq >= fe->S) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    int cnt = 0;
    SVO_HIP(ctx, hipMemcpyAsync(&cnt, fe->nA + seq, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int k = std::min(cnt, cap);
    if (k > 0 && xy) {
        SVO_HIP(ctx, hipMemcpyAsync(xy, fe->xyA + 2 * (size_t)seq * fe->CAP, sizeof(float) * 2 * k,
                                    hipMemcpyDeviceToHost, ctx->stream));
        SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (n) *n = cnt;
    return SVO_OK;
}

int svo_frontend_map_points(svo_frontend* fe, int seq, double* xyz, int cap, int* n) {
    if (!fe || seq < 0 || seq >= fe->S || cap < 0 || (cap > 0 && !xyz)) return SVO_ERR_ARG;
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    svo_ctx* ctx = fe->ctx;
    int cnt = 0, mn = 0;
    SVO_HIP(ctx, hipMemcpyAsync(&cnt, fe->nA + seq, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(ctx, hipMemcpyAsync(&mn, fe->map_n + seq, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> mid((size_t)cnt);
    std::vector<double> map(3 * (size_t)mn);
    if (cnt > 0)
        SVO_HIP(ctx, hipMemcpyAsync(mid.data(), fe->midA + (size_t)seq * fe->CAP, sizeof(int) * cnt,
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (mn > 0)
        SVO_HIP(ctx, hipMemcpyAsync(map.data(), fe->map + 3 * (size_t)seq * fe->MAPCAP, sizeof(double) * 3 * mn,
                                    hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < std::min(cnt, cap); i++) {
        if (mid[i] < 0 || mid[i] >= mn) return set_error(ctx, SVO_ERR_HIP, "svo_frontend_map_points: bad map id");
        std::memcpy(xyz + 3 * (size_t)i, &map[3 * (size_t)mid[i]], sizeof(double) * 3);
    }
    if (n) *n = cnt;
    return SVO_OK;
}

// the rig's baseline from the rectified projection matrices: P_right = K [I | (-b, 0, 0)]
static double fe_baseline(const svo_frontend* fe) {
    return -(double)fe->cfg.P_right[3] / (double)fe->cfg.P_right[0];
}

// svo_frontend_window_enable, and with the right columns svo_frontend_window_enable_stereo
static int fe_window_enable(svo_frontend* fe, int window, bool stereo) {
    if (!fe) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    FeWindow& w = fe->win;
    if (window < 1 || window > SVO_BA_MAX_CAMS)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_window_enable: window outside 1 .. SVO_BA_MAX_CAMS");
    if (fe->ahead.stepped >= 0 || w.slots)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_window_enable: once, before svo_frontend_init");
    if (stereo && !(std::isfinite(fe_baseline(fe)) && fe_baseline(fe) > 0))
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_window_enable_stereo: P_right gives no baseline > 0");
    const size_t S = fe->S, Wn = window, CAP = fe->CAP;
    auto layout = [&](Carver& p) {
        w.ring.n = p.take<int>(S * Wn);
        w.ring.epoch = p.take<int>(S * Wn);
        w.ring.xy = p.take<float>(2 * S * Wn * CAP);
        w.ring.mid = p.take<int>(S * Wn * CAP);
        w.ring.map_epoch = p.take<int>(S);
        w.sel_slot = p.take<int>(S * Wn);
        w.sel_cnt = p.take<int>(S * Wn);
        w.sel_nc = p.take<int>(S);
        w.ring.ur = stereo ? p.take<float>(S * Wn * CAP) : nullptr;
        w.ur_feat = stereo ? p.take<float>(S * CAP) : nullptr;
    };
    const size_t bytes = layout_bytes(layout);  // (leaves every pointer null)
    if (hipMalloc(&w.mem, bytes) != hipSuccess) {
        w.mem = nullptr;
        return set_error(ctx, SVO_ERR_HIP, "svo_frontend_window_enable: hipMalloc(%zu)", bytes);
    }
    layout_place(w.mem, layout);
    w.ring.window = window;
    w.ring.cap = fe->CAP;
    if (hipHostMalloc((void**)&w.h_pose, sizeof(double) * 12 * S * Wn, hipHostMallocCoherent | hipHostMallocMapped) !=
        hipSuccess) {
        (void)hipFree(w.mem);
        w.mem = nullptr;
        w.h_pose = nullptr;
        w.ring = WindowRing{};
        w.ur_feat = nullptr;
        return set_error(ctx, SVO_ERR_HIP, "svo_frontend_window_enable: host-coherent poses");
    }
    std::memset(w.h_pose, 0, sizeof(double) * 12 * S * Wn);
    SVO_HIP(ctx, hipMemsetAsync(w.mem, 0, bytes, ctx->stream));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    w.frame.assign(Wn, -1);
    w.count = 0;
    w.slots = window;
    return SVO_OK;
}

int svo_frontend_window_enable(svo_frontend* fe, int window) { return fe_window_enable(fe, window, false); }

int svo_frontend_window_enable_stereo(svo_frontend* fe, int window) { return fe_window_enable(fe, window, true); }

int svo_frontend_window(svo_frontend* fe, int seq, int cap, int* n_frames, int* frame_t, double* poses, int* counts,
                        int* ids, float* xy) {
    if (!fe || seq < 0 || seq >= fe->S || cap < 0) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    const FeWindow& w = fe->win;
    if (!w.slots) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_window: no window enabled");
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    const size_t Wn = w.slots, CAP = fe->CAP;
    std::vector<int> n(Wn), ep(Wn);
    int cur = 0;
    hipStream_t st = ctx->stream;
    SVO_HIP(ctx, hipMemcpyAsync(n.data(), w.ring.n + seq * Wn, sizeof(int) * Wn, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(ep.data(), w.ring.epoch + seq * Wn, sizeof(int) * Wn, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(&cur, w.ring.map_epoch + seq, sizeof(int), hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    const WindowOrder o = fe_window_order(fe);
    int v = 0;
    for (int i = 0; i < o.n; i++) {
        const int sl = o.slot[i];
        if (ep[sl] != cur) continue;  // recorded before the map's last reclaim
        const int k = std::min(n[sl], cap);
        const size_t src = (seq * Wn + sl) * CAP;
        if (frame_t) frame_t[v] = w.frame[sl];
        if (counts) counts[v] = k;
        if (poses) std::memcpy(poses + 12 * (size_t)v, w.h_pose + 12 * (seq * Wn + sl), sizeof(double) * 12);
        if (ids && k > 0)
            SVO_HIP(ctx, hipMemcpyAsync(ids + (size_t)v * cap, w.ring.mid + src, sizeof(int) * k, hipMemcpyDeviceToHost, st));
        if (xy && k > 0)
            SVO_HIP(ctx, hipMemcpy(xy + 2 * (size_t)v * cap, w.ring.xy + 2 * src, sizeof(float) * 2 * k,
                                   hipMemcpyDeviceToHost));
        v++;
    }
    SVO_HIP(ctx, hipStreamSynchronize(st));
    if (n_frames) *n_frames = v;
    return SVO_OK;
}

int svo_frontend_window_right(svo_frontend* fe, int seq, int cap, float* ur) {
    if (!fe || seq < 0 || seq >= fe->S || cap < 0) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    const FeWindow& w = fe->win;
    if (!w.ring.ur) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_window_right: no stereo window enabled");
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    const size_t Wn = w.slots, CAP = fe->CAP;
    std::vector<int> n(Wn), ep(Wn);
    int cur = 0;
    hipStream_t st = ctx->stream;
    SVO_HIP(ctx, hipMemcpyAsync(n.data(), w.ring.n + seq * Wn, sizeof(int) * Wn, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(ep.data(), w.ring.epoch + seq * Wn, sizeof(int) * Wn, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(&cur, w.ring.map_epoch + seq, sizeof(int), hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    const WindowOrder o = fe_window_order(fe);
    int v = 0;
    for (int i = 0; i < o.n; i++) {  // svo_frontend_window's walk
        const int sl = o.slot[i];
        if (ep[sl] != cur) continue;
        const int k = std::min(n[sl], cap);
        if (ur && k > 0)
            SVO_HIP(ctx, hipMemcpyAsync(ur + (size_t)v * cap, w.ring.ur + (seq * Wn + sl) * CAP, sizeof(float) * k,
                                        hipMemcpyDeviceToHost, st));
        v++;
    }
    SVO_HIP(ctx, hipStreamSynchronize(st));
    return SVO_OK;
}

// svo_frontend_bundle_adjust, and with the ring's right columns svo_frontend_bundle_adjust_stereo
static int fe_bundle_adjust(svo_frontend* fe, bool stereo, int n_fixed, double huber_delta, int max_iterations,
                            double* costs, int* iterations, int* sizes) {
    if (!fe) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    const FeWindow& w = fe->win;
    if (!w.slots) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_bundle_adjust: no window enabled");
    if (stereo && !w.ring.ur)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_bundle_adjust_stereo: no stereo window enabled");
    if (n_fixed < 0 || max_iterations < 0)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_bundle_adjust: n_fixed / max_iterations < 0");
    // the newest frame's pose lands and its keyframe's points reach the world frame
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    SVO_HIP(ctx, launch_window_select(w.ring, fe_window_order(fe), fe->S, w.sel_slot, w.sel_cnt, w.sel_nc, ctx->stream));
    BaDeviceWindow bw;
    bw.lists = BaLists{fe->S, w.slots, fe->CAP, w.sel_slot, w.sel_cnt, w.ring.mid, w.ring.xy};
    bw.n_cams = w.sel_nc;
    bw.ring = w.h_pose;
    bw.map = fe->map;
    bw.map_cap = fe->MAPCAP;
    bw.n_fixed = n_fixed;
    if (stereo) {
        bw.lists.ur = w.ring.ur;
        bw.baseline = fe_baseline(fe);
    }
    return ba_adjust_device(ctx, bw, fe->cfg.K, huber_delta, max_iterations, costs, iterations, sizes);
}

int svo_frontend_bundle_adjust(svo_frontend* fe, int n_fixed, double huber_delta, int max_iterations, double* costs,
                               int* iterations, int* sizes) {
    return fe_bundle_adjust(fe, false, n_fixed, huber_delta, max_iterations, costs, iterations, sizes);
}

int svo_frontend_bundle_adjust_stereo(svo_frontend* fe, int n_fixed, double huber_delta, int max_iterations,
                                      double* costs, int* iterations, int* sizes) {
    return fe_bundle_adjust(fe, true, n_fixed, huber_delta, max_iterations, costs, iterations, sizes);
}

int svo_frontend_refine_poses(svo_frontend* fe, double huber_delta, int max_iterations, double* costs,
                              int* iterations, int* counts) {
    if (!fe) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    const FeWindow& w = fe->win;
    if (!w.slots) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_refine_poses: no window enabled");
    if (max_iterations < 0 || max_iterations > SVO_REFINE_MAX_ITERATIONS)
        return set_error(ctx, SVO_ERR_ARG,
                         "svo_frontend_refine_poses: max_iterations outside 0 .. SVO_REFINE_MAX_ITERATIONS");
    // the newest frame's pose lands and its keyframe's points reach the world frame
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    SVO_HIP(ctx, launch_window_select(w.ring, fe_window_order(fe), fe->S, w.sel_slot, w.sel_cnt, w.sel_nc, st));
    // the results: [S][2] costs, [S] iterations, [S] counts, one block and one download
    const size_t S = (size_t)fe->S, bytes = S * (2 * sizeof(double) + 2 * sizeof(int));
    char* d = (char*)scratch(ctx, kScratchRefine, bytes);
    if (!d) return set_error(ctx, SVO_ERR_HIP, "scratch alloc");
    PoseRefineBatch b;
    b.P = fe->S;
    b.cap = fe->CAP;
    b.poses_in = b.poses_out = w.h_pose;
    b.sel_slot = w.sel_slot;
    b.sel_cnt = w.sel_cnt;
    b.sel_nc = w.sel_nc;
    b.window = w.slots;
    b.map = fe->map;
    b.map_cap = fe->MAPCAP;
    b.ids = w.ring.mid;
    b.xy = w.ring.xy;
    b.ur = w.ring.ur;  // (null with the plain window: every observation monocular)
    const double* K = fe->cfg.K;
    b.fx = K[0], b.fy = K[4], b.cx = K[2], b.cy = K[5];
    b.baseline = w.ring.ur ? fe_baseline(fe) : 1.0;
    b.delta = huber_delta;
    b.max_iterations = max_iterations;
    b.costs = (double*)d;
    b.iterations = (int*)(d + 2 * sizeof(double) * S);
    b.n_used = b.iterations + S;
    SVO_HIP(ctx, launch_pose_refine(b, st));
    std::vector<char> h(bytes);
    SVO_HIP(ctx, hipMemcpyAsync(h.data(), d, bytes, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    const char* its = h.data() + 2 * sizeof(double) * S;
    if (costs) std::memcpy(costs, h.data(), 2 * sizeof(double) * S);
    if (iterations) std::memcpy(iterations, its, sizeof(int) * S);
    if (counts) std::memcpy(counts, its + sizeof(int) * S, sizeof(int) * S);
    return SVO_OK;
}

int svo_frontend_scharr_level(svo_frontend* fe, int seq, int t, int level, int16_t* ix, int16_t* iy, int stride) {
    if (!fe || seq < 0 || seq >= fe->S || t < 0 || level < 0 || level >= fe->nlev) return SVO_ERR_ARG;
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    svo_ctx* ctx = fe->ctx;
    const ImgLevel& L = fe->desc_host[(size_t)(t % fe->T) * fe->S + seq].lv[level];
    if (stride < L.w) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_scharr_level: stride");
    DerivDesc dd;
    SVO_HIP(ctx, hipMemcpy(&dd, fe->d_der + (size_t)(t % 3) * fe->S + seq, sizeof(dd), hipMemcpyDeviceToHost));
    return download_deriv_level(ctx, dd, level, L.w, L.h, ix, iy, stride);
}

int svo_frontend_pyramid_level(svo_frontend* fe, int seq, int t, int right, int level, uint8_t* out, int stride) {
    static_assert(SVO_PYR_PAD == kPyrPad, "header border width");
    if (!fe || seq < 0 || seq >= fe->S || t < 0 || level < 0 || level >= fe->nlev || !out) return SVO_ERR_ARG;
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    svo_ctx* ctx = fe->ctx;
    const ImgLevel& L = (right ? fe->desc_r_host : fe->desc_host)[(size_t)(t % fe->T) * fe->S + seq].lv[level];
    const int bw = L.w + 2 * kPyrPad;
    if (stride < bw) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_pyramid_level: stride");
    SVO_HIP(ctx, hipMemcpy2D(out, stride, L.data - (ptrdiff_t)kPyrPad * L.pitch - kPyrPad, L.pitch, bw,
                             L.h + 2 * kPyrPad, hipMemcpyDeviceToHost));
    return SVO_OK;
}

int svo_frontend_time_pyramid(svo_frontend* fe, int t, int reps, double* ms_per_launch) {
    if (!fe || t < 0 || reps <= 0 || !ms_per_launch) return SVO_ERR_ARG;
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    svo_ctx* ctx = fe->ctx;
    const int S = fe->S;
    const PyrDesc* d = fe->d_desc + (size_t)(t % fe->T) * S;
    const DerivDesc* dd = fe->d_der + (size_t)(t % 3) * S;
    rc = fe_time_launches(ctx, reps, ms_per_launch, [&]() {
        return launch_pyramid_scharr_batched(d, dd, S, fe->W, fe->H, fe->nlev, ctx->stream);
    });
    if (rc) return rc;
    fe->ahead.pyr_ready = -1;
    return SVO_OK;
}

int svo_frontend_time_ingest(svo_frontend* fe, int t, int rectify, int reps, double* ms_per_launch) {
    if (!fe || t < 0 || reps <= 0 || !ms_per_launch) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    const FeUpload& up = fe->up;
    if (!up.stage || !up.stride) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_time_ingest: no frames were queued");
    if (rectify && !fe->rect[0]) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_time_ingest: no rectification set");
    if (!rectify && (fe->raw_w < fe->W || fe->raw_h < fe->H))
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_time_ingest: the staged frames are smaller than the config's");
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    SVO_HIP(ctx, hipStreamSynchronize(up.st));
    const int S = fe->S;
    const PyrDesc* d = fe->d_desc + (size_t)(t % fe->T) * S;
    rc = fe_time_launches(ctx, reps, ms_per_launch, [&]() {
        return rectify ? launch_rectify_batched(up.stage, up.seq, up.stride, fe->rect[0]->dev, d, S, up.bgr != 0,
                                                ctx->stream)
                       : launch_ingest_batched(up.stage, up.seq, up.stride, d, S, fe->W, fe->H, up.bgr != 0,
                                               ctx->stream);
    });
    if (rc) return rc;
    fe->ahead.forget_slot(t % fe->T, fe->T);  // the slot's level 0 was rewritten
    return SVO_OK;
}

int svo_frontend_time_fast(svo_frontend* fe, int t, int reps, double* ms_per_launch) {
    if (!fe || t < 0 || reps <= 0 || !ms_per_launch) return SVO_ERR_ARG;
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    svo_ctx* ctx = fe->ctx;
    const PyrDesc* d = fe->d_desc + (size_t)(t % fe->T) * fe->S;
    const FastDetBatch fb = fe_fast_batch(fe, d, false);
    rc = fe_time_launches(ctx, reps, ms_per_launch, [&]() {
        return launch_fast_detect(fb, fe->S, fe->W, fe->H, fe->cfg.fast_threshold, fe->cfg.fast_nonmax, ctx->stream,
                                  kFastDetect);
    });
    if (rc) return rc;
    fe->ahead.pre_t = -1;  // the row words now hold frame t's unmasked detection, not a queued one
    return SVO_OK;
}

int svo_frontend_host_cpus(svo_frontend* fe, int* cpus, int cap, int* n) {
    if (!fe || cap < 0 || (cap > 0 && !cpus)) return SVO_ERR_ARG;
    for (int i = 0; i < (int)fe->host_cpus.size() && i < cap; i++) cpus[i] = fe->host_cpus[i];
    if (n) *n = (int)fe->host_cpus.size();
    return SVO_OK;
}

int svo_frontend_streams(svo_frontend* fe, void** streams, int cap, int* n) {
    if (!fe || cap < 0 || (cap > 0 && !streams)) return SVO_ERR_ARG;
    const hipStream_t st[3] = {fe->st_lk, fe->st_fast, fe->st_copy};
    for (int i = 0; i < 3 && i < cap; i++) streams[i] = (void*)st[i];
    if (n) *n = 3;
    return SVO_OK;
}

int svo_frontend_phase_times(svo_frontend* fe, double* ms, int64_t* launches, int cap) {
    if (!fe) return SVO_ERR_ARG;
    ph_fold(fe, true);
    for (int i = 0; i < kPhases && i < cap; i++) {
        if (ms) ms[i] = fe->phase_ms[i];
        if (launches) launches[i] = fe->phase_n[i];
    }
    return kPhases;
}

void svo_frontend_reset_times(svo_frontend* fe) {
    if (!fe) return;
    ph_fold(fe, true);
    for (int i = 0; i < kPhases; i++) {
        fe->phase_ms[i] = 0;
        fe->phase_n[i] = 0;
    }
}

}  // extern "C"
