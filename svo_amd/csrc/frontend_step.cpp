// Batched, device-resident tracking front end: the per-frame loop of
// Tracking::startStereo (R:src/tracking.cpp:232-276) for n_seq independent
// stereo sequences advanced in lockstep.
//
//   step(t), for every sequence s at once:
//     pyramid + Scharr of left frame t+1, pyramid of right t   [pyramid.hip]   (beside LK)
//     temporal LK  frame t-1 -> t (21x21, L3, 50 it)     [lk_multi.hip]  trackFrames :154-179
//     mask of boxes around frame t-1's features + FAST   [fast.hip]      extractFeatures :74-92
//     (host) final SQPnP fits of step t-1 -> poses       [pose.cpp]      calculatePose :191-214
//     keyframe points of t-1 to the world frame, keep status == 1,
//       gather map points, first RANSAC subsets          [fe_kernels]    :169-175, :182-187, :141
//     RANSAC: host EPnP chunks <-> GPU scoring launches  [pose.cpp, pnp.hip] calculatePose :191-196
//     drop outliers + the keyframe's first corners       [fe_kernels]    :218-229
//     stereo LK of those corners into right frame t      [lk_multi.hip]  findLeftFeaturesInRight :94-118
//     |yR - yL| < 40, DLT triangulation, z > 0, append   [fe_kernels]    triangulateNewMapPoints :120-152
//       (deferred, the default of large batches: these two beside the next step's
//        temporal LK of the kept features, and a second LK launch over the new ones
//        behind them)
//     (window enabled) the frame's lists into its ring slot [fe_kernels]  the back end's input, DESIGN.md §10
//
// Which frames are keyframes: every frame, topping the set up to n_features
// (SVO_KF_EVERY, the benchmark), or Tracking::nextFrame's rule (SVO_KF_REFERENCE,
// :68-69) -- a per-sequence target (n_features or 0) the keyframe kernels read.
//
// FAST runs on the GPU beside LK; the host builds RANSAC hypotheses while the GPU
// scores; the final pose fits run on the host while the GPU tracks the next frame,
// so a keyframe's new map points stay in its camera frame until the next step
// moves them to the world frame with that pose (PendingMap, frontend.hpp).
//
// Streams (the box gives a process 4 hardware queues, GPU_MAX_HW_QUEUES): the
// LK stream (LK, post-LK, scoring, keyframe; highest priority), the FAST stream
// (box binning, FAST, the deferred keyframe's stereo LK + append + second LK
// launch, or the speculative stereo LK; lowest), the context stream
// (pyramids, FAST pre-detection) and the copy stream (host copies, SQPnP
// statistics).
//
// This file: svo_frontend_step as a sequence of stages over one FeStep. What the
// stages enqueue is in frontend_enqueue.cpp, the handle in frontend_state.hpp.
#include <algorithm>
#include <cstring>
#include <functional>
#include <thread>

#include "frontend_state.hpp"

using namespace svo;

namespace {

// One step's locals, shared by its stages.
struct FeStep {
    FeTrace TP;
    fe_clock::time_point t_call = fe_clock::now();
    // host timers and counters (svo_frontend_stats)
    double ms_enqueue = 0, ms_wait_post = 0, ms_wait_score = 0, ms_wait_kf = 0, ms_hyp = 0, ms_fit = 0, ms_orb = 0;
    int64_t rounds = 0, nhyp = 0, inl = 0, n_keyframes = 0, lk_its = 0, tracked = 0;
    bool spec = false;        // a speculative stereo LK of this step went out ...
    bool spec_early = false;  // ... with the first half (fe_front), not with the post-LK (fe_post)
    bool spec_ok = false;     // and every sequence dropped at most its margin of points
    bool need_full = false, have_full = false;  // the full point copies (fe_queue_full) are needed / on the host
    int max_take = 0;         // the keyframe's candidates per sequence are at most target - kept
    std::vector<int> ms;      // [s] hypotheses of the current RANSAC round
    std::vector<int> flat;    // (sequence, hypothesis) pairs of a chunk round
};

// Keyframe targets of step t (read by the speculative stereo prep and the
// keyframe kernels of this step): n_features on a keyframe, 0 otherwise.
// SVO_KF_EVERY: every frame. SVO_KF_REFERENCE: Tracking::nextFrame
// (R:src/tracking.cpp:68-69) -- the previous frame was no keyframe and kept fewer
// than features_to_track features (h_nA: the count after the previous step).
int64_t fe_keyframe_targets(svo_frontend* fe) {
    const svo_frontend_config& c = fe->cfg;
    int64_t nkf = 0;
    for (int s = 0; s < fe->S; s++) {
        const bool kf = c.keyframe_rule == SVO_KF_EVERY || (!fe->kf_prev[s] && fe->h_nA[s] < c.features_to_track);
        fe->h_target[s] = kf ? c.n_features : 0;
        fe->kf_prev[s] = kf ? 1 : 0;
        nkf += kf ? 1 : 0;
    }
    return nkf;
}

// The first half if the last step did not queue it, the previous step's fits,
// the post-LK.
int step_begin(svo_frontend* fe, int t, FeStep& st) {
    if (fe->ahead.front_t != t) {
        int rf = fe_front(fe, t);
        if (rf) return rf;
    }
    fe->ahead.front_t = -1;
    st.TP("front enqueued");
    st.n_keyframes = fe_keyframe_targets(fe);
    // the previous step's final pose fits: the host does them while the GPU tracks
    // this frame; they set the poses that move the previous keyframe's new map
    // points to the world frame, so this step's post-LK is queued right after
    // (with device_fits they ran on the device and the post-LK waits there)
    st.ms_enqueue += fe_ms_since(st.t_call);
    // (a window needs the device's fits on the host too, before this step's frame
    // takes the next slot: they ran behind the last step's keyframe)
    st.ms_fit = fe->sw.device_fits && !fe->win.slots ? 0.0 : fe_finish_fits(fe);
    st.TP("fits done");
    {
        const auto te = fe_clock::now();
        int rp = fe_post(fe, t);
        if (rp) return rp;
        st.ms_enqueue += fe_ms_since(te);
    }
    st.TP("post-lk queued");
    return SVO_OK;
}

// Wait for the post-LK results, priming the pool (its workers sleep after an
// idle spin window, and a futex wake-up of 15 threads cost ~40 us on the
// critical path) shortly before they are predicted to land.
int step_wait_post(svo_frontend* fe, FeStep& st) {
    const auto tw = fe_clock::now();
    const double lead_ms = fe->post_wait_ms - 0.08;
    bool primed = false;
    for (;;) {
        const hipError_t q = hipEventQuery(fe->ev_post);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) SVO_HIP(fe->ctx, q);
        if (!primed && fe_ms_since(tw) >= lead_ms) {
            fe->pool->prime();
            primed = true;
        }
    }
    const double w = fe_ms_since(tw);
    fe->post_wait_ms = fe->post_wait_ms > 0 ? 0.75 * fe->post_wait_ms + 0.25 * w : w;
    st.TP("lk results on host");
    st.ms_wait_post = fe_ms_since(tw);
    return SVO_OK;
}

// The full point copies on the host (fe_queue_full, then a wait for them).
int step_ensure_full(svo_frontend* fe, FeStep& st) {
    if (st.have_full) return SVO_OK;
    int rf = fe_queue_full(fe);
    if (rf) return rf;
    SVO_HIP(fe->ctx, hipEventSynchronize(fe->ev_full));
    st.have_full = true;
    return SVO_OK;
}

// A RANSAC round's host half: draw the chunks' subsets and solve them on the
// pool. Returns the largest hypothesis count of a sequence (0: nothing drawn).
int ransac_draw_and_solve(svo_frontend* fe, int t, FeStep& st) {
    const int S = fe->S;
    const svo_frontend_config& c = fe->cfg;
    std::vector<int>& flat = st.flat;
    auto th = fe_clock::now();
    // the chunks' subsets are drawn per sequence (the RNG's order), their EPnP
    // solves shared out one hypothesis per pool task: a sequence predicted to
    // need 5 hypotheses no longer keeps one thread busy for 5 solves while
    // others idle (forward / occluder scene: ~320 solves a step)
    flat.clear();
    for (int s = 0; s < S; s++) {
        st.ms[s] = fe->rs[s].draw_chunk();
        for (int j = 0; j < st.ms[s]; j++) flat.push_back(s * kRansacChunk + j);
    }
    // one pool task per group of kEpnpLanes hypotheses (epnp_pixels_batch: their
    // 12 x 12 SVDs in SIMD lanes), groups taken in flat order across sequences
    const int ntask = ((int)flat.size() + kEpnpLanes - 1) / kEpnpLanes;
    auto solve_task = [&](int k) {
        RansacSeq* seqs[kEpnpLanes];
        int js[kEpnpLanes];
        const int k0 = k * kEpnpLanes;
        const int cnt = std::min(kEpnpLanes, (int)flat.size() - k0);
        for (int q = 0; q < cnt; q++) {
            seqs[q] = &fe->rs[flat[k0 + q] / kRansacChunk];
            js[q] = flat[k0 + q] % kRansacChunk;
        }
        solve_hypotheses(seqs, js, cnt, c.K);
    };
    if (fe->sw.trace) {
        // per-task attribution (trace only): which threads ran the solves, how long each took
        std::vector<std::pair<size_t, double>> tk(ntask);
        const auto tb = fe_clock::now();
        fe->pool->run(ntask, [&](int k) {
            const auto a = fe_clock::now();
            solve_task(k);
            tk[k] = {std::hash<std::thread::id>{}(std::this_thread::get_id()),
                     std::chrono::duration<double, std::micro>(fe_clock::now() - a).count()};
        });
        std::vector<size_t> ids;
        double sum = 0, mx = 0;
        for (auto& e : tk) {
            if (std::find(ids.begin(), ids.end(), e.first) == ids.end()) ids.push_back(e.first);
            sum += e.second;
            mx = std::max(mx, e.second);
        }
        std::fprintf(stderr,
                     "[fe t=%d] pool: %zu solves in %zu tasks on %zu threads, mean %.1f us, max %.1f us per task, "
                     "wall %.1f us\n",
                     t, flat.size(), tk.size(), ids.size(), tk.empty() ? 0.0 : sum / tk.size(), mx,
                     std::chrono::duration<double, std::micro>(fe_clock::now() - tb).count());
    } else {
        fe->pool->run(ntask, solve_task);
    }
    int mmax = 0;
    for (int s = 0; s < S; s++) {
        fe->rs[s].nh += st.ms[s];
        mmax = std::max(mmax, st.ms[s]);
    }
    st.ms_hyp += fe_ms_since(th);
    st.TP("hyps generated");
    return mmax;
}

// A RANSAC round's device half: score the round's hypotheses (mmax rows per
// sequence) on the LK stream, wait, and let every sequence consume its counts.
int ransac_score_and_consume(svo_frontend* fe, int t, FeStep& st, int mmax) {
    svo_ctx* ctx = fe->ctx;
    const int S = fe->S;
    const svo_frontend_config& c = fe->cfg;
    hipStream_t sl = fe->st_lk;
    const float thr = (float)((double)c.pnp_reproj * (double)c.pnp_reproj);
    int slot;
    for (int s = 0; s < S; s++) {
        double* dst = fe->z_hyps + 12 * (size_t)s * kRansacChunk;
        std::memcpy(dst, fe->rs[s].hyp, sizeof(double) * 12 * st.ms[s]);
        for (int j = st.ms[s]; j < mmax; j++) std::memset(dst + 12 * j, 0, sizeof(double) * 12);
        st.nhyp += st.ms[s];
    }
    // hypotheses live at stride kRansacChunk; score only the mmax rows of this
    // round (rows beyond a sequence's own count are ignored). The kernel reads
    // the hypotheses and writes bits / counts in host-coherent memory.
    PnpBatch pb{fe->obj, fe->xyB, fe->nB, 0, fe->CAP, fe->z_hyps, mmax, nullptr, fe->z_bits, fe->WORDS, fe->z_cnt};
    pb.mstride = kRansacChunk;
    ph_begin(fe, PH_PNP, sl, &slot);
    SVO_HIP(ctx, launch_pnp_score(pb, S, c.K[0], c.K[4], c.K[2], c.K[5], thr, sl));
    ph_end(fe, sl, slot);
    st.TP("scoring enqueued");
    const auto tsw = fe_clock::now();
    SVO_HIP(ctx, hipStreamSynchronize(sl));
    st.ms_wait_score += fe_ms_since(tsw);
    st.TP("scores on host");
    // consume is a few compares per hypothesis: cheaper here than a pool dispatch
    for (int s = 0; s < S; s++) {
        const int m = st.ms[s];
        if (m <= 0) continue;
        const int* cnts = fe->z_cnt + (size_t)s * kRansacChunk;
        const uint32_t* bits = fe->z_bits + (size_t)s * kRansacChunk * fe->WORDS;
        if (fe->sw.debug) {
            const RansacSeq& r = fe->rs[s];
            unsigned hs = 0;
            for (int k = 0; k < kSampleFloats * m; k++) {
                unsigned u;
                std::memcpy(&u, r.samp + (size_t)kSampleFloats * (r.nh - m) + k, 4);
                hs = hs * 31u + u;
            }
            std::fprintf(stderr, "[fe dbg t=%d s=%d] n=%d nh=%d m=%d samp=%08x cnt=", t, s, r.n, r.nh, m, hs);
            for (int j = 0; j < m; j++) std::fprintf(stderr, "%d(%d,%.17g) ", cnts[j], (int)r.valid[j], r.hyp[12 * j]);
            std::fprintf(stderr, "\n");
        }
        fe->rs[s].consume(cnts, bits, fe->WORDS, c.pnp_confidence);
    }
    return SVO_OK;
}

// calculatePose (RANSAC per sequence, hypotheses scored on the GPU): rounds of
// host solves and GPU scoring until every sequence is done.
int step_ransac(svo_frontend* fe, int t, FeStep& st) {
    const int S = fe->S, CAP = fe->CAP;
    // the speculative stereo LK went out early (fe_front) or with the post-LK (fe_post)
    st.spec = fe->sw.spec_margin >= 0 && fe->ahead.spec_t == t;
    st.spec_early = st.spec && fe->ahead.spec_was_early;
    fe->ahead.spec_t = -1;
    for (int s = 0; s < S; s++) {
        RansacSeq& r = fe->rs[s];
        r.begin(fe->h_obj + 3 * (size_t)s * CAP, fe->h_xyB + 2 * (size_t)s * CAP, fe->h_nB[s], fe->cfg.pnp_iterations);
        r.samp = fe->h_samp + (size_t)kSampleFloats * kRansacPrefetch * s;
        r.nsamp = kRansacPrefetch;
        // first chunk sized by the hypotheses the previous frame's outlier ratio
        // implies (a prediction only: a short chunk costs one more scoring round)
        r.first_chunk = std::max(kChunk0, fe->pred_iters[s]);
        st.need_full |= r.direct && !r.done;  // n <= 5: EPnP on all points
    }
    if (st.need_full) {
        int rf = step_ensure_full(fe, st);
        if (rf) return rf;
    }
    for (;;) {
        // sequences still sampling (no pool dispatch once all are done)
        bool any = false;
        for (int s = 0; s < S; s++) {
            any |= !fe->rs[s].done && !fe->rs[s].direct;
            st.need_full |= fe->rs[s].next_end() > fe->rs[s].nsamp;
        }
        if (!any) break;
        if (st.need_full) {  // past the prefetched subsets (> 26 hypotheses): rare
            const auto tfw = fe_clock::now();
            int rf = step_ensure_full(fe, st);
            if (rf) return rf;
            st.ms_wait_score += fe_ms_since(tfw);
        }
        st.rounds++;
        const int mmax = ransac_draw_and_solve(fe, t, st);
        if (mmax == 0) break;
        int rc = ransac_score_and_consume(fe, t, st, mmax);
        if (rc) return rc;
    }
    // the RANSAC inlier set is the output (R:src/tracking.cpp:218-229); the final
    // SQPnP-objective fit only refines the pose, from statistics summed on the GPU
    st.TP("consumed");
    return SVO_OK;
}

// Every sequence's RANSAC outcome: its inlier bits for the keyframe, the
// device fit's input, the bounds and predictions the next steps size their
// work with.
void step_select(svo_frontend* fe, FeStep& st) {
    const int S = fe->S;
    const svo_frontend_config& c = fe->cfg;
    auto tf = fe_clock::now();
    int lk_loss = 0, ransac_drop = 0;
    st.spec_ok = st.spec;
    for (int s = 0; s < S; s++) {
        RansacSeq& r = fe->rs[s];
        r.select(c.K, false);
        // the device's final fit starts from this outcome (fe_queue_stats)
        SqpnpFitIn& fi = fe->h_fitin[s];
        fi.mode = !r.ok ? 0 : (r.fitted ? 2 : 1);
        std::memcpy(fi.R, r.bestR, sizeof(fi.R));
        std::memcpy(fi.t, r.fitted ? r.tvec : r.bestt, sizeof(fi.t));
        std::memcpy(fi.rv, r.rvec, sizeof(fi.rv));
        const int kept = r.ok ? r.maxGood : (r.n < 4 ? r.n : 0);
        st.max_take = std::max(st.max_take, fe->h_target[s] - kept);
        // (a sequence without a keyframe takes nothing: nothing to cover)
        // (early: h_nA still holds the count before LK; the keyframe rewrites it)
        const int n_ref = st.spec_early ? fe->h_nA[s] : fe->h_nB[s];
        st.spec_ok &= fe->h_target[s] == 0 || n_ref - kept <= fe->ahead.spec_m;
        lk_loss = std::max(lk_loss, fe->h_nA[s] - fe->h_nB[s]);
        ransac_drop = std::max(ransac_drop, fe->h_nB[s] - kept);
        uint32_t* b = fe->h_best + (size_t)s * fe->WORDS;
        std::memset(b, 0, sizeof(uint32_t) * fe->WORDS);
        if (r.ok) {
            std::memcpy(b, r.best.data(), sizeof(uint32_t) * r.best.size());
        } else if (r.n < 4) {
            // solvePnPRansac would throw (CV_Assert npoints >= 4); keep the frame's
            // features untouched instead of aborting the batch
            for (int k = 0; k < r.n; k++) b[k >> 5] |= 1u << (k & 31);
        }
        st.inl += kept;  // (no model from 4 or more points: every point is an outlier)
        fe->pred_iters[s] = (r.ok && r.n > 0)
                                ? std::max(1, RansacSeq::predict_iters(c.pnp_confidence,
                                                                       (double)(r.n - r.maxGood) / r.n,
                                                                       c.pnp_iterations))
                                : 0;
    }
    fe->lk_loss = lk_loss;
    fe->ransac_drop = ransac_drop;
    st.ms_fit += fe_ms_since(tf);
    st.TP("selected");
}

// Drop outliers (R:src/tracking.cpp:218-229) and the keyframe, the side work,
// the next step's first half; then the wait for this step's keyframe.
int step_keyframe_and_next(svo_frontend* fe, int t, FeStep& st) {
    svo_ctx* ctx = fe->ctx;
    const int S = fe->S;
    hipStream_t sl = fe->st_lk, sf = fe->st_fast;
    const PyrDesc* dcur = fe->d_desc + (size_t)(t % fe->T) * S;
    int rc;
    // the SQPnP statistics of these inliers feed the pose fits the host runs during
    // the next step's LK. They are computed by the keyframe's outlier compaction
    // (the same workgroup reads the same points and bits: suffstats.hpp), so they
    // are done when the keyframe is, ahead of the next LK on the same queue. As a
    // kernel of their own on the copy stream they were at times dispatched only
    // after the next LK had filled the GPU -- in a process that had run other front
    // ends first, every step (host_ms_fit 2.25 ms instead of 0.33: the headline
    // 12 % slower, profiles/r06/c_legs_order_cause.txt)
    fe->ahead.stats_pending = true;
    fe->ahead.stats_parity = t & 1;
    // ORB: the keyframe's detection, on the steps that take a keyframe
    if (fe->orb) {
        bool any = false;
        for (int s = 0; s < S; s++) any |= fe->h_target[s] > 0;
        if (any) {
            const auto to = fe_clock::now();
            rc = fe_orb_detect(fe, t, true, sf);
            if (rc) return rc;
            st.ms_orb += fe_ms_since(to);
        } else {
            SVO_HIP(ctx, hipMemsetAsync(fe->kn, 0, sizeof(int) * S, sf));
        }
        SVO_HIP(ctx, hipEventRecord(fe->ev_fast, sf));
    }
    // the mask (reads xyA) and FAST (writes kps) must be done before xyA is
    // rewritten / kps read
    SVO_HIP(ctx, hipStreamWaitEvent(sl, fe->ev_fast, 0));
    // drop the outliers (the kernel reads the inlier bits from host-coherent
    // memory), then the keyframe: candidates, stereo LK, triangulation, append
    // (deferred: the compaction and the candidates only; the rest below, on the
    // FAST stream)
    const bool defer = fe->sw.defer_kf;
    const auto tkq = fe_clock::now();
    rc = fe_keyframe(fe, t, fe->nB, fe->h_best, fe->xyB, fe->midB, st.max_take, sl, fe->ahead.stats_parity, st.spec_ok,
                     defer);
    if (rc) return rc;
    SVO_HIP(ctx, hipEventRecord(fe->ev_tail, sl));
    // (fe_keyframe took the statistics: done with the compaction)
    SVO_HIP(ctx, hipEventRecord(fe->ev_stats, sl));
    if (fe->sw.device_fits) {  // the device's SQPnP fits from them, on the copy stream
        const int p = fe->ahead.stats_parity;
        SVO_HIP(ctx, hipStreamWaitEvent(fe->st_copy, fe->ev_stats, 0));
        SVO_HIP(ctx, launch_sqpnp_fit(fe->h_stats, fe->h_fitin, fe->obj_b[p], fe->nB_b[p], fe->CAP, fe->h_best_b[p],
                                      fe->WORDS, fe->S, fe->h_pose6, fe->h_pose, fe->fit_work, fe->st_copy));
        SVO_HIP(ctx, hipEventRecord(fe->ev_stats, fe->st_copy));
    }
    fe->ahead.stats_pending = false;
    st.TP("tail queued");
    {
        int mt = fe->CAP;
        for (int s = 0; s < S; s++) mt = std::min(mt, fe->h_nB[s]);
        fe->min_tracked = mt;
    }
    fe->ahead.fits_pending = true;  // statistics land with the stream syncs below
    fe->ahead.fit_parity = t & 1;
    // The critical path goes on with the next step's LK right behind this
    // keyframe; only the SQPnP statistics of these inliers go to the GPU ahead of
    // it (the pose fits need them at the next step's start).
    SVO_HIP(ctx, hipStreamWaitEvent(sf, fe->ev_tail, 0));
    if (defer) {
        // the deferred keyframe's second half: the stereo LK of exactly the take, the
        // triangulation and the append on the FAST stream, beside the next step's LK
        // of the kept features. Whatever reads this frame's final lists is on this
        // stream behind it (the records and the box binning below) or waits for
        // ev_app (the host, at the end of this step); the next step's LK of the new
        // features follows it here (fe_front_lk).
        rc = fe_keyframe_append(fe, t, st.max_take, sf, true);
        if (rc) return rc;
        SVO_HIP(ctx, hipEventRecord(fe->ev_app, sf));
        fe->ahead.split_lk = true;
        fe->ahead.split_max = st.max_take;
        st.TP("append queued");
    }
    const auto records = [&]() -> int {
        // the window's copy of this frame's lists, on the FAST stream behind the
        // keyframe: the next keyframe, which rewrites them, waits for that stream's
        // FAST chain (ev_fast) queued behind this copy
        int rr = fe_window_record(fe, t, sf);
        if (rr) return rr;
        // the place memory's record of this frame, behind it on the same terms
        return fe_places_record(fe, t, sf);
    };
    // (deferred: behind the next step's second LK launch, which the post-LK waits for)
    if (!defer) {
        rc = records();
        if (rc) return rc;
    }
    // this step's counts, before the next step's first half re-fills the mirrors
    for (int s = 0; s < S; s++) {
        st.lk_its += fe->h_itsum[s];
        st.tracked += fe->h_nB[s];
    }
    rc = fe_queue_stats(fe);
    if (rc) return rc;
    // the next step's first half goes out now, behind this step's keyframe, so
    // the GPU moves on to its LK while the host returns to the caller: its LK
    // first (the keyframe -> LK hand-off is on the critical path), then the
    // binning of these features as the next frame's mask boxes (FAST stream,
    // ahead of the next step's FAST) and the rest of the first half
    // (streamed frames: the next frame was queued before this step, or the next
    // step finds it missing and fails loudly in its own first half)
    const bool next_ok = fe_has_frame(fe, t + 1);
    if (next_ok) {
        rc = fe_front_lk(fe, t + 1);
        if (rc) return rc;
    }
    if (defer) {
        rc = records();
        if (rc) return rc;
    }
    SVO_HIP(ctx, launch_box_bin(fe_fast_batch(fe, dcur, true), S, fe->W, fe->H, sf));
    fe->ahead.boxes_binned = true;
    if (next_ok) {
        rc = fe_front_rest(fe, t + 1);
        if (rc) return rc;
        fe->ahead.front_t = t + 1;
    }
    st.TP("next front queued");
    st.ms_enqueue += fe_ms_since(tkq);
    // wait for this step's keyframe only (the statistics, the next frame's
    // pyramid and the prefetched first half keep running into the next step);
    // deferred: for its append, beside the next step's LK
    const auto tw = fe_clock::now();
    SVO_HIP(ctx, hipEventSynchronize(defer ? fe->ev_app : fe->ev_tail));
    st.ms_wait_kf = fe_ms_since(tw);
    st.TP("synced");
    return SVO_OK;
}

void step_fill_stats(const svo_frontend* fe, const FeStep& st, svo_frontend_stats* stats) {
    const int S = fe->S;
    std::memset(stats, 0, sizeof(*stats));
    stats->lk_iterations = st.lk_its;
    stats->tracked = st.tracked;
    for (int s = 0; s < S; s++) {
        stats->added += fe->h_added[s];
        stats->features += fe->h_nA[s];
    }
    stats->inliers = st.inl;
    stats->hypotheses = st.nhyp;
    stats->host_ms_hyp = st.ms_hyp;
    stats->host_ms_fit = st.ms_fit;
    stats->host_ms_wait = st.ms_wait_post + st.ms_wait_score + st.ms_wait_kf;
    stats->keyframes = st.n_keyframes;
    stats->host_ms_wait_post = st.ms_wait_post;
    stats->host_ms_wait_score = st.ms_wait_score;
    stats->host_ms_wait_kf = st.ms_wait_kf;
    stats->host_ms_enqueue = st.ms_enqueue;
    stats->host_ms_step = fe_ms_since(st.t_call);
    stats->ransac_rounds = st.rounds;
    int64_t mh = 0;
    for (int s = 0; s < S; s++) mh = std::max<int64_t>(mh, fe->rs[s].nh);
    stats->max_hypotheses = mh;
    // (the deferred keyframe is neither: nothing speculated, nothing to fall back from)
    stats->serial_keyframe = fe->sw.defer_kf || st.spec_ok ? 0 : 1;
    stats->full_copy = st.have_full ? 1 : 0;
    // Tracking::nextFrame's rule: a keyframe takes every masked corner, so a
    // corner left out for lack of capacity (n_features) is a deviation
    int64_t over = 0;
    if (fe->cfg.keyframe_rule == SVO_KF_REFERENCE)
        for (int s = 0; s < S; s++)
            if (fe->h_target[s] > 0)  // a keyframe: this step's detection ran (ORB: orb_over)
                over += fe->h_over[s] + (fe->orb ? fe->orb_over[s] : 0);
    stats->kf_overflow = over;
    stats->host_ms_orb = st.ms_orb;
    stats->spec_margin = fe->ahead.spec_m;
}

}  // namespace

extern "C" int svo_frontend_step(svo_frontend* fe, int t, svo_frontend_stats* stats) {
    if (!fe || t < 1) return SVO_ERR_ARG;
    FeStep st{FeTrace{fe->sw.trace, "fe", t, true}};
    st.ms.assign(fe->S, 0);
    st.flat.reserve((size_t)fe->S * kRansacChunk);
    int rc = step_begin(fe, t, st);
    if (rc) return rc;
    // calculatePose (RANSAC per sequence, hypotheses scored on the GPU), drop
    // outliers (R:src/tracking.cpp:218-229), keyframe
    st.TP("ransac begin");
    rc = step_wait_post(fe, st);
    if (rc) return rc;
    rc = step_ransac(fe, t, st);
    if (rc) return rc;
    step_select(fe, st);
    rc = step_keyframe_and_next(fe, t, st);
    if (rc) return rc;
    ph_collect(fe);
    st.TP.flush();
    if (stats) step_fill_stats(fe, st, stats);
    fe->ahead.stepped = t;
    return SVO_OK;
}
