// The batched front end's enqueue helpers: what a step (frontend_step.cpp) and
// init (frontend_lifecycle.cpp) put on the streams -- FAST / ORB detection, the
// stereo LK, the keyframe, the speculative stereo LK, the side work (full
// copies, SQPnP statistics, final fits), the post-LK and the two parts of a
// step's first half. Enqueue only unless a comment says otherwise.
#include <algorithm>
#include <cstring>

#include "frontend_state.hpp"
#include "linalg.hpp"

namespace svo {

FastDetBatch fe_fast_batch(svo_frontend* fe, const PyrDesc* descs_cur, bool use_mask) {
    FastDetBatch fb{descs_cur, nullptr, fe->fbits, fe->rowcnt, fe->rowoff,
                    (svo_keypoint*)fe->kps, fe->kn, fe->npx, (fe->W + 63) / 64, fe->KCAP};
    fb.score_map = fe->score_map;
    fb.padded = true;  // the frames are svo_image levels
    if (use_mask) {  // boxes around the previous frame's features, rasterised per FAST tile
        fb.box_pts = fe->xyA;
        fb.box_counts = fe->nA;
        fb.box_stride = fe->CAP;
        fb.box_half = fe->cfg.mask_half;
        fb.box_binned = fe->box_binned;
        fb.box_band = fe->box_band;
    }
    return fb;
}

int fe_fast_and_bucket(svo_frontend* fe, const PyrDesc* descs_cur, bool use_mask, hipStream_t st, bool prebinned,
                       int stage) {
    svo_ctx* ctx = fe->ctx;
    int slot;
    FastDetBatch fb = fe_fast_batch(fe, descs_cur, use_mask);
    fb.box_prebinned = prebinned;
    ph_begin(fe, PH_FAST, st, &slot);
    SVO_HIP(ctx, launch_fast_detect(fb, fe->S, fe->W, fe->H, fe->cfg.fast_threshold, fe->cfg.fast_nonmax, st, stage));
    ph_end(fe, st, slot);
    if (stage == kFastDetect) return SVO_OK;
    if (fe->cfg.bucket_size > 0) {
        ph_begin(fe, PH_BUCKET, st, &slot);
        BucketBatch bb{fe->kps, 3, fe->KCAP, fe->kn, 0, nullptr, fe->cand, nullptr, fe->BCAP, fe->bn, fe->scr,
                       fe->bscr};
        SVO_HIP(ctx, launch_bucket(bb, fe->S, fe->W, fe->H, fe->cfg.bucket_size, fe->cfg.per_bucket, st));
        ph_end(fe, st, slot);
    }
    return SVO_OK;
}

// ORB keyframe detection of frame t of every sequence (cfg.use_orb): its keypoints
// into kps / kn where FAST's would go, with the box mask around xyA / nA (the
// previous frame's features, R:src/tracking.cpp:76-79) unless use_mask is false.
// Synchronous (orb_batch_detect: device stages, then the host's retainBest).
int fe_orb_detect(svo_frontend* fe, int t, bool use_mask, hipStream_t st) {
    svo_ctx* ctx = fe->ctx;
    const int S = fe->S;
    for (int s = 0; s < S; s++) fe->orb_lv0[s] = fe->desc_host[(size_t)(t % fe->T) * S + s].lv[0];
    auto par = [fe](int n, const std::function<void(int)>& fn) { fe->pool->run(n, fn); };
    SVO_HIP(ctx, orb_batch_detect(fe->orb, fe->orb_lv0.data(), use_mask ? fe->xyA : nullptr, fe->nA, fe->CAP, fe->CAP,
                                  fe->cfg.mask_half, (svo_keypoint*)fe->kps, fe->kn, fe->KCAP, st, par,
                                  fe->orb_over.data()));
    return SVO_OK;
}

// FAST pre-detection: frame tn's FAST detection + NMS without the box mask (the
// mask drops corners after NMS, so it can wait for frame tn-1's features) queued
// on the context stream once the current step's FAST chain has consumed the row
// words (ev_fdone); step tn keeps only the box filter, the recount, scan and emit
// behind its LK (kFastBoxes). NB: from here on the context stream -- the next
// right pyramid and the pyramid after next, both queued behind this detection --
// is serialised behind FAST(tn-1)'s chain on the low-priority FAST stream.
static int fe_queue_pre(svo_frontend* fe, int tn) {
    svo_ctx* ctx = fe->ctx;
    hipStream_t st = ctx->stream;
    const PyrDesc* dnext = fe->d_desc + (size_t)(tn % fe->T) * fe->S;
    SVO_HIP(ctx, hipStreamWaitEvent(st, fe->ev_fdone, 0));
    FastDetBatch fb = fe_fast_batch(fe, dnext, false);
    SVO_HIP(ctx, launch_fast_detect(fb, fe->S, fe->W, fe->H, fe->cfg.fast_threshold, fe->cfg.fast_nonmax, st,
                                    kFastDetect));
    SVO_HIP(ctx, hipEventRecord(fe->ev_pre, st));
    fe->ahead.pre_t = tn;
    return SVO_OK;
}

// findLeftFeaturesInRight: calcOpticalFlowPyrLK(left, right, pts, 11x11, 3,
// {COUNT+EPS, 30, 0.001}), flags 0 (R:src/tracking.cpp:97-105) of st_xy[0,
// counts[s]) of every sequence of frame t; max_n bounds every count (the grid).
// With svo_frontend_set_stereo_matcher: row SAD in its place, same wait, same
// buffers, same phase.
static int fe_stereo_lk(svo_frontend* fe, int t, const int* counts, int max_n, hipStream_t st, int grid_hint = 0) {
    svo_ctx* ctx = fe->ctx;
    const svo_frontend_config& c = fe->cfg;
    int slot;
    SVO_HIP(ctx, hipStreamWaitEvent(st, fe->ev_pyr_r_b[t & 1], 0));
    const PyrDesc* dl = fe->d_desc + (size_t)(t % fe->T) * fe->S;
    const PyrDesc* dr = fe->d_desc_r + (size_t)(t % fe->T) * fe->S;
    if (fe->rows_on) {
        StereoRowsBatch rb{dl, dr, fe->st_xy, fe->st_next, fe->st_status, nullptr, nullptr, counts, 0, fe->CAP};
        rb.grid_hint = grid_hint;
        ph_begin(fe, PH_STEREO, st, &slot);
        SVO_HIP(ctx, launch_stereo_rows(rb, fe->S, std::min(std::max(max_n, 0), fe->CAP), fe->rows, st));
        ph_end(fe, st, slot);
        return SVO_OK;
    }
    LKBatch lb{dl, dr, fe->d_der + (size_t)(t % 3) * fe->S, fe->st_xy, fe->st_next, fe->st_status, nullptr, nullptr,
               counts, 0, fe->CAP};
    lb.grid_hint = grid_hint;
    LKParams lp;
    lp.win_w = lp.win_h = c.stereo_win;
    lp.max_level = fe->ml_st;
    lp.max_count = std::min(std::max(c.stereo_max_count, 0), 100);
    const double eps = std::min(std::max(c.stereo_epsilon, 0.0), 10.0);
    lp.eps2 = eps * eps;
    lp.flags = 0;
    lp.cv_order = (c.lk_flags & SVO_LK_OPENCV_ORDER) ? 1 : 0;  // the config's order for both LK calls
    lp.min_eig = (float)c.min_eig;
    lp.want_err = 0;
    lk_apply_env(lp);
    ph_begin(fe, PH_STEREO, st, &slot);
    SVO_HIP(ctx, launch_lk(lb, fe->S, std::min(std::max(max_n, 0), fe->CAP), lp, st));
    ph_end(fe, st, slot);
    return SVO_OK;
}

// stereo_tri_kernel's inputs for the candidates st_xy[0, counts[s]) (the
// speculative ones: spec_n; the serial keyframe's take: st_n)
static StereoTriBatch fe_tri_batch(svo_frontend* fe, const int* counts) {
    const svo_frontend_config& c = fe->cfg;
    StereoTriBatch tb;
    tb.st_xy = fe->st_xy;
    tb.st_next = fe->st_next;
    tb.st_status = fe->st_status;
    tb.spec_n = counts;
    tb.cap = fe->CAP;
    tb.y_threshold = c.y_threshold;
    std::memcpy(tb.P, c.P_left, sizeof(float) * 12);
    std::memcpy(tb.P + 12, c.P_right, sizeof(float) * 12);
    tb.st_X = fe->st_X;
    return tb;
}

// append_kernel's inputs: the take's matches (st_next / st_status / st_X of
// st_xy[0, st_n[s])) behind the kept features xyA / midA / nA
static AppendBatch fe_append_batch(svo_frontend* fe) {
    AppendBatch ab;
    ab.n = fe->nA;
    ab.xy = fe->xyA;
    ab.mid = fe->midA;
    ab.cap = fe->CAP;
    ab.st_xy = fe->st_xy;
    ab.st_n = fe->st_n;
    ab.map = fe->map;
    ab.map_n = fe->map_n;
    ab.map_cap = fe->MAPCAP;
    ab.pend0 = fe->pend0;
    ab.pend_n = fe->pend_n;
    ab.added = fe->added;
    ab.h_n = fe->h_nA;
    ab.h_added = fe->h_added;
    ab.st_X = fe->st_X;
    ab.st_next = fe->st_next;
    ab.ur = fe->win.ur_feat;  // (null without a stereo window)
    return ab;
}

// The keyframe's second half on stream st, behind tail_kernel: the stereo LK of
// exactly the take (st_n, bounded by max_take), the take's filter + DLT (the same
// kernel as behind the speculative stereo LK), then the append compacts. beside_lk:
// the stream runs beside a temporal LK (the deferred keyframe): the append as one
// wave per sequence.
int fe_keyframe_append(svo_frontend* fe, int t, int max_take, hipStream_t st, bool beside_lk) {
    svo_ctx* ctx = fe->ctx;
    int slot;
    int rc = fe_stereo_lk(fe, t, fe->st_n, max_take, st);
    if (rc) return rc;
    SVO_HIP(ctx, launch_stereo_tri(fe_tri_batch(fe, fe->st_n), fe->S, max_take, st));
    ph_begin(fe, PH_APPEND, st, &slot);
    SVO_HIP(ctx, launch_append(fe_append_batch(fe), fe->S, st, beside_lk));
    ph_end(fe, st, slot);
    return SVO_OK;
}

// The keyframe of every sequence on stream st (R:src/tracking.cpp:247-255):
// outlier compaction (inlier bits `bits`, or every point when n_in is all zero)
// + the first candidates up to the sequence's target (h_target: n_features on a
// keyframe, 0 otherwise) (tail_kernel), their stereo LK into the right frame t
// (findLeftFeaturesInRight), then filter + triangulation + append
// (append_kernel). xy_in / mid_in / n_in: the step's tracked points (compacted
// into xyA / midA / nA). max_take: a host bound on every sequence's candidate
// count (the stereo LK grid). stats_parity >= 0: the compaction also sums the
// SQPnP statistics of these inliers (the bits, the points of that step parity)
// into h_stats. spec: the speculative stereo LK (fe_queue_spec) already matched
// every sequence's take candidates: compaction, filter, triangulation and append
// run as one kernel. defer (the deferred keyframe):
// tail_kernel only, which also leaves the kept counts in n_main; the caller
// queues fe_keyframe_append on another stream behind it.
int fe_keyframe(svo_frontend* fe, int t, const int* n_in, const uint32_t* bits, const float* xy_in, const int* mid_in,
                int max_take, hipStream_t st, int stats_parity, bool spec, bool defer) {
    svo_ctx* ctx = fe->ctx;
    const svo_frontend_config& c = fe->cfg;
    int slot;
    const bool bucketed = c.bucket_size > 0;
    TailBatch tb;
    tb.n_in = n_in;
    tb.bits = bits;
    tb.words_cap = fe->WORDS;
    tb.xy_in = xy_in;
    tb.mid_in = mid_in;
    tb.xy_out = fe->xyA;
    tb.mid_out = fe->midA;
    tb.n_out = fe->nA;
    tb.cap = fe->CAP;
    tb.n_target = fe->h_target;
    tb.cand = bucketed ? fe->cand : fe->kps;
    tb.cand_elem = bucketed ? 2 : 3;
    tb.cand_cap = bucketed ? fe->BCAP : fe->KCAP;
    tb.cand_n = bucketed ? fe->bn : fe->kn;
    tb.map = fe->map;
    tb.map_n = fe->map_n;
    tb.map_cap = fe->MAPCAP;
    tb.st_xy = fe->st_xy;
    tb.st_n = fe->st_n;
    tb.h_over = fe->h_over;
    tb.map_epoch = fe->win.ring.map_epoch;  // (null without a window)
    if (defer) tb.n_main = fe->n_main;
    if (stats_parity >= 0) {
        tb.stats_obj = fe->obj_b[stats_parity];
        tb.stats_out = fe->h_stats;
        tb.ifx = 1. / c.K[0];
        tb.ify = 1. / c.K[4];
        tb.cx = c.K[2];
        tb.cy = c.K[5];
    }
    if (spec) {
        ph_begin(fe, PH_TAIL, st, &slot);
        SVO_HIP(ctx, launch_keyframe_fused(tb, fe_append_batch(fe), fe->S, st));
        ph_end(fe, st, slot);
        return SVO_OK;
    }
    ph_begin(fe, PH_TAIL, st, &slot);
    SVO_HIP(ctx, launch_tail(tb, fe->S, st));
    ph_end(fe, st, slot);
    return defer ? SVO_OK : fe_keyframe_append(fe, t, max_take, st, false);
}

// The speculative stereo LK of step t (StereoPrepBatch) on the FAST stream,
// behind FAST (the candidates). The keyframe takes the first target - kept
// candidates, kept <= n_ref, so the first target - n_ref + margin cover the take
// whenever n_ref - kept <= margin. Two forms:
//  - early (fe_front, behind FAST(t)): n_ref = the features before LK (nA, final
//    once the FAST stream has waited for the last keyframe), margin = spec_margin
//    + the last step's largest LK loss; it runs beside LK(t), so the keyframe
//    never waits for it (SVO_KF_EVERY only: the targets of a later step are not
//    known while its first half is queued);
//  - late (fe_post, behind the post-LK): n_ref = the tracked counts (nB), margin
//    = spec_margin; it runs beside the host's RANSAC.
// ev_fast is re-recorded behind it, so the keyframe's wait for FAST covers it too.
static int fe_queue_spec(svo_frontend* fe, int t, bool early) {
    svo_ctx* ctx = fe->ctx;
    const svo_frontend_config& c = fe->cfg;
    hipStream_t sf = fe->st_fast;
    const bool bucketed = c.bucket_size > 0;
    // spec_margin is the slack over the last step's losses: an outlier-heavy
    // sequence (the forward / occluder scene drops ~100 of 2000 points a frame)
    // would otherwise miss the speculation every step and run the serial keyframe
    // (capped: a sequence whose RANSAC failed dropped everything)
    const int margin = fe->sw.spec_margin + std::min(fe->ransac_drop, c.n_features / 4) + (early ? fe->lk_loss : 0);
    StereoPrepBatch pb;
    pb.n_tracked = early ? fe->nA : fe->nB;
    pb.cand = bucketed ? fe->cand : fe->kps;
    pb.cand_elem = bucketed ? 2 : 3;
    pb.cand_cap = bucketed ? fe->BCAP : fe->KCAP;
    pb.cand_n = bucketed ? fe->bn : fe->kn;
    pb.cap = fe->CAP;
    pb.n_target = fe->h_target;
    pb.margin = margin;
    pb.st_xy = fe->st_xy;
    pb.spec_n = fe->spec_n;
    if (!early) SVO_HIP(ctx, hipStreamWaitEvent(sf, fe->ev_post, 0));
    SVO_HIP(ctx, launch_stereo_prep(pb, fe->S, sf));
    // grid for the speculation the last step's smallest tracked count implies
    // (+ slack); the kernel's waves loop over any candidates beyond it
    const int max_spec = std::min(c.n_features + margin, fe->CAP);
    const int hint = std::min(fe->CAP, c.n_features - fe->min_tracked + margin + 32);
    int rc = fe_stereo_lk(fe, t, fe->spec_n, max_spec, sf, hint);
    if (rc) return rc;
    SVO_HIP(ctx, launch_stereo_tri(fe_tri_batch(fe, fe->spec_n), fe->S, hint, sf));
    SVO_HIP(ctx, hipEventRecord(fe->ev_fast, sf));
    fe->ahead.spec_t = t;
    fe->ahead.spec_m = margin;
    fe->ahead.spec_was_early = early;
    return SVO_OK;
}

PendingMap fe_pending(svo_frontend* fe) {
    return PendingMap{fe->map, fe->MAPCAP, fe->pend0, fe->pend_n, fe->h_pose};
}

// Frame::pose() of a fitted frame (R:src/tracking.cpp:198-214): the inverse of
// the solvePnPRansac model [R(rvec) | tvec] (svo::SE3d::inverse), identity
// when RANSAC found no model (rvec = tvec = 0, as the host mirror)
void fe_set_pose(svo_frontend* fe, int s, bool ok, const double rvec[3], const double tvec[3]) {
    pose_cam_to_world(ok, rvec, tvec, fe->h_pose + 12 * (size_t)s);
}

// svo_frontend_set_stereo_tracking: the right columns of frame t's tracked features
// -- the first nA - added of the list -- ahead of the record, on its stream: the
// priors from the window's slot of frame t - 1 (the slot before `slot`, if it holds
// that frame; the kernel compares its epoch with the map's), then the guided match
// between level 0 of frame t's own images into trk_next / trk_status. The upload
// stream waits for ev_trk before it streams another frame into t's image slot.
static int fe_track_stereo(svo_frontend* fe, int t, int slot, hipStream_t st) {
    svo_ctx* ctx = fe->ctx;
    const FeWindow& w = fe->win;
    const int S = fe->S, CAP = fe->CAP;
    const int pslot = (slot + w.slots - 1) % w.slots;
    const bool lookup = fe->trk_guide > 0 && w.count > 0 && w.frame[pslot] == t - 1;
    RowPriorsBatch pb{};
    pb.mid = fe->midA;
    pb.counts = fe->nA;
    pb.sub = fe->added;
    pb.cap = CAP;
    if (lookup) {
        const size_t o = (size_t)pslot * CAP;
        pb.prev_mid = w.ring.mid + o;
        pb.prev_xy = w.ring.xy + 2 * o;
        pb.prev_ur = w.ring.ur + o;
        pb.prev_n = w.ring.n + pslot;
        pb.prev_epoch = w.ring.epoch + pslot;
        pb.cur_epoch = w.ring.map_epoch;
        pb.prev_stride = (size_t)w.slots * CAP;
        pb.prev_n_stride = w.slots;
        pb.prev_cap = CAP;
    }
    pb.d_prior = fe->trk_prior;
    pb.n_out = fe->trk_n;
    SVO_HIP(ctx, launch_row_priors(pb, S, CAP, st));
    SVO_HIP(ctx, hipStreamWaitEvent(st, fe->ev_pyr_r_b[t & 1], 0));  // the right level 0's border
    const PyrDesc* dl = fe->d_desc + (size_t)(t % fe->T) * S;
    const PyrDesc* dr = fe->d_desc_r + (size_t)(t % fe->T) * S;
    StereoRowsBatch rb{dl, dr, fe->xyA, fe->trk_next, fe->trk_status, nullptr, nullptr, fe->trk_n, 0, CAP};
    // the tracked counts are the device's; the last step's tracked counts bound them
    int bound = 0;
    for (int s = 0; s < S; s++) bound = std::max(bound, fe->h_nB[s]);
    bound = std::min(std::max(bound, 1), CAP);
    if (lookup) {
        // few features lack a prior (a lost match one frame ago, a sequence whose map
        // was reclaimed): an eighth of the waves loop over them
        SVO_HIP(ctx, launch_stereo_rows_guided(rb, S, bound, fe->trk, fe->trk_prior, fe->trk_guide, (bound + 7) / 8, st));
    } else {
        SVO_HIP(ctx, launch_stereo_rows(rb, S, bound, fe->trk, st));
    }
    const int is = t % fe->T;
    SVO_HIP(ctx, hipEventRecord(fe->ev_trk[is], st));
    fe->trk_rec[is] = 1;
    return SVO_OK;
}

// The window's slot of frame t: the feature list as the step leaves it (xyA /
// midA / nA) copied on stream st, which runs behind the frame's keyframe and ahead
// of whatever rewrites those lists; the slot's pose is the identity until the
// frame's final fit lands (fe_window_pose). Enqueue only.
int fe_window_record(svo_frontend* fe, int t, hipStream_t st) {
    FeWindow& w = fe->win;
    if (!w.slots) return SVO_OK;
    const int slot = w.count % w.slots;
    if (fe->trk_on) {
        int rc = fe_track_stereo(fe, t, slot, st);
        if (rc) return rc;
        SVO_HIP(fe->ctx, launch_window_record(w.ring, slot, fe->nA, fe->xyA, fe->midA, w.ur_feat, fe->added, fe->S, st,
                                              fe->trk_next, fe->trk_status));
    } else {
        SVO_HIP(fe->ctx,
                launch_window_record(w.ring, slot, fe->nA, fe->xyA, fe->midA, w.ur_feat, fe->added, fe->S, st));
    }
    w.frame[slot] = t;
    w.count++;
    for (int s = 0; s < fe->S; s++) {
        double* T = w.h_pose + 12 * ((size_t)s * w.slots + slot);
        for (int q = 0; q < 12; q++) T[q] = (q == 0 || q == 4 || q == 8) ? 1.0 : 0.0;
    }
    return SVO_OK;
}

// The newest slot's poses from the fits that just landed (fe->pose: rvec, tvec;
// zero without a model): the solvePnPRansac model itself, [R(rvec) | tvec], world
// -> camera -- the bundle adjustment's convention.
static void fe_window_pose(svo_frontend* fe) {
    FeWindow& w = fe->win;
    if (!w.slots || w.count == 0) return;
    const int slot = (w.count - 1) % w.slots;
    for (int s = 0; s < fe->S; s++) {
        const double* P = &fe->pose[6 * (size_t)s];
        double* T = w.h_pose + 12 * ((size_t)s * w.slots + slot);
        la::rodrigues<true>(P, T);  // (the functions h_pose is built with: pose_cam_to_world)
        std::memcpy(T + 9, P + 3, sizeof(double) * 3);
    }
}

// Full D2H of the step's tracked points and map points (after the post-LK), on
// the copy stream; queued once per step, when first needed or at the step's end.
int fe_queue_full(svo_frontend* fe) {
    if (fe->ahead.full_queued) return SVO_OK;
    svo_ctx* ctx = fe->ctx;
    const size_t S = fe->S, CAP = fe->CAP;
    SVO_HIP(ctx, hipStreamWaitEvent(fe->st_copy, fe->ev_post, 0));
    SVO_HIP(ctx, hipMemcpyAsync(fe->h_xyB, fe->xyB, sizeof(float) * 2 * S * CAP, hipMemcpyDeviceToHost, fe->st_copy));
    SVO_HIP(ctx, hipMemcpyAsync(fe->h_obj, fe->obj, sizeof(float) * 3 * S * CAP, hipMemcpyDeviceToHost, fe->st_copy));
    SVO_HIP(ctx, hipEventRecord(fe->ev_full, fe->st_copy));
    fe->ahead.full_queued = true;
    return SVO_OK;
}

// Queue the SQPnP sufficient statistics of the last step's RANSAC inliers on the
// copy stream, written straight to host-coherent memory. The inputs -- inlier
// bits on the host, points from the post-LK kernel the host already waited for
// -- need no device-side wait, so they are queued right behind the keyframe and
// run beside it, ahead of the next LK (a kernel queued beside a running LK waits
// for it: LK leaves no registers free).
int fe_queue_stats(svo_frontend* fe) {
    if (!fe->ahead.stats_pending) return SVO_OK;
    svo_ctx* ctx = fe->ctx;
    const int p = fe->ahead.stats_parity;
    SVO_HIP(ctx, launch_suffstats(fe->obj_b[p], fe->xyB_b[p], fe->nB_b[p], fe->CAP, fe->h_best_b[p], fe->WORDS, fe->S,
                                  fe->cfg.K, fe->h_stats, fe->st_copy));
    // and, with device_fits, the final SQPnP fits from them on the device: the next
    // post-LK (which moves the keyframe's new map points with these poses) then
    // waits for ev_stats
    if (fe->sw.device_fits)
        SVO_HIP(ctx, launch_sqpnp_fit(fe->h_stats, fe->h_fitin, fe->obj_b[p], fe->nB_b[p], fe->CAP, fe->h_best_b[p],
                                      fe->WORDS, fe->S, fe->h_pose6, fe->h_pose, fe->fit_work, fe->st_copy));
    SVO_HIP(ctx, hipEventRecord(fe->ev_stats, fe->st_copy));
    fe->ahead.stats_pending = false;
    return SVO_OK;
}

// Final SQPnP-objective fits of the last step (from the GPU sufficient
// statistics in h_stats): they refine the reported poses, so they run lazily --
// at the next step while the GPU tracks, or when a pose is read. With
// device_fits they ran on the device behind the statistics (fe_queue_stats) and
// the host only reads their poses.
double fe_finish_fits(svo_frontend* fe) {
    if (!fe->ahead.fits_pending) return 0.0;
    auto t0 = fe_clock::now();
    (void)hipEventSynchronize(fe->ev_stats);
    if (fe->sw.device_fits) {
        std::memcpy(fe->pose.data(), fe->h_pose6, sizeof(double) * 6 * (size_t)fe->S);
    } else {
        (void)hipEventSynchronize(fe->ev_full_b[fe->ahead.fit_parity]);  // cheirality test reads h_obj
        fe->pool->run(fe->S, [&](int s) {
            fit_pose(fe->rs[s], fe->cfg.K, fe->h_stats + kSqpnpStats * (size_t)s, &fe->pose[6 * (size_t)s],
                     fe->h_pose + 12 * (size_t)s);
        });
    }
    fe_window_pose(fe);
    fe->ahead.fits_pending = false;
    return fe_ms_since(t0);
}

// The pyramid builds of frame f (context stream) wait for its streamed upload.
int fe_wait_upload(svo_frontend* fe, int f, hipStream_t st) {
    if (!fe->up.t.empty() && fe->up.t[f % fe->T] == f) SVO_HIP(fe->ctx, hipStreamWaitEvent(st, fe->up.ev[f % fe->T], 0));
    return SVO_OK;
}

// Frame f can be built ahead: resident frames are 0 .. n_frames - 1 (a caller
// that reuses slots with set_frame gets no ahead-builds past them); once frames
// are streamed (queue_frames), the ring holds the frames queued into it.
bool fe_has_frame(const svo_frontend* fe, int f) {
    if (fe->up.t.empty()) return f < fe->T;
    return fe->up.t[f % fe->T] == f;
}

// trackFrames' calcOpticalFlowPyrLK parameters (R:src/tracking.cpp:154-179)
static LKParams fe_temporal_params(const svo_frontend* fe) {
    const svo_frontend_config& c = fe->cfg;
    LKParams lp;
    lp.win_w = lp.win_h = c.win;
    lp.max_level = fe->ml;
    lp.max_count = std::min(std::max(c.lk_max_count, 0), 100);
    const double eps = std::min(std::max(c.lk_epsilon, 0.0), 10.0);
    lp.eps2 = eps * eps;
    lp.flags = c.lk_flags & ~(SVO_LK_USE_INITIAL_FLOW | SVO_LK_OPENCV_ORDER);
    lp.cv_order = (c.lk_flags & SVO_LK_OPENCV_ORDER) ? 1 : 0;
    lp.min_eig = (float)c.min_eig;
    lp.want_err = 0;
    lk_apply_env(lp);
    return lp;
}

static int fe_queue_pre_and_right(svo_frontend* fe, int tn);
static int fe_queue_next_image(svo_frontend* fe, int tn);

// Post-LK of step t, queued once the previous step's poses are set
// (fe_finish_fits): its keyframe points go to the world frame first. The
// keyframe's stereo matches go out right behind it, speculatively, beside the
// host's RANSAC.
int fe_post(svo_frontend* fe, int t) {
    FeTrace TP{fe->sw.trace, "fe post", t, false};
    svo_ctx* ctx = fe->ctx;
    const int CAP = fe->CAP;
    hipStream_t sl = fe->st_lk;
    int slot;
    // the previous step's final fits (launch_sqpnp_fit) set the poses the post-LK
    // moves the previous keyframe's new map points with
    if (fe->sw.device_fits) SVO_HIP(ctx, hipStreamWaitEvent(sl, fe->ev_stats, 0));
    PostLkBatch pb{fe->nA, fe->status, fe->next_xy, fe->midA, fe->iters, fe->xyB, fe->midB, fe->nB, fe_pending(fe),
                   fe->obj, CAP, kRansacPrefetch, fe->h_nB, fe->h_itsum, fe->h_samp};
    ph_begin(fe, PH_POST, sl, &slot);
    SVO_HIP(ctx, launch_post_lk(pb, fe->S, sl));
    ph_end(fe, sl, slot);
    SVO_HIP(ctx, hipEventRecord(fe->ev_post, sl));
    TP("post_lk launched");
    // the place memory: the last record's points are in the world frame now; their
    // copy runs while the host draws hypotheses, ahead of this step's keyframe
    {
        int rp = fe_places_flush(fe, sl);
        if (rp) return rp;
    }
    if (fe->ahead.pre_pending == t + 1) {
        // (SVO_FE_PRE_AFTER_POST) frame t+1's pre-detection and right pyramid, on the
        // context stream behind this post-LK: when LK runs long, the pre-detection
        // would otherwise be dispatched ahead of the critical post-LK
        SVO_HIP(ctx, hipStreamWaitEvent(ctx->stream, fe->ev_post, 0));
        int rc = fe_queue_pre_and_right(fe, t + 1);
        if (rc) return rc;
    }
    fe->ahead.pre_pending = -1;
    if (fe->sw.spec_margin >= 0 && fe->ahead.spec_t != t) {
        int rq = fe_queue_spec(fe, t, false);
        if (rq) return rq;
    }
    TP("spec stereo launched");
    // the full point set for the final fits / long RANSAC runs, on the copy stream
    // (parity buffers: the previous step's fits still read theirs)
    return fe_queue_full(fe);
}

// First half of a step (enqueue only, no host waits): the previous step's side
// work if still pending, the pyramid of frame t if not built ahead, temporal LK,
// FAST, the right pyramid of frame t and frame t+1's left pyramid.
// svo_frontend_step enqueues the next step's first half right after its own
// keyframe, so the GPU goes on with LK while the caller is between steps.
// Split in two so that the step can put the next LK on the GPU right behind its
// keyframe (fe_front_lk) before the side work's launches (fe_front_rest).
int fe_front(svo_frontend* fe, int t) {
    int rc = fe_front_lk(fe, t);
    return rc ? rc : fe_front_rest(fe, t);
}

int fe_front_lk(svo_frontend* fe, int t) {
    svo_ctx* ctx = fe->ctx;
    hipStream_t st0 = ctx->stream;
    // (resident frames: the caller keeps slot t % n_frames current, set_frame)
    if (!fe->up.t.empty() && (!fe_has_frame(fe, t) || !fe_has_frame(fe, t - 1)))
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_step: frame %d is not in the ring (queue_frames)", t);
    const int S = fe->S;
    const PyrDesc* dcur = fe->d_desc + (size_t)(t % fe->T) * S;
    int slot;
    // this step's parity buffers (the previous step's stay with its side work)
    fe->xyB = fe->xyB_b[t & 1];
    fe->obj = fe->obj_b[t & 1];
    fe->nB = fe->nB_b[t & 1];
    fe->h_best = fe->h_best_b[t & 1];
    fe->h_xyB = fe->h_xyB_b[t & 1];
    fe->h_obj = fe->h_obj_b[t & 1];
    fe->ev_full = fe->ev_full_b[t & 1];
    fe->ahead.full_queued = false;
    // 0. the previous step's SQPnP statistics and the binning of the FAST mask's
    //    box centres (frame t-1's features) normally went out at the end of that
    //    step, ahead of this step's LK; only after init / a reset are they queued here
    {
        int rq = fe_queue_stats(fe);
        if (rq) return rq;
    }
    // 1. pyramid of frame t and its Scharr derivative pyramid (used when frame
    //    t is the prev image of the next step; OpenCV recomputes it per call),
    //    normally built ahead by the previous step's front half
    if (fe->ahead.pyr_ready != t) {
        int rw = fe_wait_upload(fe, t, st0);
        if (rw) return rw;
        ph_begin(fe, PH_PYR, st0, &slot);
        SVO_HIP(ctx, launch_pyramid_scharr_batched(dcur, fe->d_der + (size_t)(t % 3) * S, S, fe->W, fe->H, fe->nlev,
                                                   st0));
        ph_end(fe, st0, slot);
        SVO_HIP(ctx, hipEventRecord(fe->ev_pyr, st0));
    }
    // 2. temporal LK (trackFrames, frame t-1 -> t) behind frame t's pyramid
    {
        const LKParams lp = fe_temporal_params(fe);
        const PyrDesc* dprev = fe->d_desc + (size_t)((t - 1) % fe->T) * S;
        hipStream_t sl = fe->st_lk;
        // behind a deferred keyframe: the kept features [0, n_main) here -- not nA,
        // which the append rewrites while this launch is still starting waves --
        // and the new ones in a launch of their own behind the append (below)
        const bool split = fe->ahead.split_lk;
        SVO_HIP(ctx, hipStreamWaitEvent(sl, fe->ev_pyr, 0));
        LKBatch lb{dprev, dcur, fe->d_der + (size_t)((t - 1) % 3) * S, fe->xyA, fe->next_xy, fe->status, nullptr,
                   fe->iters, split ? fe->n_main : fe->nA, 0, fe->CAP};
        ph_begin(fe, PH_LK, sl, &slot);
        // grid bound CAP: the host counts of the previous keyframe may not be back yet
        SVO_HIP(ctx, launch_lk(lb, S, fe->CAP, lp, sl));
        ph_end(fe, sl, slot);
        SVO_HIP(ctx, hipEventRecord(fe->ev_lk, sl));
        if (split) {
            // the new features [n_main, nA) on the FAST stream, behind the append that
            // made them, beside the launch above: same parameters, same output arrays
            // (disjoint points). The post-LK, behind both on the LK stream, waits here.
            hipStream_t sf = fe->st_fast;
            SVO_HIP(ctx, hipStreamWaitEvent(sf, fe->ev_pyr, 0));
            LKBatch l2 = lb;
            l2.counts = fe->nA;
            l2.first = fe->n_main;
            SVO_HIP(ctx, launch_lk(l2, S, std::min(std::max(fe->ahead.split_max, 0), fe->CAP), lp, sf));
            SVO_HIP(ctx, hipEventRecord(fe->ev_lk2, sf));
            SVO_HIP(ctx, hipStreamWaitEvent(sl, fe->ev_lk2, 0));
        }
        // frame t-1's images are not read after this LK (its stereo LK and keyframe
        // ran before it on this stream or were waited for there; a deferred
        // keyframe's stereo LK and the second launch: the wait above): its ring
        // slot may be streamed into once this event fires
        if (!fe->up.ev_free.empty()) {
            const int fs = (t - 1) % fe->T;
            SVO_HIP(ctx, hipEventRecord(fe->up.ev_free[fs], sl));
            fe->up.free_rec[fs] = 1;
        }
    }
    return SVO_OK;
}

int fe_front_rest(svo_frontend* fe, int t) {
    svo_ctx* ctx = fe->ctx;
    hipStream_t st0 = ctx->stream;
    const int S = fe->S;
    const PyrDesc* dcur = fe->d_desc + (size_t)(t % fe->T) * S;
    int slot;
    if (!fe->ahead.boxes_binned)
        SVO_HIP(ctx, launch_box_bin(fe_fast_batch(fe, dcur, true), S, fe->W, fe->H, fe->st_fast));
    fe->ahead.boxes_binned = false;
    // 3. mask around frame t-1's features (the reference masks with prevFrame's
    //    features, R:src/tracking.cpp:77) + FAST/bucket on frame t, whole batch:
    //    independent of this step's LK and pose, so it is queued right behind the
    //    LK on the low-priority FAST stream, where it fills the CUs the LK's last
    //    waves leave idle and the post-LK window; the keyframe waits for it
    {
        hipStream_t sf = fe->st_fast;
        int stage = kFastAll;
        if (fe->sw.fast_pre && fe->ahead.pre_t == t) {
            // frame t was detected (unmasked) during step t-1; only the box mask of
            // frame t-1's features, the recount, scan and emit remain
            SVO_HIP(ctx, hipStreamWaitEvent(sf, fe->ev_pre, 0));
            stage = kFastBoxes;
        }
        fe->ahead.pre_t = -1;
        if (!fe->orb) {  // (ORB detects at the keyframe, fe_orb_detect)
            int rc = fe_fast_and_bucket(fe, dcur, true, sf, true, stage);
            if (rc) return rc;
        }
        SVO_HIP(ctx, hipEventRecord(fe->ev_fast, sf));
        SVO_HIP(ctx, hipEventRecord(fe->ev_fdone, sf));
    }
    // 4. the right frame t's pyramid (no derivatives: it is the stereo LK's next
    //    image), normally built ahead in the previous step (6b); the stereo LK of
    //    frame t waits for ev_pyr_r_b[t & 1]
    if (fe->ahead.pyr_r_ready != t) {
        int rw = fe_wait_upload(fe, t, st0);
        if (rw) return rw;
        ph_begin(fe, PH_PYR_R, st0, &slot);
        SVO_HIP(ctx, launch_pyramid_batched(fe->d_desc_r + (size_t)(t % fe->T) * S, S, fe->W, fe->H, fe->nlev, st0));
        ph_end(fe, st0, slot);
        SVO_HIP(ctx, hipEventRecord(fe->ev_pyr_r_b[t & 1], st0));
    }
    fe->ahead.pyr_r_ready = -1;
    // 4b. early speculative stereo LK of frame t (fe_queue_spec), behind FAST(t)
    //     and this right pyramid
    if (fe->sw.spec_early && fe->sw.spec_margin >= 0 && fe->cfg.keyframe_rule == SVO_KF_EVERY) {
        for (int s = 0; s < S; s++) fe->h_target[s] = fe->cfg.n_features;
        int rc = fe_queue_spec(fe, t, true);
        if (rc) return rc;
    }
    // 5. frame t+1's pyramid + Scharr + borders, queued beside this LK: the
    //    derivative pyramids are triple-buffered (frame f in f % 3), so nothing
    //    this step reads is overwritten, and the memory-bound pyramid shares the
    //    GPU with the VALU-bound LK instead of the post-LK window
    if (fe_has_frame(fe, t + 1)) return fe_queue_next_image(fe, t + 1);
    return SVO_OK;
}

// Frame tn's left pyramid, its FAST pre-detection and its right pyramid on the
// context stream (steps 5-6b of the first half of step tn - 1).
static int fe_queue_next_image(svo_frontend* fe, int tn) {
    svo_ctx* ctx = fe->ctx;
    hipStream_t st0 = ctx->stream;
    const int S = fe->S;
    int slot;
    {
        int rw = fe_wait_upload(fe, tn, st0);
        if (rw) return rw;
        const PyrDesc* dnext = fe->d_desc + (size_t)(tn % fe->T) * S;
        ph_begin(fe, PH_PYR, st0, &slot);
        SVO_HIP(ctx, launch_pyramid_scharr_batched(dnext, fe->d_der + (size_t)(tn % 3) * S, S, fe->W, fe->H,
                                                   fe->nlev, st0));
        ph_end(fe, st0, slot);
        SVO_HIP(ctx, hipEventRecord(fe->ev_pyr, st0));
        fe->ahead.pyr_ready = tn;
        // (pre_after_post: 6 and 6b are queued by fe_post instead, behind the post-LK)
        if (fe->sw.pre_after_post) {
            fe->ahead.pre_pending = tn;
            return SVO_OK;
        }
        fe->ahead.pre_pending = -1;
    }
    return fe_queue_pre_and_right(fe, tn);
}

// 6. FAST pre-detection of frame tn (fe_queue_pre), behind its pyramid: it fills
//    the CUs the latency-bound post-LK / stereo chain leaves; 6b. then frame tn's
//    right pyramid: ready when step tn begins, so its speculative stereo LK can
//    start right behind FAST(tn) beside LK(tn) (built beside LK(tn) instead, it was
//    starved until LK's end).
static int fe_queue_pre_and_right(svo_frontend* fe, int tn) {
    svo_ctx* ctx = fe->ctx;
    hipStream_t st0 = ctx->stream;
    const int S = fe->S;
    int slot;
    if (fe->sw.fast_pre) {
        int rc = fe_queue_pre(fe, tn);
        if (rc) return rc;
    }
    ph_begin(fe, PH_PYR_R, st0, &slot);
    SVO_HIP(ctx, launch_pyramid_batched(fe->d_desc_r + (size_t)(tn % fe->T) * S, S, fe->W, fe->H, fe->nlev, st0));
    ph_end(fe, st0, slot);
    SVO_HIP(ctx, hipEventRecord(fe->ev_pyr_r_b[tn & 1], st0));
    fe->ahead.pyr_r_ready = tn;
    return SVO_OK;
}

}  // namespace svo
