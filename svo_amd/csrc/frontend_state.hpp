// The batched front end's handle and the helpers its translation units share
// (frontend_lifecycle.cpp, frontend_enqueue.cpp, frontend_step.cpp,
// frontend_api.cpp). Internal: plain structs, public fields.
#pragma once

#include <chrono>
#include <utility>
#include <vector>

#include "frontend.hpp"
#include "host_pool.hpp"
#include "orb.hpp"
#include "pose.hpp"

namespace svo {

constexpr int kPhases = 10;
enum Phase { PH_PYR, PH_LK, PH_POST, PH_STEREO, PH_PNP, PH_TAIL, PH_FAST, PH_BUCKET, PH_APPEND, PH_PYR_R };
constexpr int kEvRing = 256;  // phase-timing events (pairs)

// floor of the first RANSAC hypothesis chunk: a floor of 1 saves an EPnP per
// sequence when one hypothesis is predicted, but the misses' extra scoring
// rounds measured 2-6 % slower on the KITTI bench
constexpr int kChunk0 = 2;

// The deferred keyframe pays where the next temporal LK is long enough to hide the
// stereo LK -> append -> second LK chain beside it (~0.2 ms of latency): n_seq x
// n_features from here on. Measured at 2,000 features (profiles/deferred_keyframe_ab.txt):
// 64 sequences +3.4 % (LK 0.42 ms), 256 sequences +2 % to +2.7 % (LK 1.68 ms); at 16
// sequences (LK 0.15 ms) the chain is the longer of the two and a first form of this
// schedule measured 2-10 % slower, so small batches keep the speculative schedule.
constexpr long long kDeferMinFeatures = 128000;

// Everything read from the environment, once, when a front end is created
// (fe_read_switches).
struct FeSwitches {
    // FAST pre-detection (SVO_FE_FAST_PRE=1, the default): frame t+1's detection +
    // NMS without the box mask queued in step t on the context stream (0: FAST
    // detection behind LK(t) on the FAST stream)
    int fast_pre = 1;
    // SVO_FE_PRE_AFTER_POST (default 1): the pre-detection of frame t+1 and its right
    // pyramid are queued behind step t's post-LK (fe_post) instead of behind frame
    // t+1's left pyramid, so that they cannot take the CUs ahead of the critical
    // post-LK when LK runs long (the forward scene: +3 %; the headline: neutral)
    int pre_after_post = 1;
    int spec_margin = 32;  // RANSAC drops covered by the speculative stereo LK (SVO_FE_SPEC_MARGIN, < 0: off)
    // early speculation (SVO_FE_SPEC_EARLY=1, the default; SVO_KF_EVERY only): the
    // speculative stereo LK of step t goes out in its first half, behind FAST(t),
    // sized from the features before LK (nA) with margin spec_margin + lk_loss
    int spec_early = 1;
    // the deferred keyframe (SVO_KF_EVERY with FAST only): behind
    // RANSAC only tail_kernel runs ahead of the next temporal LK; the stereo LK of
    // exactly the take, the append and a second LK launch over the new features run
    // beside that LK, and nothing is speculated (spec_margin -1, spec_early 0).
    // SVO_FE_DEFER_KF=1 selects it, 0 the speculative schedule; unset, it is the
    // default for batches of kDeferMinFeatures and more, unless SVO_FE_SPEC_MARGIN or
    // SVO_FE_SPEC_EARLY is set explicitly (the speculative schedule then).
    bool defer_kf = false;
    bool trace = false;  // SVO_FE_TRACE=1: the host-side step trace (FeTrace)
    // final SQPnP fits on the device (SVO_FE_DEVICE_FITS=1) instead of the host pool
    // (launch_sqpnp_fit: the eigen-decomposition, the SQP runs over waves, the
    // search). The host's fits take ~0.17 ms per step and hide behind the wait for
    // the post-LK results, while the device's run beside LK and take its CUs
    // (DESIGN.md §6 has the measurements), so the host is the default
    bool device_fits = false;
    bool debug = false;  // SVO_FE_DEBUG=1: per-round RANSAC inputs / scores on stderr
    // SVO_POOL_PIN: 1 pin the pool always, 0 never; -1 (unset): pin when several
    // ranks share the node (one process alone keeps the OS placement: pinning it
    // to fixed cores measured up to 4x slower host work on a shared box)
    int pool_pin = -1;
    double pool_spin_us = 400.0;  // SVO_POOL_SPIN_US (Pool)
};
// (ORB -- detection at the keyframe, the serial keyframe path -- overrides
// fast_pre = 0, spec_margin = -1, spec_early = 0, defer_kf = false)
FeSwitches fe_read_switches(const svo_frontend_config& c);

// What is queued or built ahead of the step that will use it. A frame index
// names the step / frame the work belongs to; -1: none.
struct FeAhead {
    int front_t = -1;      // step whose first half (LK .. FAST) is enqueued; set by the step before (its tail), taken by step
    int pyr_ready = -1;    // frame whose pyramid + Scharr were built ahead; fe_queue_next_image -> fe_front_lk
    int pyr_r_ready = -1;  // frame whose right pyramid was built ahead; fe_queue_pre_and_right -> fe_front_rest
    int pre_t = -1;        // frame whose unmasked detection sits in fbits / rowcnt / score_map; fe_queue_pre -> fe_front_rest
    int pre_pending = -1;  // frame whose pre-detection waits for fe_post; fe_queue_next_image -> fe_post
    int spec_t = -1;       // step whose speculative stereo LK went out; fe_queue_spec -> the step's RANSAC stage
    int spec_m = 0;        // its margin (features lost to LK + RANSAC it covers); fe_queue_spec -> selection
    bool spec_was_early = false;  // it went out with the first half; fe_queue_spec -> selection
    bool boxes_binned = false;    // box_bin is queued for the next step's FAST; the step's tail -> fe_front_rest
    // the SQPnP statistics of a step's inliers are wanted: the step sets it, its
    // keyframe computes them (fe_keyframe's stats_parity) and the step clears it;
    // fe_queue_stats computes them instead where an error came between
    bool stats_pending = false;
    int stats_parity = 0;       // step parity whose inliers they cover
    bool fits_pending = false;  // the final pose fits of the last step; the step's tail -> fe_finish_fits
    int fit_parity = 0;         // step parity whose RANSAC results they refine
    bool full_queued = false;   // this step's full D2H copy is queued; fe_queue_full, reset by fe_front_lk
    // the last keyframe was deferred: n_main holds its kept counts and its append
    // runs on the FAST stream, so the next temporal LK goes out as two launches,
    // [0, n_main) on the LK stream and [n_main, nA) behind the append; the step's
    // tail -> fe_front_lk (init's keyframe is serial: one launch over [0, nA))
    bool split_lk = false;
    int split_max = 0;          // host bound of nA - n_main (the deferred keyframe's max_take)
    int stepped = -1;           // last completed step (init: t0), -1 before init; step / init -> queue_frames' window
    // everything: init, a restart of the ring
    void forget_all() { *this = FeAhead{}; }
    // everything built from ring slot k of T, whose image is about to change: the
    // first half of step front_t read frames front_t - 1 .. front_t + 1
    void forget_slot(int k, int T) {
        auto in_slot = [&](int f) { return f >= 0 && f % T == k; };
        if (front_t >= 0 && (in_slot(front_t - 1) || in_slot(front_t) || in_slot(front_t + 1))) front_t = -1;
        for (int* f : {&pyr_ready, &pyr_r_ready, &pre_t, &pre_pending, &spec_t})
            if (in_slot(*f)) *f = -1;
    }
};

// streamed frames (svo_frontend_queue_frames): pinned H2D of a step's stereo
// pairs on their own stream into a device staging block (double-buffered by
// frame parity), the conversion kernel into level 0 of the frame's ring slot;
// the pyramid builds of that frame wait for ev[slot]
struct FeUpload {
    hipStream_t st = nullptr;
    uint8_t* stage = nullptr;         // [2 side][S x cap]: the host frames' bytes (copy and conversion
                                      // run in order on st, so one block serves every frame)
    size_t cap = 0;                   // staging bytes per sequence (the widest h * stride seen)
    size_t seq = 0;                   // h * stride of the last queued frame (sequence stride in staging)
    int stride = 0, bgr = 0;          // its row stride and format (svo_frontend_time_ingest)
    std::vector<hipEvent_t> ev;       // [T] conversion of the slot's frame done
    std::vector<int> t;               // [T] frame last streamed into the slot (-1: none)
    std::vector<hipEvent_t> ev_free;  // [T] the slot's frame f read for the last time (after LK(f + 1))
    std::vector<char> free_rec;       // [T] ev_free recorded since the slot was last queued
};

// the observation window (svo_frontend_window_enable; slots == 0: off, every
// pointer below null and nothing added to a step)
struct FeWindow {
    int slots = 0;           // per sequence
    int count = 0;           // frames recorded since init (slot of the next: count % slots)
    std::vector<int> frame;  // [slots] frame number in each slot
    void* mem = nullptr;     // device: the ring, the map epochs, the selection
    WindowRing ring{};
    int *sel_slot = nullptr, *sel_cnt = nullptr, *sel_nc = nullptr;  // launch_window_select's outputs
    double* h_pose = nullptr;  // host-coherent [s][slots][12]: the slots' poses, world -> camera
    // svo_frontend_window_enable_stereo only: the current list's right columns
    // [s][cap] (the append writes its new features'), recorded into ring.ur
    float* ur_feat = nullptr;
};

// the place memory (svo_frontend_places_enable; slots == 0: off, every pointer
// below null and nothing added to a step). Rules: DESIGN.md section 3e.
struct FePlaces {
    int slots = 0;           // records per sequence
    int every = 1;           // frame t is recorded iff (t - t0) % every == 0
    int t0 = -1;             // the init frame
    int count = 0;           // records since init (slot of the next: count % slots)
    std::vector<int> frame;  // [slots] frame number in each slot, -1: none yet
    int hp = 0, reach = 0, umax[16] = {0};
    void* mem = nullptr;  // device: everything below
    int8_t* pat = nullptr;  // 512 (x, y)
    // the work of one describe pass, a record's or a query's: the blurred frames
    // [s] (planes blur_stride apart, rows blur_pitch apart), the uncompacted
    // descriptors [s][CAP][32] and their validity [s][CAP]
    uint8_t* blur = nullptr;
    size_t blur_stride = 0;
    int blur_pitch = 0;
    uint8_t *desc_tmp = nullptr, *valid = nullptr;
    // the ring, [s][slots][CAP] entries: descriptors, pixels, world points; n [s][slots]
    uint8_t* desc = nullptr;
    float* xy = nullptr;
    double* xyz = nullptr;
    int* n = nullptr;
    // The newest record's map ids [s][CAP] until its points are copied: a keyframe's
    // new points reach the world frame only when the frame's pose has landed (the
    // next step's post-LK, or svo_frontend_synchronize), so the copy is queued
    // right behind that (fe_places_flush) -- ahead of the next keyframe, which may
    // renumber the ids. The record itself keeps no id.
    int* pend_mid = nullptr;
    bool pending = false;
    int pend_slot = 0;
    hipEvent_t ev_rec = nullptr;  // the newest record's compaction done (its stream)
    // the query set: the last step's frame described and compacted, [s][CAP]; q_n [s]
    uint8_t* q_desc = nullptr;
    float* q_xy = nullptr;
    int* q_n = nullptr;
    // per image ring slot, the event behind the describe pass that read the slot's
    // frame (a streamed upload into the slot waits for it, as for ev_trk)
    std::vector<hipEvent_t> ev_img;
    std::vector<char> img_rec;
};

}  // namespace svo

struct svo_frontend {
    svo_ctx* ctx = nullptr;
    svo_frontend_config cfg{};
    svo::FeSwitches sw;
    svo::FeAhead ahead;
    svo::FeUpload up;
    svo::FeWindow win;
    svo::FePlaces pl;
    int S = 0, T = 0, CAP = 0, MAPCAP = 0, WORDS = 0, KCAP = 0, BCAP = 0;
    int W = 0, H = 0, nlev = 0, ml = 0, ml_st = 0;
    size_t npx = 0, bscr = 0;
    std::vector<svo_image*> frames;         // left  [s*T + t]
    std::vector<svo_image*> frames_r;       // right [s*T + t]
    std::vector<svo::PyrDesc> desc_host;    // [t*S + s]
    std::vector<svo::PyrDesc> desc_r_host;  // [t*S + s]
    // svo_frontend_set_rectification: the eyes' maps (left, right; null: the frames
    // arrive rectified) and the size the frames' checks use: the raw frame's, W x H
    // without maps
    const svo_rect_maps* rect[2] = {nullptr, nullptr};
    int raw_w = 0, raw_h = 0;
    bool fed = false;  // a frame was set or queued, or init ran: too late for set_rectification / set_stereo_matcher
    // svo_frontend_set_stereo_matcher: row SAD (launch_stereo_rows) in place of the stereo LK
    bool rows_on = false;
    svo_stereo_rows_params rows{};
    // svo_frontend_set_stereo_tracking: the guided row match of every recorded
    // frame's tracked features (fe_window_record), its buffers ([s][CAP]; trk_n [s]:
    // the tracked counts) and, per image ring slot, the event behind the match
    // that read the slot's frame (a streamed upload into the slot waits for it)
    bool trk_on = false;
    svo_stereo_rows_params trk{};
    int trk_guide = 0;
    void* trk_mem = nullptr;
    int *trk_prior = nullptr, *trk_n = nullptr;
    float* trk_next = nullptr;
    uint8_t* trk_status = nullptr;
    std::vector<hipEvent_t> ev_trk;
    std::vector<char> trk_rec;
    uint8_t* rect_stage = nullptr;  // set_frame with maps: the raw pair's staging ([2 side][rect_cap])
    size_t rect_cap = 0;
    // device state (one allocation, in carve order)
    void* dmem = nullptr;
    svo::PyrDesc* d_desc = nullptr;    // [t][s]
    svo::PyrDesc* d_desc_r = nullptr;  // [t][s]
    float *xyA, *next_xy;
    float *st_xy, *st_next;  // keyframe candidates (left) and their stereo LK matches (right)
    uint8_t* st_status;
    float4* st_X;  // stereo_tri_kernel's points of the speculative candidates
    int* st_n;
    int *pend0, *pend_n;  // PendingMap ranges
    int* spec_n;          // speculative stereo candidates per sequence (StereoPrepBatch)
    int* n_main;          // the deferred keyframe's kept counts (TailBatch::n_main)
    float *kps, *cand;
    int *midA, *midB, *iters, *nA, *kn, *bn, *map_n, *added, *rowcnt, *scr;
    uint8_t* status;
    unsigned long long* fbits;
    int* rowoff;
    double* map;
    float* box_binned;
    int* box_band;
    // the tracked-point arrays of a step (xyB, obj, nB) and its inlier bits are
    // double-buffered by step parity: the side work of step t (SQPnP statistics,
    // full copy to the host) reads them while step t+1 already runs
    float *xyB_b[2], *obj_b[2];
    int* nB_b[2];
    float *xyB, *obj;  // this step's parity of the pairs above
    int* nB;
    // host mirrors (pinned): the full point copies for the fits and long RANSAC runs
    void* hmem = nullptr;
    float *h_xyB_b[2], *h_obj_b[2];
    float *h_xyB, *h_obj;  // this step's parity half of h_*_b
    // host-coherent buffers the scoring kernel reads / writes directly (zero-copy:
    // no H2D of the hypotheses, no D2H of bits / counts, no count memset)
    void* zmem = nullptr;
    double* z_hyps = nullptr;    // [s][kRansacChunk][12]
    uint32_t* z_bits = nullptr;  // [s][kRansacChunk][WORDS]
    int* z_cnt = nullptr;        // [s][kRansacChunk] inliers per hypothesis
    // host-coherent memory the kernels write / read directly (no D2H copies on
    // the critical path): post-LK counts / iteration sums / RANSAC subsets, the
    // keyframe's counts, the inlier bits, statistics, poses, keyframe targets
    void* zout = nullptr;
    int *h_nB, *h_nA, *h_added, *h_target, *h_over;
    long long* h_itsum;
    float* h_samp;
    uint32_t* h_best_b[2];
    uint32_t* h_best;          // this step's parity of h_best_b
    double *h_stats, *h_pose;  // h_pose: [s][12] camera -> world of the last fitted frame
    double* h_pose6;           // [s][6] rvec, tvec of the last fitted frame (launch_sqpnp_fit)
    svo::SqpnpFitIn* h_fitin;  // [s] the host RANSAC's outcome the device fit starts from
    void* dermem = nullptr;         // Scharr pyramids of frames t-1, t, t+1: [3][s], frame f in f % 3
    svo::DerivDesc* d_der = nullptr;  // [3][s]
    void* fit_work = nullptr;       // sw.device_fits: sqpnp_fit_work_bytes(S)
    svo::OrbBatch* orb = nullptr;   // cfg.use_orb: the keyframe detector (orb_batch_detect)
    std::vector<svo::ImgLevel> orb_lv0;
    std::vector<int> orb_over;
    uint8_t* score_map = nullptr;  // [s][npx] FAST scores of the kept corners
    // host state of the loop
    std::vector<svo::RansacSeq> rs;
    std::vector<int> pred_iters;   // [s] RANSAC hypotheses the last frame's outlier ratio implies
    std::vector<uint8_t> kf_prev;  // [s] the last frame was a keyframe (SVO_KF_REFERENCE)
    std::vector<double> pose;      // [s][6]
    int min_tracked = 0;           // min over sequences of the last step's tracked count (stereo LK grid hint)
    int lk_loss = 0;               // max over sequences of the last step's LK losses
    int ransac_drop = 0;           // max over sequences of the last step's RANSAC drops
    double post_wait_ms = 0;       // running estimate of the host's wait for the post-LK results
    svo::Pool* pool = nullptr;
    std::vector<int> host_cpus;  // the pool's pinned CPU set (svo_host_cpu_plan)
    // streams (the context's) and events
    hipStream_t st_lk = nullptr;    // LK, post-LK, scoring, keyframe (highest priority)
    hipStream_t st_fast = nullptr;  // box binning + FAST + bucket + speculative stereo LK (lowest)
    // full copies of the tracked points / map points (h_xyB, h_obj): needed only by
    // the final fits, RANSAC past the prefetched subsets and the n <= 5 solve, so
    // they travel on their own stream once requested
    hipStream_t st_copy = nullptr;
    hipEvent_t ev_pyr = nullptr;    // left pyramid of the step's frame built
    hipEvent_t ev_fast = nullptr;   // FAST (and the speculative stereo LK behind it) done
    hipEvent_t ev_lk = nullptr, ev_post = nullptr, ev_tail = nullptr;
    // the deferred keyframe (FAST stream): its append done; the second temporal LK
    // launch (the new features) behind it done
    hipEvent_t ev_app = nullptr, ev_lk2 = nullptr;
    hipEvent_t ev_stats = nullptr;  // SQPnP statistics + final fits of the last step done (copy stream)
    hipEvent_t ev_pyr_r_b[2] = {nullptr, nullptr};  // right pyramid of frame f built: [f & 1]
    hipEvent_t ev_pre = nullptr;    // the pre-detection ahead.pre_t done (context stream)
    hipEvent_t ev_fdone = nullptr;  // this step's FAST chain done (FAST stream)
    hipEvent_t ev_full_b[2] = {nullptr, nullptr};
    hipEvent_t ev_full = nullptr;  // this step's parity of ev_full_b
    // phase timing (ph_begin / ph_end)
    hipEvent_t ev[svo::kEvRing] = {};
    double phase_ms[svo::kPhases] = {0};
    int64_t phase_n[svo::kPhases] = {0};
    std::vector<std::pair<int, int>> pending;  // (phase, event pair index)
    int ev_used = 0;
};

namespace svo {

using fe_clock = std::chrono::steady_clock;
inline double fe_ms_since(fe_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(fe_clock::now() - t0).count();
}

// Host-side trace of a step (sw.trace): label + microseconds since its start.
// Buffered points are printed by flush() (the step: printing would stretch the
// gaps it measures), the others at once (fe_post).
struct FeTrace {
    bool on;
    const char* prefix;  // "fe", "fe post"
    int t;
    bool buffered;
    fe_clock::time_point t0 = fe_clock::now();
    std::vector<std::pair<const char*, double>> points;
    void operator()(const char* label) {
        if (!on) return;
        const double us = std::chrono::duration<double, std::micro>(fe_clock::now() - t0).count();
        if (buffered)
            points.push_back({label, us});
        else
            std::fprintf(stderr, "[%s t=%d] %8.1f us  %s\n", prefix, t, us, label);
    }
    void flush() {
        for (auto& e : points) std::fprintf(stderr, "[%s t=%d] %8.1f us  %s\n", prefix, t, e.second, e.first);
        points.clear();
    }
};

// Phase timing (frontend_api.cpp): event pairs from a ring, folded into the
// totals once complete.
void ph_fold(svo_frontend* fe, bool wait);
void ph_begin(svo_frontend* fe, int ph, hipStream_t st, int* slot);
void ph_end(svo_frontend* fe, hipStream_t st, int slot);
inline void ph_collect(svo_frontend* fe) { ph_fold(fe, false); }

// Enqueue helpers (frontend_enqueue.cpp); each has its comment there.
FastDetBatch fe_fast_batch(svo_frontend* fe, const PyrDesc* descs_cur, bool use_mask);
int fe_fast_and_bucket(svo_frontend* fe, const PyrDesc* descs_cur, bool use_mask, hipStream_t st,
                       bool prebinned = false, int stage = kFastAll);
int fe_orb_detect(svo_frontend* fe, int t, bool use_mask, hipStream_t st);
int fe_keyframe(svo_frontend* fe, int t, const int* n_in, const uint32_t* bits, const float* xy_in, const int* mid_in,
                int max_take, hipStream_t st, int stats_parity, bool spec = false, bool defer = false);
int fe_keyframe_append(svo_frontend* fe, int t, int max_take, hipStream_t st, bool beside_lk);
PendingMap fe_pending(svo_frontend* fe);
void fe_set_pose(svo_frontend* fe, int s, bool ok, const double rvec[3], const double tvec[3]);
int fe_window_record(svo_frontend* fe, int t, hipStream_t st);
// The place memory's hooks (frontend_places.cpp); each a no-op without
// svo_frontend_places_enable. Enqueue only.
void fe_places_restart(svo_frontend* fe, int t0);
int fe_places_record(svo_frontend* fe, int t, hipStream_t st);
int fe_places_flush(svo_frontend* fe, hipStream_t st);
void fe_places_destroy(svo_frontend* fe);
int fe_queue_full(svo_frontend* fe);
int fe_queue_stats(svo_frontend* fe);
double fe_finish_fits(svo_frontend* fe);
int fe_wait_upload(svo_frontend* fe, int f, hipStream_t st);
bool fe_has_frame(const svo_frontend* fe, int f);
int fe_post(svo_frontend* fe, int t);
int fe_front(svo_frontend* fe, int t);
int fe_front_lk(svo_frontend* fe, int t);
int fe_front_rest(svo_frontend* fe, int t);

}  // namespace svo
