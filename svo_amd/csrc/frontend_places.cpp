// The batched front end's place memory (svo_frontend_places_*; the rules:
// DESIGN.md section 3e): every recorded frame's features described on the frame
// itself and kept, with their world points, in a ring per sequence; a query
// describes the last step's frame, matches it against the records of a frame
// range, and solves the pose in the best record's world. The records are queued
// in stream order behind the step's keyframe; the query is synchronous and rare:
// its matching and filtering run on the device for every (sequence, record) at
// once, the choice of the record and the RANSAC of each chosen sequence on the host.
#include <algorithm>
#include <cstring>
#include <vector>

#include "frontend_state.hpp"
#include "linalg.hpp"
#include "match_projected.hpp"
#include "places.hpp"

namespace svo {

void fe_places_restart(svo_frontend* fe, int t0) {
    FePlaces& pl = fe->pl;
    if (!pl.slots) return;
    // (the streams were drained: nothing reads the ring; a copy still pending
    // belongs to a record the restart forgets)
    pl.t0 = t0;
    pl.count = 0;
    pl.pending = false;
    std::fill(pl.frame.begin(), pl.frame.end(), -1);
}

// One describe pass on stream st: frame t's level 0 of every sequence blurred,
// then the current lists (xyA / nA) described into desc_tmp / valid.
static int places_describe(svo_frontend* fe, int t, hipStream_t st) {
    svo_ctx* ctx = fe->ctx;
    FePlaces& pl = fe->pl;
    const PyrDesc* frames = fe->d_desc + (size_t)(t % fe->T) * fe->S;
    SVO_HIP(ctx, launch_places_blur(frames, fe->S, fe->W, fe->H, pl.blur, pl.blur_stride, pl.blur_pitch, st));
    SVO_HIP(ctx, launch_places_describe(frames, pl.blur, pl.blur_stride, pl.blur_pitch, fe->xyA, fe->nA, fe->CAP,
                                        fe->S, pl.hp, pl.umax, pl.reach, pl.pat, pl.desc_tmp, pl.valid, st));
    return SVO_OK;
}

// The describe pass and the compaction of frame t's lists into `slot` (desc, xy,
// count; the ids into pend_mid), without touching the ring's bookkeeping.
static int places_record_into(svo_frontend* fe, int t, int slot, hipStream_t st) {
    FePlaces& pl = fe->pl;
    int rc = places_describe(fe, t, st);
    if (rc) return rc;
    const size_t CAP = fe->CAP, at = (size_t)slot * CAP;
    PlacesCompact c{fe->nA, pl.valid, pl.desc_tmp, fe->xyA, fe->midA, fe->CAP, pl.desc + at * SVO_ORB_DESC_BYTES,
                    pl.xy + 2 * at, pl.pend_mid, (size_t)pl.slots * CAP, pl.n + slot, pl.slots};
    SVO_HIP(fe->ctx, launch_places_compact(c, fe->S, st));
    return SVO_OK;
}

static int places_gather_into(svo_frontend* fe, int slot, hipStream_t st) {
    FePlaces& pl = fe->pl;
    const size_t CAP = fe->CAP;
    SVO_HIP(fe->ctx, launch_places_gather_xyz(pl.pend_mid, fe->CAP, pl.n + slot, pl.slots, fe->map, fe->MAPCAP,
                                              pl.xyz + 3 * (size_t)slot * CAP, (size_t)pl.slots * CAP, fe->S, st));
    return SVO_OK;
}

// The record of frame t, if it is one of the recorded frames: on stream st, which
// runs behind the frame's keyframe and ahead of whatever rewrites the lists (as
// fe_window_record). The points follow in fe_places_flush.
int fe_places_record(svo_frontend* fe, int t, hipStream_t st) {
    FePlaces& pl = fe->pl;
    if (!pl.slots || t < pl.t0 || (t - pl.t0) % pl.every != 0) return SVO_OK;
    svo_ctx* ctx = fe->ctx;
    int rc = fe_places_flush(fe, st);  // (never pending here: every step's post-LK flushes)
    if (rc) return rc;
    const int slot = pl.count % pl.slots;
    rc = places_record_into(fe, t, slot, st);
    if (rc) return rc;
    SVO_HIP(ctx, hipEventRecord(pl.ev_rec, st));
    const int is = t % fe->T;
    SVO_HIP(ctx, hipEventRecord(pl.ev_img[is], st));
    pl.img_rec[is] = 1;
    pl.frame[slot] = t;
    pl.count++;
    pl.pending = true;
    pl.pend_slot = slot;
    return SVO_OK;
}

// The pending record's world points, on a stream that runs behind the
// finalisation of the last keyframe's map points and ahead of the next keyframe.
int fe_places_flush(svo_frontend* fe, hipStream_t st) {
    FePlaces& pl = fe->pl;
    if (!pl.slots || !pl.pending) return SVO_OK;
    SVO_HIP(fe->ctx, hipStreamWaitEvent(st, pl.ev_rec, 0));
    int rc = places_gather_into(fe, pl.pend_slot, st);
    if (rc) return rc;
    pl.pending = false;
    return SVO_OK;
}

void fe_places_destroy(svo_frontend* fe) {
    FePlaces& pl = fe->pl;
    if (pl.ev_rec) (void)hipEventDestroy(pl.ev_rec);
    for (hipEvent_t e : pl.ev_img)
        if (e) (void)hipEventDestroy(e);
    if (pl.mem) (void)hipFree(pl.mem);
    pl = FePlaces{};
}

namespace {

// A query's problems: one per (flagged sequence, record whose frame lies in the
// bound), and their device arrays in the context's scratch.
struct PlacesWork {
    std::vector<int> seq, slot;  // per problem
    int *q_set, *t_set;          // device [P]: the query set (s) and the record (s * slots + slot)
    int *idx_qt, *dist_qt, *idx_tq, *dist_tq;  // [P][CAP][2] (the query alone)
    int *pairs, *n_pairs;                      // [P][CAP][2], [P]
    int *sel_prob, *sel_q, *sel_rec;           // [S] the chosen problems
    double* obj;                               // [S][CAP][3]
    float* img;                                // [S][CAP][2]
};

int places_problems(svo_frontend* fe, const uint8_t* which, int t_lo, int t_hi, const char* who, PlacesWork& w) {
    svo_ctx* ctx = fe->ctx;
    const FePlaces& pl = fe->pl;
    for (int s = 0; s < fe->S; s++) {
        if (which && !which[s]) continue;
        for (int k = 0; k < pl.slots; k++)
            if (pl.frame[k] >= 0 && pl.frame[k] >= t_lo && pl.frame[k] <= t_hi) {
                w.seq.push_back(s);
                w.slot.push_back(k);
            }
    }
    const size_t P = w.seq.size(), S = fe->S, CAP = fe->CAP;
    if (P > 65535) return set_error(ctx, SVO_ERR_ARG, "%s: more than 65535 (sequence, record) problems", who);
    if (!carve_scratch(ctx, kScratchDescribe, [&](Carver& c) {
            w.q_set = c.take<int>(P);
            w.t_set = c.take<int>(P);
            w.idx_qt = c.take<int>(2 * P * CAP);
            w.dist_qt = c.take<int>(2 * P * CAP);
            w.idx_tq = c.take<int>(2 * P * CAP);
            w.dist_tq = c.take<int>(2 * P * CAP);
            w.pairs = c.take<int>(2 * P * CAP);
            w.n_pairs = c.take<int>(P);
            w.sel_prob = c.take<int>(S);
            w.sel_q = c.take<int>(S);
            w.sel_rec = c.take<int>(S);
            w.obj = c.take<double>(3 * S * CAP);
            w.img = c.take<float>(2 * S * CAP);
        }))
        return set_error(ctx, SVO_ERR_HIP, "%s: workspace alloc failed", who);
    return SVO_OK;
}

// The query set of every sequence on stream st: the last step's frame described
// and compacted into q_desc / q_xy / q_n.
int places_query_set(svo_frontend* fe, hipStream_t st) {
    FePlaces& pl = fe->pl;
    const int CAP = fe->CAP;
    int rc = places_describe(fe, fe->ahead.stepped, st);
    if (rc) return rc;
    PlacesCompact c{fe->nA,  pl.valid, pl.desc_tmp, fe->xyA, nullptr, CAP, pl.q_desc,
                    pl.q_xy, nullptr, (size_t)CAP, pl.q_n, 1};
    SVO_HIP(fe->ctx, launch_places_compact(c, fe->S, st));
    return SVO_OK;
}

// The device half of a query on the context stream: the query set (the last
// step's frame described and compacted), the 2-NN of every problem in both
// directions -- a sequence's problems share its query set in place -- and the filter.
int places_match(svo_frontend* fe, const PlacesWork& w, const int* h_q_set, const int* h_t_set, int ratio_pct,
                 bool cross_check) {
    svo_ctx* ctx = fe->ctx;
    FePlaces& pl = fe->pl;
    hipStream_t st = ctx->stream;
    const int P = (int)w.seq.size(), CAP = fe->CAP;
    int rc = places_query_set(fe, st);
    if (rc) return rc;
    if (P == 0) return SVO_OK;
    SVO_HIP(ctx, hipMemcpyAsync(w.q_set, h_q_set, sizeof(int) * P, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(w.t_set, h_t_set, sizeof(int) * P, hipMemcpyHostToDevice, st));
    const uint32_t* qd = reinterpret_cast<const uint32_t*>(pl.q_desc);
    const uint32_t* rd = reinterpret_cast<const uint32_t*>(pl.desc);
    // (the counts live on the device: every problem gets the grid of a full list,
    // blocks past a set's count return at once)
    SVO_HIP(ctx, launch_hamming_knn2(qd, rd, pl.q_n, pl.n, CAP, CAP, P, CAP, w.idx_qt, w.dist_qt, st, w.q_set, w.t_set));
    if (cross_check)
        SVO_HIP(ctx,
                launch_hamming_knn2(rd, qd, pl.n, pl.q_n, CAP, CAP, P, CAP, w.idx_tq, w.dist_tq, st, w.t_set, w.q_set));
    SVO_HIP(ctx, launch_match_filter(w.idx_qt, w.dist_qt, cross_check ? w.idx_tq : nullptr, pl.q_n, pl.n, CAP, CAP, P,
                                     ratio_pct, w.pairs, w.n_pairs, st, w.q_set, w.t_set));
    return SVO_OK;
}

}  // namespace

}  // namespace svo

using namespace svo;

extern "C" {

int svo_frontend_places_enable(svo_frontend* fe, int slots, int every, int patch_size, const int8_t* pattern_xy) {
    if (!fe) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    FePlaces& pl = fe->pl;
    if (fe->ahead.stepped >= 0 || pl.slots)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_places_enable: once, before svo_frontend_init");
    if (slots < 1 || slots > SVO_PLACES_MAX_SLOTS || every < 1)
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_places_enable: slots outside 1 .. SVO_PLACES_MAX_SLOTS or "
                                           "every < 1");
    int8_t pat[2 * kOrbPatternPoints];
    if (const char* why = orb_describe_tables(patch_size, pattern_xy, pat, pl.umax, &pl.reach))
        return set_error(ctx, SVO_ERR_ARG, "svo_frontend_places_enable: %s", why);
    pl.hp = patch_size / 2;
    const size_t S = fe->S, N = slots, CAP = fe->CAP;
    pl.blur_pitch = (fe->W + 63) & ~63;
    pl.blur_stride = (size_t)pl.blur_pitch * fe->H;
    auto layout = [&](Carver& p) {
        pl.pat = p.take<int8_t>(2 * kOrbPatternPoints);
        pl.blur = p.take<uint8_t>(S * pl.blur_stride);
        pl.desc_tmp = p.take<uint8_t>(S * CAP * SVO_ORB_DESC_BYTES);
        pl.valid = p.take<uint8_t>(S * CAP);
        pl.desc = p.take<uint8_t>(S * N * CAP * SVO_ORB_DESC_BYTES);
        pl.xy = p.take<float>(2 * S * N * CAP);
        pl.xyz = p.take<double>(3 * S * N * CAP);
        pl.n = p.take<int>(S * N);
        pl.pend_mid = p.take<int>(S * CAP);
        pl.q_desc = p.take<uint8_t>(S * CAP * SVO_ORB_DESC_BYTES);
        pl.q_xy = p.take<float>(2 * S * CAP);
        pl.q_n = p.take<int>(S);
    };
    auto fail = [&](int code, const char* what) {
        fe_places_destroy(fe);
        return set_error(ctx, code, "svo_frontend_places_enable: %s", what);
    };
    const size_t bytes = layout_bytes(layout);  // (leaves every pointer null)
    if (hipMalloc(&pl.mem, bytes) != hipSuccess) {
        pl.mem = nullptr;
        return fail(SVO_ERR_HIP, "hipMalloc");
    }
    layout_place(pl.mem, layout);
    if (hipEventCreateWithFlags(&pl.ev_rec, hipEventDisableTiming) != hipSuccess) return fail(SVO_ERR_HIP, "event");
    pl.ev_img.assign(fe->T, nullptr);
    for (auto& e : pl.ev_img)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(SVO_ERR_HIP, "event");
    pl.img_rec.assign(fe->T, 0);
    if (hipMemsetAsync(pl.mem, 0, bytes, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(pl.pat, pat, sizeof(pat), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)  // (pat is on the stack)
        return fail(SVO_ERR_HIP, "clearing the ring");
    pl.frame.assign(slots, -1);
    pl.every = every;
    pl.count = 0;
    pl.t0 = -1;
    pl.slots = slots;
    return SVO_OK;
}

int svo_frontend_place(svo_frontend* fe, int seq, int slot, int* frame_t, int* n, uint8_t* desc, float* xy,
                       double* xyz, int cap) {
    if (!fe || seq < 0 || seq >= fe->S || cap < 0) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    const FePlaces& pl = fe->pl;
    if (!pl.slots) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_place: no place memory enabled");
    if (slot < 0 || slot >= pl.slots) return set_error(ctx, SVO_ERR_ARG, "svo_frontend_place: slot outside the ring");
    int rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const size_t at = ((size_t)seq * pl.slots + slot) * fe->CAP;
    int cnt = 0;
    if (pl.frame[slot] >= 0) {
        SVO_HIP(ctx, hipMemcpyAsync(&cnt, pl.n + (size_t)seq * pl.slots + slot, sizeof(int), hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipStreamSynchronize(st));
    }
    const size_t k = (size_t)std::min(cnt, cap);
    if (k > 0) {
        if (desc)
            SVO_HIP(ctx, hipMemcpyAsync(desc, pl.desc + at * SVO_ORB_DESC_BYTES, k * SVO_ORB_DESC_BYTES,
                                        hipMemcpyDeviceToHost, st));
        if (xy) SVO_HIP(ctx, hipMemcpyAsync(xy, pl.xy + 2 * at, sizeof(float) * 2 * k, hipMemcpyDeviceToHost, st));
        if (xyz) SVO_HIP(ctx, hipMemcpyAsync(xyz, pl.xyz + 3 * at, sizeof(double) * 3 * k, hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipStreamSynchronize(st));
    }
    if (frame_t) *frame_t = pl.frame[slot];
    if (n) *n = cnt;
    return SVO_OK;
}

// what svo_frontend_places_query and svo_frontend_places_time refuse alike
static int places_query_check(svo_frontend* fe, int t_lo, int t_hi, int ratio_pct, int min_pairs, const char* who) {
    svo_ctx* ctx = fe->ctx;
    if (!fe->pl.slots) return set_error(ctx, SVO_ERR_ARG, "%s: no place memory enabled", who);
    if (fe->ahead.stepped < 0) return set_error(ctx, SVO_ERR_ARG, "%s: before svo_frontend_init", who);
    if (t_lo > t_hi || ratio_pct < 0 || min_pairs < 0)
        return set_error(ctx, SVO_ERR_ARG, "%s: t_lo > t_hi, ratio_pct < 0 or min_pairs < 0", who);
    return SVO_OK;
}

int svo_frontend_places_query(svo_frontend* fe, const uint8_t* which, int t_lo, int t_hi, int ratio_pct,
                              int cross_check, int min_pairs, int* frame_t, int* n_pairs, int* n_inliers, int* ok,
                              double* rvec, double* tvec, int* slot_pairs, int* pairs, int* inliers, int cap) {
    const char* who = "svo_frontend_places_query";
    if (!fe) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    if (!frame_t || !n_pairs || !n_inliers || !ok || !rvec || !tvec || cap < 0)
        return set_error(ctx, SVO_ERR_ARG, "%s: null outputs or cap < 0", who);
    int rc = places_query_check(fe, t_lo, t_hi, ratio_pct, min_pairs, who);
    if (rc) return rc;
    rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    const FePlaces& pl = fe->pl;
    const svo_frontend_config& cfg = fe->cfg;
    hipStream_t st = ctx->stream;
    const int S = fe->S, CAP = fe->CAP;
    PlacesWork w;
    rc = places_problems(fe, which, t_lo, t_hi, who, w);
    if (rc) return rc;
    const int P = (int)w.seq.size();
    std::vector<int> hq(P), ht(P), hn(P, 0);
    for (int p = 0; p < P; p++) {
        hq[p] = w.seq[p];
        ht[p] = w.seq[p] * pl.slots + w.slot[p];
    }
    rc = places_match(fe, w, hq.data(), ht.data(), ratio_pct, cross_check != 0);
    if (rc) return rc;
    if (P) SVO_HIP(ctx, hipMemcpyAsync(hn.data(), w.n_pairs, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));  // (also: hq and ht have left the host)
    // the best record of every flagged sequence: the most pairs, ties to the oldest frame
    std::vector<int> best(S, -1);
    for (int s = 0; s < S; s++) {
        if (which && !which[s]) continue;
        if (slot_pairs)
            for (int k = 0; k < pl.slots; k++) slot_pairs[(size_t)s * pl.slots + k] = -1;
    }
    for (int p = 0; p < P; p++) {
        const int s = w.seq[p];
        if (slot_pairs) slot_pairs[(size_t)s * pl.slots + w.slot[p]] = hn[p];
        const int b = best[s];
        if (b < 0 || hn[p] > hn[b] || (hn[p] == hn[b] && pl.frame[w.slot[p]] < pl.frame[w.slot[b]])) best[s] = p;
    }
    const int need = std::max(min_pairs, 4);
    std::vector<int> sel_s, sel_p, sel_q, sel_r;
    for (int s = 0; s < S; s++) {
        if (which && !which[s]) continue;
        const int b = best[s];
        frame_t[s] = -1;
        n_pairs[s] = b >= 0 ? hn[b] : 0;
        n_inliers[s] = 0;
        ok[s] = 0;
        for (int q = 0; q < 3; q++) rvec[3 * s + q] = tvec[3 * s + q] = 0.0;
        if (b < 0 || hn[b] < need) continue;
        frame_t[s] = pl.frame[w.slot[b]];
        sel_s.push_back(s);
        sel_p.push_back(b);
        sel_q.push_back(hq[b]);
        sel_r.push_back(ht[b]);
    }
    const int nsel = (int)sel_s.size();
    if (nsel == 0) return SVO_OK;
    SVO_HIP(ctx, hipMemcpyAsync(w.sel_prob, sel_p.data(), sizeof(int) * nsel, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(w.sel_q, sel_q.data(), sizeof(int) * nsel, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(w.sel_rec, sel_r.data(), sizeof(int) * nsel, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, launch_places_gather_pairs(w.pairs, w.n_pairs, w.sel_prob, w.sel_q, w.sel_rec, nsel, CAP, pl.q_xy,
                                            pl.xyz, w.obj, w.img, st));
    std::vector<double> obj(3 * (size_t)nsel * CAP);
    std::vector<float> img(2 * (size_t)nsel * CAP);
    std::vector<int> hp(pairs ? 2 * (size_t)nsel * CAP : 0);
    for (int k = 0; k < nsel; k++) {
        const size_t n = hn[sel_p[k]], o = (size_t)k * CAP;
        SVO_HIP(ctx, hipMemcpyAsync(&obj[3 * o], w.obj + 3 * o, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipMemcpyAsync(&img[2 * o], w.img + 2 * o, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, st));
        if (pairs)
            SVO_HIP(ctx, hipMemcpyAsync(&hp[2 * o], w.pairs + 2 * (size_t)sel_p[k] * CAP, sizeof(int) * 2 * n,
                                        hipMemcpyDeviceToHost, st));
    }
    SVO_HIP(ctx, hipStreamSynchronize(st));
    // solvePnPRansac per chosen sequence, as svo_solve_pnp_ransac runs it (its
    // hypotheses are scored on the context stream: one sequence after the other)
    std::vector<int> inl(CAP);
    for (int k = 0; k < nsel; k++) {
        const int s = sel_s[k], n = hn[sel_p[k]];
        const size_t o = (size_t)k * CAP;
        if (pairs) std::memcpy(pairs + 2 * (size_t)s * cap, &hp[2 * o], sizeof(int) * 2 * std::min(n, cap));
        int ni = 0;
        const int found = svo_solve_pnp_ransac(ctx, &obj[3 * o], &img[2 * o], n, cfg.K, cfg.pnp_iterations,
                                               cfg.pnp_reproj, cfg.pnp_confidence, rvec + 3 * s, tvec + 3 * s,
                                               inl.data(), &ni);
        if (found < 0) return found;
        ok[s] = found;
        n_inliers[s] = found ? ni : 0;
        if (!found)
            for (int q = 0; q < 3; q++) rvec[3 * s + q] = tvec[3 * s + q] = 0.0;
        if (inliers && found) std::memcpy(inliers + (size_t)s * cap, inl.data(), sizeof(int) * std::min(ni, cap));
    }
    return SVO_OK;
}

int svo_frontend_places_widen(svo_frontend* fe, const uint8_t* which, const int* frame_t, const double* rvec,
                              const double* tvec, const svo_proj_match_params* params, int* n_pairs, int* n_inliers,
                              int* ok, double* rvec_out, double* tvec_out, int* pairs, int* inliers, int cap) {
    const char* who = "svo_frontend_places_widen";
    if (!fe) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    if (!frame_t || !rvec || !tvec || !n_pairs || !n_inliers || !ok || !rvec_out || !tvec_out || cap < 0)
        return set_error(ctx, SVO_ERR_ARG, "%s: null arguments or cap < 0", who);
    int rc = places_query_check(fe, 0, 0, 0, 0, who);
    if (rc) return rc;
    if (const char* why = proj_params_refused(fe->W, fe->H, params))
        return set_error(ctx, SVO_ERR_ARG, "%s: %s", who, why);
    if (fe->CAP > kProjMaxStride) return set_error(ctx, SVO_ERR_ARG, "%s: more than 2^20 features per sequence", who);
    rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    const FePlaces& pl = fe->pl;
    const svo_frontend_config& cfg = fe->cfg;
    hipStream_t st = ctx->stream;
    const int S = fe->S, CAP = fe->CAP;
    // one problem per flagged sequence whose record is still in the ring
    PlacesWork w{};
    std::vector<int> hq, ht;
    std::vector<double> hT;
    for (int s = 0; s < S; s++) {
        if ((which && !which[s]) || frame_t[s] < 0) continue;
        int slot = -1;
        for (int k = 0; k < pl.slots; k++)
            if (pl.frame[k] == frame_t[s]) slot = k;
        n_pairs[s] = n_inliers[s] = ok[s] = 0;
        double T[12];
        la::rodrigues(rvec + 3 * s, T);  // (before the outputs, which may alias the inputs, are cleared)
        for (int q = 0; q < 3; q++) T[9 + q] = tvec[3 * s + q];
        for (int q = 0; q < 3; q++) rvec_out[3 * s + q] = tvec_out[3 * s + q] = 0.0;
        if (slot < 0) continue;
        w.seq.push_back(s);
        w.slot.push_back(slot);
        hq.push_back(s);
        ht.push_back(s * pl.slots + slot);
        hT.insert(hT.end(), T, T + 12);
    }
    const int P = (int)w.seq.size();
    if (P == 0) return SVO_OK;
    ProjMatch m{};
    m.grid = proj_grid(fe->W, fe->H);
    double* d_poses = nullptr;
    if (!carve_scratch(ctx, kScratchDescribe, [&](Carver& c) {
            w.q_set = c.take<int>(P);
            w.t_set = c.take<int>(P);
            d_poses = c.take<double>(12 * (size_t)P);
            proj_scratch_layout(c, m.scr, (size_t)P, (size_t)CAP, m.grid);
            w.pairs = c.take<int>(2 * (size_t)P * CAP);
            w.n_pairs = c.take<int>(P);
            w.sel_prob = c.take<int>(P);
            w.obj = c.take<double>(3 * (size_t)P * CAP);
            w.img = c.take<float>(2 * (size_t)P * CAP);
        }))
        return set_error(ctx, SVO_ERR_HIP, "%s: workspace alloc failed", who);
    rc = places_query_set(fe, st);
    if (rc) return rc;
    SVO_HIP(ctx, hipMemcpyAsync(w.q_set, hq.data(), sizeof(int) * P, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(w.t_set, ht.data(), sizeof(int) * P, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(d_poses, hT.data(), sizeof(double) * 12 * P, hipMemcpyHostToDevice, st));
    // the points: the records in place (set s * slots + slot of the ring); the keypoints: the query sets
    m.n_pts = pl.n;
    m.n_kp = pl.q_n;
    m.p_stride = m.k_stride = CAP;
    m.xyz = pl.xyz;
    m.pdesc = reinterpret_cast<const uint32_t*>(pl.desc);
    m.kxy = pl.q_xy;
    m.kdesc = reinterpret_cast<const uint32_t*>(pl.q_desc);
    m.poses = d_poses;
    m.p_set = w.t_set;
    m.k_set = w.q_set;
    m.fx = cfg.K[0];
    m.fy = cfg.K[4];
    m.cx = cfg.K[2];
    m.cy = cfg.K[5];
    m.w = fe->W;
    m.h = fe->H;
    m.radius = params->radius;
    m.max_dist = params->max_dist;
    m.ratio_pct = params->ratio_pct;
    m.pairs = w.pairs;
    m.n_pairs = w.n_pairs;
    SVO_HIP(ctx, launch_proj_bin(m, P, st));
    SVO_HIP(ctx, launch_proj_match(m, P, CAP, st));  // (the counts live on the device: a full list's grid)
    SVO_HIP(ctx, launch_proj_pairs(m, P, st));
    // the solver's inputs of every problem (problem k is its own selection)
    std::vector<int> iota(P), hn(P, 0);
    for (int k = 0; k < P; k++) iota[k] = k;
    SVO_HIP(ctx, hipMemcpyAsync(w.sel_prob, iota.data(), sizeof(int) * P, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, launch_places_gather_pairs(w.pairs, w.n_pairs, w.sel_prob, w.q_set, w.t_set, P, CAP, pl.q_xy, pl.xyz,
                                            w.obj, w.img, st));
    SVO_HIP(ctx, hipMemcpyAsync(hn.data(), w.n_pairs, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));  // (also: hq, ht, hT and iota have left the host)
    std::vector<double> obj(3 * (size_t)P * CAP);
    std::vector<float> img(2 * (size_t)P * CAP);
    std::vector<int> hp(pairs ? 2 * (size_t)P * CAP : 0);
    for (int k = 0; k < P; k++) {
        const size_t n = hn[k], o = (size_t)k * CAP;
        if (n == 0) continue;
        SVO_HIP(ctx, hipMemcpyAsync(&obj[3 * o], w.obj + 3 * o, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipMemcpyAsync(&img[2 * o], w.img + 2 * o, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, st));
        if (pairs)
            SVO_HIP(ctx, hipMemcpyAsync(&hp[2 * o], w.pairs + 2 * o, sizeof(int) * 2 * n, hipMemcpyDeviceToHost, st));
    }
    SVO_HIP(ctx, hipStreamSynchronize(st));
    std::vector<int> inl(CAP);
    for (int k = 0; k < P; k++) {
        const int s = w.seq[k], n = hn[k];
        const size_t o = (size_t)k * CAP;
        n_pairs[s] = n;
        if (pairs) std::memcpy(pairs + 2 * (size_t)s * cap, &hp[2 * o], sizeof(int) * 2 * std::min(n, cap));
        if (n < 4) continue;
        int ni = 0;
        const int found = svo_solve_pnp_ransac(ctx, &obj[3 * o], &img[2 * o], n, cfg.K, cfg.pnp_iterations,
                                               cfg.pnp_reproj, cfg.pnp_confidence, rvec_out + 3 * s, tvec_out + 3 * s,
                                               inl.data(), &ni);
        if (found < 0) return found;
        ok[s] = found;
        n_inliers[s] = found ? ni : 0;
        if (!found)
            for (int q = 0; q < 3; q++) rvec_out[3 * s + q] = tvec_out[3 * s + q] = 0.0;
        if (inliers && found) std::memcpy(inliers + (size_t)s * cap, inl.data(), sizeof(int) * std::min(ni, cap));
    }
    return SVO_OK;
}

int svo_frontend_places_time(svo_frontend* fe, int t_lo, int t_hi, int ratio_pct, int cross_check, double ms[2],
                             int* n_problems) {
    const char* who = "svo_frontend_places_time";
    if (!fe || !ms) return SVO_ERR_ARG;
    svo_ctx* ctx = fe->ctx;
    int rc = places_query_check(fe, t_lo, t_hi, ratio_pct, 0, who);
    if (rc) return rc;
    const FePlaces& pl = fe->pl;
    const int t = fe->ahead.stepped;
    const int newest = pl.count > 0 ? (pl.count - 1) % pl.slots : -1;
    if (newest < 0 || pl.frame[newest] != t)
        return set_error(ctx, SVO_ERR_ARG, "%s: the last step's frame is not the newest record", who);
    rc = svo_frontend_synchronize(fe);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    for (auto& ev : e) SVO_HIP(ctx, hipEventCreate(&ev));
    PlacesWork w;
    rc = places_problems(fe, nullptr, t_lo, t_hi, who, w);
    const int P = (int)w.seq.size();
    std::vector<int> hq(P), ht(P);
    for (int p = 0; p < P; p++) {
        hq[p] = w.seq[p];
        ht[p] = w.seq[p] * pl.slots + w.slot[p];
    }
    auto timed = [&]() -> int {
        // the newest record once more, from the same frame, lists and map: the same bytes
        SVO_HIP(ctx, hipEventRecord(e[0], st));
        int r = places_record_into(fe, t, newest, st);
        if (r) return r;
        r = places_gather_into(fe, newest, st);
        if (r) return r;
        SVO_HIP(ctx, hipEventRecord(e[1], st));
        r = places_match(fe, w, hq.data(), ht.data(), ratio_pct, cross_check != 0);
        if (r) return r;
        SVO_HIP(ctx, hipEventRecord(e[2], st));
        SVO_HIP(ctx, hipEventSynchronize(e[2]));
        float a = 0.f, b = 0.f;
        SVO_HIP(ctx, hipEventElapsedTime(&a, e[0], e[1]));
        SVO_HIP(ctx, hipEventElapsedTime(&b, e[1], e[2]));
        ms[0] = a;
        ms[1] = b;
        return SVO_OK;
    };
    if (!rc) rc = timed();
    (void)hipStreamSynchronize(st);
    for (auto& ev : e) (void)hipEventDestroy(ev);
    if (n_problems) *n_problems = P;
    return rc;
}

}  // extern "C"
