// Windowed bundle adjustment C ABI: staging of the ragged
// problem batch (observations sorted by (point, camera), index lists per point
// and per camera) and the Levenberg-Marquardt control over the device stages of
// ba.hip. Poses, points and observations go up once and come down once; per
// iteration the host reads a cost, a status flag and the step size per problem
// and sends back lambda and the accept / active flags. A problem batch that
// already lies on the device as sorted lists per camera (the front end's window)
// is staged there instead (ba_stage.hip, ba_adjust_device) and runs the same LM.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "ba.hpp"

using namespace svo;

namespace {

// Stable counting sort by (point, camera): order[k] = caller's index of the
// k-th staged observation; pt_off (n_points + 1) delimits each point's run,
// cam_idx[cam_off[j] .. cam_off[j + 1]) lists camera j's staged positions, ascending.
void sort_observations(const int* cam, const int* pt, int n, int C, int M, int* order, int* pt_off, int* cam_off,
                       int* cam_idx) {
    std::vector<int> by_cam((size_t)n), head((size_t)(C > M ? C : M) + 1, 0);
    for (int k = 0; k < n; k++) head[(size_t)cam[k] + 1]++;
    for (int j = 0; j < C; j++) head[(size_t)j + 1] += head[j];
    for (int j = 0; j <= C; j++) cam_off[j] = head[j];
    for (int k = 0; k < n; k++) by_cam[(size_t)head[cam[k]]++] = k;
    for (int i = 0; i <= M; i++) pt_off[i] = 0;
    for (int k = 0; k < n; k++) pt_off[pt[k] + 1]++;
    for (int i = 0; i < M; i++) pt_off[i + 1] += pt_off[i];
    std::vector<int> at(pt_off, pt_off + M);
    for (int k = 0; k < n; k++) order[at[pt[by_cam[k]]]++] = by_cam[k];
    std::vector<int> fill(cam_off, cam_off + C);
    for (int k = 0; k < n; k++) cam_idx[fill[cam[order[k]]]++] = k;
}

struct Args {
    int P, maxC, maxM, maxO;
    const int *n_cams, *n_points, *n_obs;
    const double* poses;
    const uint8_t* fixed;
    const double* points;
    const int *obs_cam, *obs_point;
    const float* obs_xy;
    const double* K;
    double delta;
    const float* obs_ur = nullptr;  // stereo: the right column per observation (< 0: monocular) ...
    double baseline = 0;            // ... and the rig's baseline; null / 0 for the monocular entries
};

// the stereo entries' own two arguments
const char* check_stereo(const float* obs_ur, double baseline) {
    if (!obs_ur) return "obs_ur is null";
    if (!std::isfinite(baseline) || !(baseline > 0)) return "baseline is not a finite length > 0";
    return nullptr;
}

const char* check(const Args& a) {
    if (a.P < 0 || a.maxC < 0 || a.maxM < 0 || a.maxO < 0) return "negative size";
    if (!a.K) return "K is null";
    if (a.maxC > SVO_BA_MAX_CAMS) return "more cameras than SVO_BA_MAX_CAMS";
    if (a.P == 0) return nullptr;
    if (a.maxC > 0 && (!a.poses || !a.fixed)) return "poses / fixed is null";
    if (a.maxM > 0 && !a.points) return "points is null";
    if (a.maxO > 0 && (!a.obs_cam || !a.obs_point || !a.obs_xy)) return "observations are null";
    for (int p = 0; p < a.P; p++) {
        const int C = a.n_cams ? a.n_cams[p] : a.maxC, M = a.n_points ? a.n_points[p] : a.maxM;
        const int O = a.n_obs ? a.n_obs[p] : a.maxO;
        if (C < 0 || C > a.maxC) return "camera count outside [0, max_cams]";
        if (M < 0 || M > a.maxM) return "point count outside [0, max_points]";
        if (O < 0 || O > a.maxO) return "observation count outside [0, max_obs]";
        for (int k = 0; k < O; k++) {
            const int c = a.obs_cam[(size_t)p * a.maxO + k], i = a.obs_point[(size_t)p * a.maxO + k];
            if (c < 0 || c >= C) return "observation names a camera out of range";
            if (i < 0 || i >= M) return "observation names a point out of range";
        }
    }
    return nullptr;
}

struct Staged {
    BaBatch b{};
    double *poses, *points, *tposes, *tpoints, *cost, *tcost, *S, *bvec, *dp, *lambda;
    int *active, *accept;
    int nblk;
    // the staged problem (what b's const pointers name), for whoever fills it
    int *n_cams, *n_points, *ocam, *cam_idx, *cam_pt, *pt_off, *cam_off, *pt_id;
    float *oxy, *our;  // our: null for a monocular batch
    uint8_t* fixed;
};

struct Sizes {
    int P, maxC, maxM, maxO;
    double baseline = 0;  // > 0: a stereo batch, with the `our` plane
};

// The device block of a batch of that size, carved: everything the LM's stages
// read and write. Nothing is filled (S / bvec are zeroed); want_ids: pt_id
// [P][maxM], the device staging's map ids.
int alloc_staged(svo_ctx* ctx, const Sizes& a, const double* K, double delta, bool want_S, bool want_dp,
                 bool want_ids, Staged& s) {
    const size_t P = (size_t)a.P, nC = P * a.maxC, nM = P * a.maxM, nO = P * a.maxO;
    s.nblk = ba_point_blocks(a.maxM);
    const size_t ld = 6 * (size_t)a.maxC;
    const bool stereo = a.baseline > 0;
    BaBatch& b = s.b;
    b.P = a.P;
    b.maxC = a.maxC;
    b.maxM = a.maxM;
    b.maxO = a.maxO;
    b.fx = K[0];
    b.fy = K[4];
    b.cx = K[2];
    b.cy = K[5];
    b.delta = delta;
    auto layout = [&](Carver& c) {
        s.poses = c.take<double>(12 * nC);
        s.tposes = c.take<double>(12 * nC);
        s.points = c.take<double>(3 * nM);
        s.tpoints = c.take<double>(3 * nM);
        b.cam_ne = c.take<double>(kNE * nC);
        b.pt_V = c.take<double>(6 * nM);
        b.pt_g = c.take<double>(3 * nM);
        b.pt_Vinv = c.take<double>(6 * nM);
        b.dc = c.take<double>(6 * nC);
        b.step_part = c.take<double>(2 * P * s.nblk);
        b.stepinfo = c.take<double>(2 * P);
        b.cam_cost = c.take<double>(nC);
        s.cost = c.take<double>(P);
        s.tcost = c.take<double>(P);
        b.lambda = s.lambda = c.take<double>(P);
        s.S = want_S ? c.take<double>(P * ld * ld) : nullptr;
        s.bvec = want_S ? c.take<double>(P * ld) : nullptr;
        s.dp = want_dp ? c.take<double>(3 * nM) : nullptr;
        b.n_cams = s.n_cams = c.take<int>(P);
        b.n_points = s.n_points = c.take<int>(P);
        b.ocam = s.ocam = c.take<int>(nO);
        b.cam_idx = s.cam_idx = c.take<int>(nO);
        b.cam_pt = s.cam_pt = c.take<int>(nO);
        b.pt_off = s.pt_off = c.take<int>(P * (a.maxM + 1));
        b.cam_off = s.cam_off = c.take<int>(P * (a.maxC + 1));
        b.cam_cnt = c.take<int>(nC);
        b.pt_free = c.take<int>(nM);
        b.status = c.take<int>(P);
        b.n_free = c.take<int>(P);
        b.active = s.active = c.take<int>(P);
        s.accept = c.take<int>(P);
        s.pt_id = want_ids ? c.take<int>(nM) : nullptr;
        b.oxy = s.oxy = c.take<float>(2 * nO);
        b.fixed = s.fixed = c.take<uint8_t>(nC);
        b.our = s.our = stereo ? c.take<float>(nO) : nullptr;
    };
    if (!carve_scratch(ctx, kScratchBa, layout)) return set_error(ctx, SVO_ERR_HIP, "scratch alloc");
    b.baseline = a.baseline;
    if (s.S) {
        SVO_HIP(ctx, hipMemsetAsync(s.S, 0, sizeof(double) * P * ld * ld, ctx->stream));
        SVO_HIP(ctx, hipMemsetAsync(s.bvec, 0, sizeof(double) * P * ld, ctx->stream));
    }
    return SVO_OK;
}

// The host's problem into the block: the stable sort by (point, camera) and the
// uploads.
int stage(svo_ctx* ctx, const Args& a, bool want_S, bool want_dp, Staged& s) {
    const size_t P = (size_t)a.P, nC = P * a.maxC, nM = P * a.maxM, nO = P * a.maxO;
    std::vector<int> h_nc(P), h_nm(P), ocam(nO, 0), pt_off(P * (a.maxM + 1), 0), cam_off(P * (a.maxC + 1), 0),
        cam_idx(nO, 0), cam_pt(nO, 0), order((size_t)a.maxO);
    std::vector<float> oxy(2 * nO, 0.f), our(a.obs_ur ? nO : 0, 0.f);
    for (size_t p = 0; p < P; p++) {
        const int C = a.n_cams ? a.n_cams[p] : a.maxC, M = a.n_points ? a.n_points[p] : a.maxM;
        const int O = a.n_obs ? a.n_obs[p] : a.maxO;
        h_nc[p] = C;
        h_nm[p] = M;
        const int* cam = a.obs_cam + p * a.maxO;
        const int* pt = a.obs_point + p * a.maxO;
        int* po = &pt_off[p * (a.maxM + 1)];
        int* co = &cam_off[p * (a.maxC + 1)];
        sort_observations(cam, pt, O, C, M, order.data(), po, co, cam_idx.data() + p * a.maxO);
        for (int i = M; i < a.maxM; i++) po[i + 1] = po[M];
        for (int j = C; j < a.maxC; j++) co[j + 1] = co[C];
        for (int k = 0; k < O; k++) {
            const size_t g = p * a.maxO + k, src = p * a.maxO + order[k];
            ocam[g] = cam[order[k]];
            oxy[2 * g] = a.obs_xy[2 * src];
            oxy[2 * g + 1] = a.obs_xy[2 * src + 1];
            if (a.obs_ur) our[g] = a.obs_ur[src];
        }
        for (int k = 0; k < O; k++) cam_pt[p * a.maxO + k] = pt[order[cam_idx[p * a.maxO + k]]];
    }
    int rc = alloc_staged(ctx, Sizes{a.P, a.maxC, a.maxM, a.maxO, a.obs_ur ? a.baseline : 0.0}, a.K, a.delta, want_S,
                          want_dp, false, s);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    auto up = [&](void* dst, const void* src, size_t n) {
        return n ? hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    SVO_HIP(ctx, up(s.poses, a.poses, sizeof(double) * 12 * nC));
    SVO_HIP(ctx, up(s.points, a.points, sizeof(double) * 3 * nM));
    SVO_HIP(ctx, up(s.fixed, a.fixed, nC));
    SVO_HIP(ctx, up(s.n_cams, h_nc.data(), sizeof(int) * P));
    SVO_HIP(ctx, up(s.n_points, h_nm.data(), sizeof(int) * P));
    SVO_HIP(ctx, up(s.ocam, ocam.data(), sizeof(int) * nO));
    SVO_HIP(ctx, up(s.cam_idx, cam_idx.data(), sizeof(int) * nO));
    SVO_HIP(ctx, up(s.cam_pt, cam_pt.data(), sizeof(int) * nO));
    SVO_HIP(ctx, up(s.pt_off, pt_off.data(), sizeof(int) * pt_off.size()));
    SVO_HIP(ctx, up(s.cam_off, cam_off.data(), sizeof(int) * cam_off.size()));
    SVO_HIP(ctx, up(s.oxy, oxy.data(), sizeof(float) * 2 * nO));
    if (s.our) SVO_HIP(ctx, up(s.our, our.data(), sizeof(float) * nO));
    // the staging vectors go out of scope on return: the copies must have left them
    SVO_HIP(ctx, hipStreamSynchronize(st));
    return SVO_OK;
}

// lambda and the active flags of the next pass
int send_control(svo_ctx* ctx, Staged& s, const std::vector<double>& lambda, const std::vector<int>& active) {
    SVO_HIP(ctx, hipMemcpyAsync(s.lambda, lambda.data(), sizeof(double) * lambda.size(), hipMemcpyHostToDevice,
                                ctx->stream));
    SVO_HIP(ctx, hipMemcpyAsync(s.active, active.data(), sizeof(int) * active.size(), hipMemcpyHostToDevice,
                                ctx->stream));
    // pageable source: the copy has left the vectors before the caller changes them
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

// stages 2 - 5 of one iteration (the caller launches stage 1)
int launch_solve_chain(svo_ctx* ctx, Staged& s) {
    hipStream_t st = ctx->stream;
    SVO_HIP(ctx, launch_ba_schur_solve(s.b, s.poses, s.points, s.S, s.bvec, st));
    SVO_HIP(ctx, launch_ba_update(s.b, s.poses, s.points, s.tposes, s.tpoints, s.dp, st));
    SVO_HIP(ctx, launch_ba_cost(s.b, s.tposes, s.tpoints, s.tcost, st));
    return SVO_OK;
}

// Per problem: does it hold a value that is not finite (within its counts)?
std::vector<uint8_t> non_finite(const Args& a) {
    std::vector<uint8_t> bad((size_t)a.P, 0);
    for (size_t p = 0; p < (size_t)a.P; p++) {
        const int C = a.n_cams ? a.n_cams[p] : a.maxC, M = a.n_points ? a.n_points[p] : a.maxM;
        const int O = a.n_obs ? a.n_obs[p] : a.maxO;
        bool ok = true;
        for (int q = 0; q < 12 * C && ok; q++) ok = std::isfinite(a.poses[12 * p * a.maxC + q]);
        for (int q = 0; q < 3 * M && ok; q++) ok = std::isfinite(a.points[3 * p * a.maxM + q]);
        for (int q = 0; q < 2 * O && ok; q++) ok = std::isfinite(a.obs_xy[2 * p * a.maxO + q]);
        for (int q = 0; q < O && ok && a.obs_ur; q++) ok = std::isfinite(a.obs_ur[p * a.maxO + q]);
        bad[p] = !ok;
    }
    return bad;
}

// svo_bundle_adjust's Levenberg-Marquardt control over a filled block: the
// refined state stays in s.poses / s.points. c_first / c_cur: the initial and the
// final cost, its: the iterations each problem began. A problem the caller marks
// in `bad` (empty: none), or whose initial cost is not finite, is not iterated on:
// its state is never written, its costs are NaN and its count 0.
int run_lm(svo_ctx* ctx, Staged& s, int max_iterations, const std::vector<uint8_t>& bad,
           std::vector<double>& c_first, std::vector<double>& c_cur, std::vector<int>& its) {
    const size_t P = (size_t)s.b.P;
    int rc;
    hipStream_t st = ctx->stream;
    std::vector<double> lambda(P, kLmLambda0), c_trial(P), stepinfo(2 * P);
    std::vector<int> active(P, 1), accept(P), status(P), done(P, 0);
    c_cur.assign(P, 0.0);
    its.assign(P, 0);
    auto read_back = [&]() -> int {
        SVO_HIP(ctx, hipMemcpyAsync(c_trial.data(), s.tcost, sizeof(double) * P, hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipMemcpyAsync(stepinfo.data(), s.b.stepinfo, sizeof(double) * 2 * P, hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipMemcpyAsync(status.data(), s.b.status, sizeof(int) * P, hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipStreamSynchronize(st));
        return SVO_OK;
    };
    if ((rc = send_control(ctx, s, lambda, active))) return rc;
    SVO_HIP(ctx, launch_ba_cost(s.b, s.poses, s.points, s.cost, st));
    SVO_HIP(ctx, hipMemcpyAsync(c_cur.data(), s.cost, sizeof(double) * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    for (size_t p = 0; p < P; p++)
        if ((!bad.empty() && bad[p]) || !std::isfinite(c_cur[p])) {
            done[p] = 1;
            c_cur[p] = std::numeric_limits<double>::quiet_NaN();
        }
    c_first = c_cur;
    for (int it = 0; it < max_iterations; it++) {
        bool any = false;
        for (size_t p = 0; p < P; p++) {
            active[p] = !done[p];
            any = any || active[p];
            its[p] += active[p];  // begun: it counts even if it gives up below
        }
        if (!any) break;
        if ((rc = send_control(ctx, s, lambda, active))) return rc;
        SVO_HIP(ctx, launch_ba_linearize(s.b, s.poses, s.points, st));
        if ((rc = launch_solve_chain(ctx, s))) return rc;
        if ((rc = read_back())) return rc;
        // reduced system not positive definite: raise lambda and solve again from
        // the same linearisation, as lm_solve6's callers do
        for (;;) {
            bool retry = false;
            for (size_t p = 0; p < P; p++) {
                const bool again = active[p] && status[p] != 0;
                if (again) {
                    lambda[p] *= kLmUp;
                    if (lambda[p] >= kLmCeiling) {
                        done[p] = 1;
                        active[p] = 0;
                        continue;
                    }
                    retry = true;
                } else if (active[p] && status[p] == 0) {
                    active[p] = 2;  // solved: waits for the verdict below
                }
            }
            if (!retry) break;
            std::vector<int> again(P);
            for (size_t p = 0; p < P; p++) again[p] = active[p] == 1;
            if ((rc = send_control(ctx, s, lambda, again))) return rc;
            // V*^-1 depends on lambda, so stage 1 runs again (its camera pass repeats itself)
            SVO_HIP(ctx, launch_ba_linearize(s.b, s.poses, s.points, st));
            if ((rc = launch_solve_chain(ctx, s))) return rc;
            if ((rc = read_back())) return rc;
        }
        for (size_t p = 0; p < P; p++) {
            accept[p] = 0;
            if (done[p] || active[p] != 2) continue;
            if (lm_step_is_small(stepinfo[2 * p], stepinfo[2 * p + 1])) {
                done[p] = 1;
                continue;
            }
            const LmVerdict v = lm_verdict(c_cur[p], c_trial[p], lambda[p]);
            accept[p] = v.accept;
            if (v.accept) c_cur[p] = c_trial[p];
            done[p] = v.stop;
        }
        SVO_HIP(ctx, hipMemcpyAsync(s.accept, accept.data(), sizeof(int) * P, hipMemcpyHostToDevice, st));
        SVO_HIP(ctx, launch_ba_commit(s.b, s.accept, s.tposes, s.tpoints, s.poses, s.points, st));
        SVO_HIP(ctx, hipStreamSynchronize(st));
    }
    return SVO_OK;
}

// The staging chain's own memory (a slot of its own: the LM's block lives beside it).
int stage_work(svo_ctx* ctx, const BaLists& l, BaStageWork& w) {
    if (!carve_scratch(ctx, kScratchBaStage, [&](Carver& c) { ba_stage_layout(c, l.P, l.W, l.cap, w); }))
        return set_error(ctx, SVO_ERR_HIP, "scratch alloc");
    return SVO_OK;
}

// Host lists, checked (null when they are fine) ...
const char* check_lists(int P, int W, int cap, const int* counts, const int* ids, const float* xy) {
    if (P < 0 || W < 1 || W > SVO_BA_MAX_CAMS || cap < 1 || (int64_t)W * cap > (1 << 24)) return "sizes";
    if (P == 0) return nullptr;
    if (!counts || !ids || !xy) return "lists are null";
    for (size_t q = 0; q < (size_t)P * W; q++) {
        if (counts[q] < 0 || counts[q] > cap) return "count outside 0 .. cap";
        const int* a = ids + q * cap;
        for (int k = 0; k < counts[q]; k++)
            if (a[k] < 0 || (k > 0 && a[k] <= a[k - 1])) return "ids not strictly increasing";
    }
    return nullptr;
}

// ... and uploaded as they are
int upload_lists(svo_ctx* ctx, int P, int W, int cap, const int* counts, const int* ids, const float* xy, BaLists& l,
                 const float* ur = nullptr) {
    const size_t nL = (size_t)P * W, nO = nL * cap;
    int *d_counts, *d_ids;
    float *d_xy, *d_ur;
    if (!carve_scratch(ctx, kScratchBaLists, [&](Carver& c) {
            d_counts = c.take<int>(nL);
            d_ids = c.take<int>(nO);
            d_xy = c.take<float>(2 * nO);
            d_ur = ur ? c.take<float>(nO) : nullptr;
        }))
        return set_error(ctx, SVO_ERR_HIP, "scratch alloc");
    hipStream_t st = ctx->stream;
    SVO_HIP(ctx, hipMemcpyAsync(d_counts, counts, sizeof(int) * nL, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(d_ids, ids, sizeof(int) * nO, hipMemcpyHostToDevice, st));
    SVO_HIP(ctx, hipMemcpyAsync(d_xy, xy, sizeof(float) * 2 * nO, hipMemcpyHostToDevice, st));
    l = BaLists{P, W, cap, nullptr, d_counts, d_ids, d_xy};
    if (ur) {
        SVO_HIP(ctx, hipMemcpyAsync(d_ur, ur, sizeof(float) * nO, hipMemcpyHostToDevice, st));
        l.ur = d_ur;
    }
    return SVO_OK;
}

// what the host's stage() leaves zero behind a problem's last observation
int zero_observations(svo_ctx* ctx, const Staged& s) {
    const size_t nO = (size_t)s.b.P * s.b.maxO;
    for (int* a : {s.ocam, s.cam_idx, s.cam_pt}) SVO_HIP(ctx, hipMemsetAsync(a, 0, sizeof(int) * nO, ctx->stream));
    SVO_HIP(ctx, hipMemsetAsync(s.oxy, 0, sizeof(float) * 2 * nO, ctx->stream));
    if (s.our) SVO_HIP(ctx, hipMemsetAsync(s.our, 0, sizeof(float) * nO, ctx->stream));
    return SVO_OK;
}

BaStageOut stage_out(const Staged& s, const double* map, int map_cap) {
    BaStageOut o;
    o.our = s.our;
    o.maxM = s.b.maxM;
    o.maxO = s.b.maxO;
    o.ocam = s.ocam;
    o.pt_off = s.pt_off;
    o.cam_off = s.cam_off;
    o.cam_idx = s.cam_idx;
    o.cam_pt = s.cam_pt;
    o.pt_id = s.pt_id;
    o.n_points = s.n_points;
    o.oxy = s.oxy;
    o.points = map ? s.points : nullptr;
    o.map = map;
    o.map_cap = map_cap;
    return o;
}

}  // namespace

// The LM's block is sized from the staged counts (the largest problem's points
// and observations, one download of 3 P ints behind the placing pass), not from
// the worst case W cap: at ~200 bytes per point the block of 256 windows of 8 x
// 2000 features (~2070 points each, not 16384) is several times smaller. The
// staging's own 12 bytes per possible observation are sized for the worst case.
int svo::ba_adjust_device(svo_ctx* ctx, const BaDeviceWindow& w, const double K[9], double huber_delta,
                          int max_iterations, double* costs, int* iterations, int* sizes) {
    const BaLists& l = w.lists;
    const size_t P = (size_t)l.P;
    hipStream_t st = ctx->stream;
    BaStageWork wk;
    int rc = stage_work(ctx, l, wk);
    if (rc) return rc;
    SVO_HIP(ctx, launch_ba_stage_place(l, wk, st));
    std::vector<int> h_nc(P), h_nm(P), h_no(P);
    SVO_HIP(ctx, hipMemcpyAsync(h_nc.data(), w.n_cams, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(h_nm.data(), wk.n_points, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(h_no.data(), wk.n_obs, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    int maxM = 1, maxO = 1;  // (an all-empty batch keeps non-empty arrays)
    for (size_t p = 0; p < P; p++) {
        if (h_nm[p] < 0 || h_no[p] < 0 || h_nm[p] > h_no[p] || h_no[p] > l.W * l.cap)
            return set_error(ctx, SVO_ERR_HIP, "bundle adjustment staging: counts out of range");
        maxM = std::max(maxM, h_nm[p]);
        maxO = std::max(maxO, h_no[p]);
    }
    Staged s;
    const double baseline = l.ur ? w.baseline : 0.0;
    if ((rc = alloc_staged(ctx, Sizes{l.P, l.W, maxM, maxO, baseline}, K, huber_delta, false, false, true, s)))
        return rc;
    if ((rc = zero_observations(ctx, s))) return rc;
    SVO_HIP(ctx, hipMemcpyAsync(s.n_cams, w.n_cams, sizeof(int) * P, hipMemcpyDeviceToDevice, st));
    SVO_HIP(ctx, launch_ba_stage_fill(l, wk, stage_out(s, w.map, w.map_cap), st));
    SVO_HIP(ctx, launch_ba_stage_cams(l, w.n_cams, w.ring, w.n_fixed, s.poses, s.fixed, st));
    std::vector<double> c_first, c_cur;
    std::vector<int> its;
    if ((rc = run_lm(ctx, s, max_iterations, {}, c_first, c_cur, its))) return rc;
    SVO_HIP(ctx, launch_ba_stage_unstage(l, w.n_cams, s.n_points, s.pt_id, maxM, s.points, s.poses, s.fixed, w.map,
                                         w.map_cap, w.ring, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    for (size_t p = 0; p < P; p++) {
        if (costs) {
            costs[2 * p] = c_first[p];
            costs[2 * p + 1] = c_cur[p];
        }
        if (iterations) iterations[p] = its[p];
        if (sizes) {
            sizes[3 * p] = h_nc[p];
            sizes[3 * p + 1] = h_nm[p];
            sizes[3 * p + 2] = h_no[p];
        }
    }
    return SVO_OK;
}

extern "C" {

// svo_ba_stage_lists, and with ur (not null) svo_ba_stage_lists_stereo
static int stage_lists_entry(svo_ctx* ctx, const char* who, int n_problems, int n_cams, int cap, const int* counts,
                             const int* ids, const float* xy, const float* ur, int* ocam, float* oxy, float* our,
                             int* pt_off, int* cam_off, int* cam_idx, int* cam_pt, int* pt_id, int* n_points,
                             int* n_obs) {
    if (const char* why = check_lists(n_problems, n_cams, cap, counts, ids, xy))
        return set_error(ctx, SVO_ERR_ARG, "%s: %s", who, why);
    if (n_problems == 0) return SVO_OK;
    const size_t P = (size_t)n_problems, WC = (size_t)n_cams * cap, nO = P * WC;
    // the outputs are a block of the BA's own layout with max_points = max_obs = n_cams * cap
    hipStream_t st = ctx->stream;
    BaLists l;
    BaStageWork wk;
    int rc = upload_lists(ctx, n_problems, n_cams, cap, counts, ids, xy, l, ur);
    if (rc || (rc = stage_work(ctx, l, wk))) return rc;
    const double K[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    Staged s;
    // (the baseline only asks for the `our` plane: no BA kernel runs here)
    if ((rc = alloc_staged(ctx, Sizes{n_problems, n_cams, (int)WC, (int)WC, ur ? 1.0 : 0.0}, K, 0.0, false, false, true,
                           s)))
        return rc;
    if ((rc = zero_observations(ctx, s))) return rc;
    SVO_HIP(ctx, hipMemsetAsync(s.pt_id, 0, sizeof(int) * nO, st));
    SVO_HIP(ctx, launch_ba_stage_place(l, wk, st));
    SVO_HIP(ctx, launch_ba_stage_fill(l, wk, stage_out(s, nullptr, 0), st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    auto down = [&](void* dst, const void* src, size_t n) {
        return dst && n ? hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) : hipSuccess;
    };
    SVO_HIP(ctx, down(ocam, s.ocam, sizeof(int) * nO));
    SVO_HIP(ctx, down(oxy, s.oxy, sizeof(float) * 2 * nO));
    if (s.our) SVO_HIP(ctx, down(our, s.our, sizeof(float) * nO));
    SVO_HIP(ctx, down(pt_off, s.pt_off, sizeof(int) * P * (WC + 1)));
    SVO_HIP(ctx, down(cam_off, s.cam_off, sizeof(int) * P * (n_cams + 1)));
    SVO_HIP(ctx, down(cam_idx, s.cam_idx, sizeof(int) * nO));
    SVO_HIP(ctx, down(cam_pt, s.cam_pt, sizeof(int) * nO));
    SVO_HIP(ctx, down(pt_id, s.pt_id, sizeof(int) * nO));
    SVO_HIP(ctx, down(n_points, s.n_points, sizeof(int) * P));
    SVO_HIP(ctx, down(n_obs, wk.n_obs, sizeof(int) * P));
    return SVO_OK;
}

int svo_ba_stage_lists(svo_ctx* ctx, int n_problems, int n_cams, int cap, const int* counts, const int* ids,
                       const float* xy, int* ocam, float* oxy, int* pt_off, int* cam_off, int* cam_idx, int* cam_pt,
                       int* pt_id, int* n_points, int* n_obs) {
    if (!ctx) return SVO_ERR_ARG;
    return stage_lists_entry(ctx, "svo_ba_stage_lists", n_problems, n_cams, cap, counts, ids, xy, nullptr, ocam, oxy,
                             nullptr, pt_off, cam_off, cam_idx, cam_pt, pt_id, n_points, n_obs);
}

int svo_ba_stage_lists_stereo(svo_ctx* ctx, int n_problems, int n_cams, int cap, const int* counts, const int* ids,
                              const float* xy, const float* ur, int* ocam, float* oxy, float* our, int* pt_off,
                              int* cam_off, int* cam_idx, int* cam_pt, int* pt_id, int* n_points, int* n_obs) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_problems > 0 && !ur) return set_error(ctx, SVO_ERR_ARG, "svo_ba_stage_lists_stereo: ur is null");
    return stage_lists_entry(ctx, "svo_ba_stage_lists_stereo", n_problems, n_cams, cap, counts, ids, xy, ur, ocam, oxy,
                             our, pt_off, cam_off, cam_idx, cam_pt, pt_id, n_points, n_obs);
}

int svo_ba_time_staging(svo_ctx* ctx, int n_problems, int n_cams, int cap, const int* counts, const int* ids,
                        const float* xy, int reps, double* ms_device, double* ms_host_readback,
                        double* ms_host_stage) {
    if (!ctx) return SVO_ERR_ARG;
    if (n_problems < 1 || reps < 1 || !ms_device || !ms_host_readback || !ms_host_stage)
        return set_error(ctx, SVO_ERR_ARG, "svo_ba_time_staging: bad arguments");
    if (const char* why = check_lists(n_problems, n_cams, cap, counts, ids, xy))
        return set_error(ctx, SVO_ERR_ARG, "svo_ba_time_staging: %s", why);
    const size_t P = (size_t)n_problems, nL = P * n_cams, nO = nL * cap;
    hipStream_t st = ctx->stream;
    BaLists l;
    BaStageWork wk;
    int rc = upload_lists(ctx, n_problems, n_cams, cap, counts, ids, xy, l);
    if (rc || (rc = stage_work(ctx, l, wk))) return rc;
    // the counts size the block, as in ba_adjust_device
    SVO_HIP(ctx, launch_ba_stage_place(l, wk, st));
    std::vector<int> h_nm(P), h_no(P);
    SVO_HIP(ctx, hipMemcpyAsync(h_nm.data(), wk.n_points, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipMemcpyAsync(h_no.data(), wk.n_obs, sizeof(int) * P, hipMemcpyDeviceToHost, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    const int maxM = std::max(1, *std::max_element(h_nm.begin(), h_nm.end()));
    const int maxO = std::max(1, *std::max_element(h_no.begin(), h_no.end()));
    const double K[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    Staged s;
    if ((rc = alloc_staged(ctx, Sizes{n_problems, n_cams, maxM, maxO}, K, 0.0, false, false, true, s))) return rc;
    hipEvent_t e0, e1;
    SVO_HIP(ctx, hipEventCreate(&e0));
    SVO_HIP(ctx, hipEventCreate(&e1));
    rc = SVO_OK;
    for (int r = -1; r < reps && rc == SVO_OK; r++) {  // r = -1: warm-up
        if (r == 0 && hipEventRecord(e0, st) != hipSuccess) rc = set_error(ctx, SVO_ERR_HIP, "hipEventRecord");
        if (rc == SVO_OK && launch_ba_stage_place(l, wk, st) != hipSuccess)
            rc = set_error(ctx, SVO_ERR_HIP, "launch_ba_stage_place");
        if (rc == SVO_OK) rc = zero_observations(ctx, s);
        if (rc == SVO_OK && launch_ba_stage_fill(l, wk, stage_out(s, nullptr, 0), st) != hipSuccess)
            rc = set_error(ctx, SVO_ERR_HIP, "launch_ba_stage_fill");
    }
    float ms = 0;
    if (rc == SVO_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                         hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
        rc = set_error(ctx, SVO_ERR_HIP, "svo_ba_time_staging: events");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    *ms_device = (double)ms / reps;
    // the host's way: the lists come down ...
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    {
        std::vector<int> b_counts(nL), b_ids(nO);
        std::vector<float> b_xy(2 * nO);
        const auto t0 = clk::now();
        SVO_HIP(ctx, hipMemcpyAsync(b_counts.data(), l.counts, sizeof(int) * nL, hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipMemcpyAsync(b_ids.data(), l.ids, sizeof(int) * nO, hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipMemcpyAsync(b_xy.data(), l.xy, sizeof(float) * 2 * nO, hipMemcpyDeviceToHost, st));
        SVO_HIP(ctx, hipStreamSynchronize(st));
        *ms_host_readback = ms_since(t0);
    }
    // ... become svo_bundle_adjust's arrays (camera by camera, points numbered by
    // ascending id: untimed), and stage() sorts and uploads them
    std::vector<int> oc(P * maxO, 0), op(P * maxO, 0);
    std::vector<float> oxy(2 * P * maxO, 0.f);
    for (size_t p = 0; p < P; p++) {
        std::vector<int> pid;
        for (int j = 0; j < n_cams; j++)
            pid.insert(pid.end(), ids + (p * n_cams + j) * cap, ids + (p * n_cams + j) * cap + counts[p * n_cams + j]);
        std::sort(pid.begin(), pid.end());
        pid.erase(std::unique(pid.begin(), pid.end()), pid.end());
        size_t k = p * maxO;
        for (int j = 0; j < n_cams; j++)
            for (int q = 0; q < counts[p * n_cams + j]; q++, k++) {
                const size_t src = (p * n_cams + j) * cap + q;
                oc[k] = j;
                op[k] = (int)(std::lower_bound(pid.begin(), pid.end(), ids[src]) - pid.begin());
                oxy[2 * k] = xy[2 * src];
                oxy[2 * k + 1] = xy[2 * src + 1];
            }
    }
    const std::vector<double> poses(12 * P * n_cams, 0.0), points(3 * P * maxM, 0.0);
    const std::vector<uint8_t> fixed(P * n_cams, 1);
    const Args a{n_problems, n_cams, maxM, maxO, nullptr, h_nm.data(), h_no.data(), poses.data(), fixed.data(),
                 points.data(), oc.data(), op.data(), oxy.data(), K, 0.0};
    const auto t0 = clk::now();
    Staged hs;
    if ((rc = stage(ctx, a, false, false, hs))) return rc;
    *ms_host_stage = ms_since(t0);
    return SVO_OK;
}

int svo_ba_sort_observations(const int* obs_cam, const int* obs_point, int n_obs, int n_cams, int n_points,
                             int* order, int* pt_off, int* cam_off, int* cam_idx) {
    if (n_obs < 0 || n_cams < 0 || n_points < 0 || !pt_off || !cam_off) return SVO_ERR_ARG;
    if (n_obs > 0 && (!obs_cam || !obs_point || !order || !cam_idx)) return SVO_ERR_ARG;
    for (int k = 0; k < n_obs; k++)
        if (obs_cam[k] < 0 || obs_cam[k] >= n_cams || obs_point[k] < 0 || obs_point[k] >= n_points)
            return SVO_ERR_ARG;
    sort_observations(obs_cam, obs_point, n_obs, n_cams, n_points, order, pt_off, cam_off, cam_idx);
    return SVO_OK;
}

// svo_ba_linearize and svo_ba_linearize_stereo (a.obs_ur set, checked by the caller)
static int linearize_entry(svo_ctx* ctx, const char* who, const Args& a, double lambda, double* U, double* gc,
                           double* V, double* gp, double* cost, double* S, double* b, double* dc, double* dp,
                           int* n_free, int* status) {
    const int n_problems = a.P, max_cams = a.maxC, max_points = a.maxM;
    const int *n_cams = a.n_cams, *n_points = a.n_points;
    if (const char* why = check(a)) return set_error(ctx, SVO_ERR_ARG, "%s: %s", who, why);
    if (!(lambda >= 0) || !std::isfinite(lambda)) return set_error(ctx, SVO_ERR_ARG, "%s: lambda", who);
    if (n_problems == 0) return SVO_OK;
    Staged s;
    int rc = stage(ctx, a, S || b, dp != nullptr, s);
    if (rc) return rc;
    const size_t P = (size_t)n_problems, nC = P * max_cams, nM = P * max_points;
    if ((rc = send_control(ctx, s, std::vector<double>(P, lambda), std::vector<int>(P, 1)))) return rc;
    hipStream_t st = ctx->stream;
    SVO_HIP(ctx, launch_ba_linearize(s.b, s.poses, s.points, st));
    SVO_HIP(ctx, launch_ba_cost(s.b, s.poses, s.points, s.cost, st));
    if ((rc = launch_solve_chain(ctx, s))) return rc;
    SVO_HIP(ctx, hipStreamSynchronize(st));
    auto down = [&](void* dst, const void* src, size_t n) {
        return dst && n ? hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) : hipSuccess;
    };
    if (U || gc) {
        std::vector<double> ne(kNE * nC);
        SVO_HIP(ctx, down(ne.data(), s.b.cam_ne, sizeof(double) * ne.size()));
        for (size_t p = 0; p < P; p++)
            for (int j = 0; j < max_cams; j++) {
                const size_t cj = p * max_cams + j;
                const bool live = j < (n_cams ? n_cams[p] : max_cams);
                for (int q = 0; q < 21 && U; q++) U[21 * cj + q] = live ? ne[kNE * cj + q] : 0;
                for (int q = 0; q < 6 && gc; q++) gc[6 * cj + q] = live ? ne[kNE * cj + 21 + q] : 0;
            }
    }
    if (V || gp) {
        std::vector<double> hv(6 * nM), hg(3 * nM);
        SVO_HIP(ctx, down(hv.data(), s.b.pt_V, sizeof(double) * hv.size()));
        SVO_HIP(ctx, down(hg.data(), s.b.pt_g, sizeof(double) * hg.size()));
        for (size_t p = 0; p < P; p++)
            for (int i = 0; i < max_points; i++) {
                const size_t pi = p * max_points + i;
                const bool live = i < (n_points ? n_points[p] : max_points);
                for (int q = 0; q < 6 && V; q++) V[6 * pi + q] = live ? hv[6 * pi + q] : 0;
                for (int q = 0; q < 3 && gp; q++) gp[3 * pi + q] = live ? hg[3 * pi + q] : 0;
            }
    }
    const size_t ld = 6 * (size_t)max_cams;
    SVO_HIP(ctx, down(cost, s.cost, sizeof(double) * P));
    SVO_HIP(ctx, down(S, s.S, sizeof(double) * P * ld * ld));
    SVO_HIP(ctx, down(b, s.bvec, sizeof(double) * P * ld));
    SVO_HIP(ctx, down(dc, s.b.dc, sizeof(double) * 6 * nC));
    if (dp) {
        std::vector<double> hd(3 * nM);
        SVO_HIP(ctx, down(hd.data(), s.dp, sizeof(double) * hd.size()));
        for (size_t p = 0; p < P; p++)
            for (int i = 0; i < max_points; i++)
                for (int q = 0; q < 3; q++) {
                    const size_t k = 3 * (p * max_points + i) + q;
                    dp[k] = i < (n_points ? n_points[p] : max_points) ? hd[k] : 0;
                }
    }
    SVO_HIP(ctx, down(n_free, s.b.n_free, sizeof(int) * P));
    SVO_HIP(ctx, down(status, s.b.status, sizeof(int) * P));
    return SVO_OK;
}

int svo_ba_linearize(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs, const int* n_cams,
                     const int* n_points, const int* n_obs, const double* poses, const uint8_t* fixed,
                     const double* points, const int* obs_cam, const int* obs_point, const float* obs_xy,
                     const double K[9], double huber_delta, double lambda, double* U, double* gc, double* V,
                     double* gp, double* cost, double* S, double* b, double* dc, double* dp, int* n_free,
                     int* status) {
    if (!ctx) return SVO_ERR_ARG;
    const Args a{n_problems, max_cams, max_points, max_obs, n_cams, n_points, n_obs, poses,
                 fixed,      points,   obs_cam,    obs_point, obs_xy, K,       huber_delta};
    return linearize_entry(ctx, "svo_ba_linearize", a, lambda, U, gc, V, gp, cost, S, b, dc, dp, n_free, status);
}

int svo_ba_linearize_stereo(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs,
                            const int* n_cams, const int* n_points, const int* n_obs, const double* poses,
                            const uint8_t* fixed, const double* points, const int* obs_cam, const int* obs_point,
                            const float* obs_xy, const float* obs_ur, double baseline, const double K[9],
                            double huber_delta, double lambda, double* U, double* gc, double* V, double* gp,
                            double* cost, double* S, double* b, double* dc, double* dp, int* n_free, int* status) {
    if (!ctx) return SVO_ERR_ARG;
    if (const char* why = check_stereo(obs_ur, baseline))
        return set_error(ctx, SVO_ERR_ARG, "svo_ba_linearize_stereo: %s", why);
    const Args a{n_problems, max_cams, max_points, max_obs, n_cams,      n_points, n_obs,  poses,   fixed,
                 points,     obs_cam,  obs_point,  obs_xy,  K,           huber_delta,      obs_ur,  baseline};
    return linearize_entry(ctx, "svo_ba_linearize_stereo", a, lambda, U, gc, V, gp, cost, S, b, dc, dp, n_free,
                           status);
}

// svo_bundle_adjust and svo_bundle_adjust_stereo (a.obs_ur set, checked by the caller)
static int adjust_entry(svo_ctx* ctx, const char* who, const Args& a, double* poses, double* points,
                        int max_iterations, double* costs, int* iterations) {
    const int n_problems = a.P, max_cams = a.maxC, max_points = a.maxM;
    const int *n_cams = a.n_cams, *n_points = a.n_points;
    if (const char* why = check(a)) return set_error(ctx, SVO_ERR_ARG, "%s: %s", who, why);
    if (max_iterations < 0) return set_error(ctx, SVO_ERR_ARG, "%s: max_iterations < 0", who);
    if (n_problems == 0) return SVO_OK;
    Staged s;
    int rc = stage(ctx, a, false, false, s);
    if (rc) return rc;
    const size_t P = (size_t)n_problems;
    std::vector<double> c_first, c_cur;
    std::vector<int> its;
    if ((rc = run_lm(ctx, s, max_iterations, non_finite(a), c_first, c_cur, its))) return rc;
    // the device state is the caller's input wherever nothing was accepted
    const size_t nC = P * max_cams, nM = P * max_points;
    std::vector<double> hp(12 * nC), hx(3 * nM);
    if (nC) SVO_HIP(ctx, hipMemcpy(hp.data(), s.poses, sizeof(double) * hp.size(), hipMemcpyDeviceToHost));
    if (nM) SVO_HIP(ctx, hipMemcpy(hx.data(), s.points, sizeof(double) * hx.size(), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < P; p++) {
        const int C = n_cams ? n_cams[p] : max_cams, M = n_points ? n_points[p] : max_points;
        std::memcpy(poses + 12 * p * max_cams, hp.data() + 12 * p * max_cams, sizeof(double) * 12 * C);
        std::memcpy(points + 3 * p * max_points, hx.data() + 3 * p * max_points, sizeof(double) * 3 * M);
        if (costs) {
            costs[2 * p] = c_first[p];
            costs[2 * p + 1] = c_cur[p];
        }
        if (iterations) iterations[p] = its[p];
    }
    return SVO_OK;
}

int svo_bundle_adjust(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs, const int* n_cams,
                      const int* n_points, const int* n_obs, double* poses, const uint8_t* fixed, double* points,
                      const int* obs_cam, const int* obs_point, const float* obs_xy, const double K[9],
                      double huber_delta, int max_iterations, double* costs, int* iterations) {
    if (!ctx) return SVO_ERR_ARG;
    const Args a{n_problems, max_cams, max_points, max_obs, n_cams, n_points, n_obs, poses,
                 fixed,      points,   obs_cam,    obs_point, obs_xy, K,       huber_delta};
    return adjust_entry(ctx, "svo_bundle_adjust", a, poses, points, max_iterations, costs, iterations);
}

int svo_bundle_adjust_stereo(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs,
                             const int* n_cams, const int* n_points, const int* n_obs, double* poses,
                             const uint8_t* fixed, double* points, const int* obs_cam, const int* obs_point,
                             const float* obs_xy, const float* obs_ur, double baseline, const double K[9],
                             double huber_delta, int max_iterations, double* costs, int* iterations) {
    if (!ctx) return SVO_ERR_ARG;
    if (const char* why = check_stereo(obs_ur, baseline))
        return set_error(ctx, SVO_ERR_ARG, "svo_bundle_adjust_stereo: %s", why);
    const Args a{n_problems, max_cams, max_points, max_obs, n_cams,      n_points, n_obs,  poses,   fixed,
                 points,     obs_cam,  obs_point,  obs_xy,  K,           huber_delta,      obs_ur,  baseline};
    return adjust_entry(ctx, "svo_bundle_adjust_stereo", a, poses, points, max_iterations, costs, iterations);
}

int svo_ba_time_iteration(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs, const int* n_cams,
                          const int* n_points, const int* n_obs, const double* poses, const uint8_t* fixed,
                          const double* points, const int* obs_cam, const int* obs_point, const float* obs_xy,
                          const double K[9], double huber_delta, double lambda, int reps, double* ms_per_iteration) {
    if (!ctx) return SVO_ERR_ARG;
    const Args a{n_problems, max_cams, max_points, max_obs, n_cams, n_points, n_obs, poses,
                 fixed,      points,   obs_cam,    obs_point, obs_xy, K,       huber_delta};
    if (const char* why = check(a)) return set_error(ctx, SVO_ERR_ARG, "svo_ba_time_iteration: %s", why);
    if (reps <= 0 || !ms_per_iteration || n_problems <= 0 || !(lambda >= 0))
        return set_error(ctx, SVO_ERR_ARG, "svo_ba_time_iteration: bad arguments");
    Staged s;
    int rc = stage(ctx, a, false, false, s);
    if (rc) return rc;
    const size_t P = (size_t)n_problems;
    if ((rc = send_control(ctx, s, std::vector<double>(P, lambda), std::vector<int>(P, 1)))) return rc;
    hipStream_t st = ctx->stream;
    hipEvent_t e0, e1;
    SVO_HIP(ctx, hipEventCreate(&e0));
    SVO_HIP(ctx, hipEventCreate(&e1));
    rc = SVO_OK;
    for (int r = -1; r < reps && rc == SVO_OK; r++) {  // r = -1: warm-up
        if (r == 0 && hipEventRecord(e0, st) != hipSuccess) rc = set_error(ctx, SVO_ERR_HIP, "hipEventRecord");
        if (rc == SVO_OK && launch_ba_linearize(s.b, s.poses, s.points, st) != hipSuccess)
            rc = set_error(ctx, SVO_ERR_HIP, "launch_ba_linearize");
        if (rc == SVO_OK) rc = launch_solve_chain(ctx, s);
    }
    float ms = 0;
    if (rc == SVO_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                         hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
        rc = set_error(ctx, SVO_ERR_HIP, "svo_ba_time_iteration: events");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == SVO_OK) *ms_per_iteration = (double)ms / reps;
    return rc;
}

}  // extern "C"
