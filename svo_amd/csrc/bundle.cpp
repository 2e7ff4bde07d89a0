// Windowed bundle adjustment C ABI: staging of the ragged
// problem batch (observations sorted by (point, camera), index lists per point
// and per camera) and the Levenberg-Marquardt control over the device stages of
// ba.hip. Poses, points and observations go up once and come down once; per
// iteration the host reads a cost, a status flag and the step size per problem
// and sends back lambda and the accept / active flags.
#include <cmath>
#include <cstring>
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
};

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
};

int stage(svo_ctx* ctx, const Args& a, bool want_S, bool want_dp, Staged& s) {
    const size_t P = (size_t)a.P, nC = P * a.maxC, nM = P * a.maxM, nO = P * a.maxO;
    std::vector<int> h_nc(P), h_nm(P), ocam(nO, 0), pt_off(P * (a.maxM + 1), 0), cam_off(P * (a.maxC + 1), 0),
        cam_idx(nO, 0), cam_pt(nO, 0), order((size_t)a.maxO);
    std::vector<float> oxy(2 * nO, 0.f);
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
        }
        for (int k = 0; k < O; k++) cam_pt[p * a.maxO + k] = pt[order[cam_idx[p * a.maxO + k]]];
    }
    s.nblk = ba_point_blocks(a.maxM);
    const size_t ld = 6 * (size_t)a.maxC;
    const size_t dbl = 2 * 12 * nC + 2 * 3 * nM + kBaNE * nC + 6 * nM + 3 * nM + 6 * nM + 6 * nC +
                       2 * P * s.nblk + 2 * P + nC + 3 * P + (want_S ? P * ld * ld + P * ld : 0) +
                       (want_dp ? 3 * nM : 0);
    const size_t ints = 2 * P + 3 * nO + P * (a.maxM + 1) + P * (a.maxC + 1) + nC + nM + 4 * P;
    const size_t bytes = sizeof(double) * dbl + sizeof(int) * ints + sizeof(float) * 2 * nO + nC + 64 * 256;
    char* d = (char*)scratch(ctx, 11, bytes);
    if (!d) return set_error(ctx, SVO_ERR_HIP, "scratch alloc");
    auto carve = [&](size_t n) {
        d = (char*)(((uintptr_t)d + 255) & ~(uintptr_t)255);
        char* r = d;
        d += n;
        return r;
    };
    auto dd = [&](size_t n) { return (double*)carve(sizeof(double) * n); };
    auto di = [&](size_t n) { return (int*)carve(sizeof(int) * n); };
    BaBatch& b = s.b;
    b.P = a.P;
    b.maxC = a.maxC;
    b.maxM = a.maxM;
    b.maxO = a.maxO;
    b.fx = a.K[0];
    b.fy = a.K[4];
    b.cx = a.K[2];
    b.cy = a.K[5];
    b.delta = a.delta;
    s.poses = dd(12 * nC);
    s.tposes = dd(12 * nC);
    s.points = dd(3 * nM);
    s.tpoints = dd(3 * nM);
    b.cam_ne = dd(kBaNE * nC);
    b.pt_V = dd(6 * nM);
    b.pt_g = dd(3 * nM);
    b.pt_Vinv = dd(6 * nM);
    b.dc = dd(6 * nC);
    b.step_part = dd(2 * P * s.nblk);
    b.stepinfo = dd(2 * P);
    b.cam_cost = dd(nC);
    s.cost = dd(P);
    s.tcost = dd(P);
    s.lambda = dd(P);
    s.S = want_S ? dd(P * ld * ld) : nullptr;
    s.bvec = want_S ? dd(P * ld) : nullptr;
    s.dp = want_dp ? dd(3 * nM) : nullptr;
    int* d_nc = di(P);
    int* d_nm = di(P);
    int* d_ocam = di(nO);
    int* d_cam_idx = di(nO);
    int* d_cam_pt = di(nO);
    int* d_pt_off = di(P * (a.maxM + 1));
    int* d_cam_off = di(P * (a.maxC + 1));
    b.cam_cnt = di(nC);
    b.pt_free = di(nM);
    b.status = di(P);
    b.n_free = di(P);
    s.active = di(P);
    s.accept = di(P);
    float* d_oxy = (float*)carve(sizeof(float) * 2 * nO);
    uint8_t* d_fixed = (uint8_t*)carve(nC);
    b.n_cams = d_nc;
    b.n_points = d_nm;
    b.ocam = d_ocam;
    b.cam_idx = d_cam_idx;
    b.cam_pt = d_cam_pt;
    b.pt_off = d_pt_off;
    b.cam_off = d_cam_off;
    b.oxy = d_oxy;
    b.fixed = d_fixed;
    b.lambda = s.lambda;
    b.active = s.active;
    hipStream_t st = ctx->stream;
    auto up = [&](void* dst, const void* src, size_t n) {
        return n ? hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    SVO_HIP(ctx, up(s.poses, a.poses, sizeof(double) * 12 * nC));
    SVO_HIP(ctx, up(s.points, a.points, sizeof(double) * 3 * nM));
    SVO_HIP(ctx, up(d_fixed, a.fixed, nC));
    SVO_HIP(ctx, up(d_nc, h_nc.data(), sizeof(int) * P));
    SVO_HIP(ctx, up(d_nm, h_nm.data(), sizeof(int) * P));
    SVO_HIP(ctx, up(d_ocam, ocam.data(), sizeof(int) * nO));
    SVO_HIP(ctx, up(d_cam_idx, cam_idx.data(), sizeof(int) * nO));
    SVO_HIP(ctx, up(d_cam_pt, cam_pt.data(), sizeof(int) * nO));
    SVO_HIP(ctx, up(d_pt_off, pt_off.data(), sizeof(int) * pt_off.size()));
    SVO_HIP(ctx, up(d_cam_off, cam_off.data(), sizeof(int) * cam_off.size()));
    SVO_HIP(ctx, up(d_oxy, oxy.data(), sizeof(float) * 2 * nO));
    if (s.S) {
        SVO_HIP(ctx, hipMemsetAsync(s.S, 0, sizeof(double) * P * ld * ld, st));
        SVO_HIP(ctx, hipMemsetAsync(s.bvec, 0, sizeof(double) * P * ld, st));
    }
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

}  // namespace

extern "C" {

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

int svo_ba_linearize(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs, const int* n_cams,
                     const int* n_points, const int* n_obs, const double* poses, const uint8_t* fixed,
                     const double* points, const int* obs_cam, const int* obs_point, const float* obs_xy,
                     const double K[9], double huber_delta, double lambda, double* U, double* gc, double* V,
                     double* gp, double* cost, double* S, double* b, double* dc, double* dp, int* n_free,
                     int* status) {
    if (!ctx) return SVO_ERR_ARG;
    const Args a{n_problems, max_cams, max_points, max_obs, n_cams, n_points, n_obs, poses,
                 fixed,      points,   obs_cam,    obs_point, obs_xy, K,       huber_delta};
    if (const char* why = check(a)) return set_error(ctx, SVO_ERR_ARG, "svo_ba_linearize: %s", why);
    if (!(lambda >= 0) || !std::isfinite(lambda)) return set_error(ctx, SVO_ERR_ARG, "svo_ba_linearize: lambda");
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
        std::vector<double> ne(kBaNE * nC);
        SVO_HIP(ctx, down(ne.data(), s.b.cam_ne, sizeof(double) * ne.size()));
        for (size_t p = 0; p < P; p++)
            for (int j = 0; j < max_cams; j++) {
                const size_t cj = p * max_cams + j;
                const bool live = j < (n_cams ? n_cams[p] : max_cams);
                for (int q = 0; q < 21 && U; q++) U[21 * cj + q] = live ? ne[kBaNE * cj + q] : 0;
                for (int q = 0; q < 6 && gc; q++) gc[6 * cj + q] = live ? ne[kBaNE * cj + 21 + q] : 0;
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

int svo_bundle_adjust(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs, const int* n_cams,
                      const int* n_points, const int* n_obs, double* poses, const uint8_t* fixed, double* points,
                      const int* obs_cam, const int* obs_point, const float* obs_xy, const double K[9],
                      double huber_delta, int max_iterations, double* costs, int* iterations) {
    if (!ctx) return SVO_ERR_ARG;
    const Args a{n_problems, max_cams, max_points, max_obs, n_cams, n_points, n_obs, poses,
                 fixed,      points,   obs_cam,    obs_point, obs_xy, K,       huber_delta};
    if (const char* why = check(a)) return set_error(ctx, SVO_ERR_ARG, "svo_bundle_adjust: %s", why);
    if (max_iterations < 0) return set_error(ctx, SVO_ERR_ARG, "svo_bundle_adjust: max_iterations < 0");
    if (n_problems == 0) return SVO_OK;
    Staged s;
    int rc = stage(ctx, a, false, false, s);
    if (rc) return rc;
    const size_t P = (size_t)n_problems;
    hipStream_t st = ctx->stream;
    std::vector<double> lambda(P, 1e-4), c_cur(P), c_first(P), c_trial(P), stepinfo(2 * P);
    std::vector<int> active(P, 1), accept(P), status(P), done(P, 0), its(P, 0);
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
    c_first = c_cur;
    for (int it = 0; it < max_iterations; it++) {
        bool any = false;
        for (size_t p = 0; p < P; p++) {
            active[p] = !done[p];
            any = any || active[p];
        }
        if (!any) break;
        if ((rc = send_control(ctx, s, lambda, active))) return rc;
        SVO_HIP(ctx, launch_ba_linearize(s.b, s.poses, s.points, st));
        if ((rc = launch_solve_chain(ctx, s))) return rc;
        if ((rc = read_back())) return rc;
        // reduced system not positive definite: raise lambda and solve again from
        // the same linearisation, as lm_solve's caller does
        for (;;) {
            bool retry = false;
            for (size_t p = 0; p < P; p++) {
                const bool again = active[p] && status[p] != 0;
                if (again) {
                    lambda[p] *= 10;
                    if (lambda[p] >= 1e16) {
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
            if (done[p]) continue;
            its[p]++;
            if (active[p] != 2) continue;
            if (std::sqrt(stepinfo[2 * p]) < 1e-12 * (1 + std::sqrt(stepinfo[2 * p + 1]))) {
                done[p] = 1;
                continue;
            }
            const double c0 = c_cur[p], c1 = c_trial[p];
            if (c1 <= c0) {
                accept[p] = 1;
                c_cur[p] = c1;
                lambda[p] = lambda[p] * 0.1 > 1e-12 ? lambda[p] * 0.1 : 1e-12;
                if (c0 - c1 <= 1e-15 * c0) done[p] = 1;
            } else {
                lambda[p] *= 10;
                if (lambda[p] >= 1e16) done[p] = 1;
            }
        }
        SVO_HIP(ctx, hipMemcpyAsync(s.accept, accept.data(), sizeof(int) * P, hipMemcpyHostToDevice, st));
        SVO_HIP(ctx, launch_ba_commit(s.b, s.accept, s.tposes, s.tpoints, s.poses, s.points, st));
        SVO_HIP(ctx, hipStreamSynchronize(st));
    }
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
