// Pose-graph optimisation, the C ABI around pose_graph.hip (§10):
// svo_pose_graph_optimize (one upload, one launch, one download), its test view
// svo_pose_graph_linearize, its timing probe and the host helper that builds an
// edge's measurement.
#include <cmath>
#include <vector>

#include "pose_graph.hpp"

using namespace svo;

namespace {

struct Args {
    int P, max_nodes, max_edges;
    const int *n_nodes, *n_edges;
    const double* poses;
    const uint8_t* fixed;
    const int* ij;
    const double *Z, *info;
    double delta;
    int max_iterations, max_cg;
};

int count_of(const int* counts, int p, int max) { return counts ? counts[p] : max; }

const char* bad_args(const Args& a) {
    if (a.P < 0 || a.max_nodes < 0 || a.max_edges < 0) return "sizes < 0";
    if (a.max_nodes > SVO_PG_MAX_NODES) return "max_nodes above SVO_PG_MAX_NODES";
    if (a.max_edges > SVO_PG_MAX_EDGES) return "max_edges above SVO_PG_MAX_EDGES";
    if (a.max_iterations < 0 || a.max_iterations > SVO_PG_MAX_ITERATIONS)
        return "max_iterations outside 0 .. SVO_PG_MAX_ITERATIONS";
    if (a.max_cg < 1 || a.max_cg > SVO_PG_MAX_CG) return "max_cg outside 1 .. SVO_PG_MAX_CG";
    if (a.P > 0 && a.max_nodes > 0 && (!a.poses || !a.fixed)) return "poses / fixed null";
    if (a.P > 0 && a.max_edges > 0 && (!a.ij || !a.Z || !a.info)) return "edge_ij / edge_Z / edge_info null";
    for (int p = 0; p < a.P; p++) {
        const int N = count_of(a.n_nodes, p, a.max_nodes), E = count_of(a.n_edges, p, a.max_edges);
        if (N < 0 || N > a.max_nodes) return "a node count outside 0 .. max_nodes";
        if (E < 0 || E > a.max_edges) return "an edge count outside 0 .. max_edges";
        const int* ij = a.ij + 2 * (size_t)p * a.max_edges;
        for (int e = 0; e < E; e++) {
            const int i = ij[2 * e], j = ij[2 * e + 1];
            if (i < 0 || i >= N || j < 0 || j >= N) return "an edge names a node outside its problem";
            if (i == j) return "an edge with i == j";
        }
    }
    return nullptr;
}

// Every node's incident edges as 2*edge + end, ascending: a stable counting sort
// of the edge ends by node. start: P*(max_nodes+1), list: P*2*max_edges.
void incidence_lists(const Args& a, std::vector<int>& start, std::vector<int>& list) {
    start.assign((size_t)a.P * (a.max_nodes + 1), 0);
    list.assign((size_t)a.P * 2 * a.max_edges + 1, 0);
    std::vector<int> at(a.max_nodes + 1);
    for (int p = 0; p < a.P; p++) {
        const int N = count_of(a.n_nodes, p, a.max_nodes), E = count_of(a.n_edges, p, a.max_edges);
        const int* ij = a.ij + 2 * (size_t)p * a.max_edges;
        int* s = start.data() + (size_t)p * (a.max_nodes + 1);
        int* l = list.data() + (size_t)p * 2 * a.max_edges;
        for (int e = 0; e < 2 * E; e++) s[ij[e] + 1]++;
        for (int n = 0; n < a.max_nodes; n++) s[n + 1] += s[n];  // (nodes past N: empty lists)
        for (int n = 0; n < N; n++) at[n] = s[n];
        for (int e = 0; e < E; e++) {
            l[at[ij[2 * e]]++] = 2 * e;
            l[at[ij[2 * e + 1]]++] = 2 * e + 1;
        }
    }
}

struct View {
    double *cost, *e, *w, *Ji, *Jj, *node;
};

// the inputs on the device (context stream) and the launch's arguments
int stage(svo_ctx* ctx, const Args& a, bool separate_out, const View* view, PoseGraphBatch& b) {
    std::vector<int> start, list;
    incidence_lists(a, start, list);
    const size_t P = (size_t)a.P, nn = P * a.max_nodes, ne = P * a.max_edges;
    b = PoseGraphBatch{};
    double *d_poses, *d_Z, *d_info;
    uint8_t* d_fixed;
    int *d_ij, *d_start, *d_list, *d_nn, *d_ne;
    if (!carve_scratch(ctx, kScratchPoseGraph, [&](Carver& c) {
            b.poses_in = d_poses = c.take<double>(12 * nn);
            b.poses_out = separate_out ? c.take<double>(12 * nn) : d_poses;
            b.edge_Z = d_Z = c.take<double>(12 * ne);
            b.edge_info = d_info = c.take<double>(21 * ne);
            b.cur = c.take<double>(12 * nn);
            b.trial = c.take<double>(12 * nn);
            b.terms = c.take<double>(kPgEdgeTerms * ne);
            b.node = c.take<double>(27 * nn);
            b.chol = c.take<double>(21 * nn);
            b.costs = c.take<double>(2 * P);
            if (view) {
                b.lin_e = view->e ? c.take<double>(6 * ne) : nullptr;
                b.lin_w = view->w ? c.take<double>(ne) : nullptr;
                b.lin_Ji = view->Ji ? c.take<double>(36 * ne) : nullptr;
                b.lin_Jj = view->Jj ? c.take<double>(36 * ne) : nullptr;
                b.lin_node = view->node ? c.take<double>(27 * nn) : nullptr;
            }
            b.edge_ij = d_ij = c.take<int>(2 * ne);
            b.inc_start = d_start = c.take<int>(start.size());
            b.inc_list = d_list = c.take<int>(list.size());
            b.n_nodes = d_nn = a.n_nodes ? c.take<int>(P) : nullptr;
            b.n_edges = d_ne = a.n_edges ? c.take<int>(P) : nullptr;
            b.iterations = c.take<int>(P);
            b.cg_iterations = c.take<int>(P);
            b.fixed = d_fixed = c.take<uint8_t>(nn);
        }))
        return set_error(ctx, SVO_ERR_HIP, "scratch alloc");
    hipStream_t st = ctx->stream;
    const auto H2D = hipMemcpyHostToDevice;
    if (nn) {
        SVO_HIP(ctx, hipMemcpyAsync(d_poses, a.poses, sizeof(double) * 12 * nn, H2D, st));
        SVO_HIP(ctx, hipMemcpyAsync(d_fixed, a.fixed, nn, H2D, st));
    }
    if (ne) {
        SVO_HIP(ctx, hipMemcpyAsync(d_ij, a.ij, sizeof(int) * 2 * ne, H2D, st));
        SVO_HIP(ctx, hipMemcpyAsync(d_Z, a.Z, sizeof(double) * 12 * ne, H2D, st));
        SVO_HIP(ctx, hipMemcpyAsync(d_info, a.info, sizeof(double) * 21 * ne, H2D, st));
    }
    SVO_HIP(ctx, hipMemcpyAsync(d_start, start.data(), sizeof(int) * start.size(), H2D, st));
    SVO_HIP(ctx, hipMemcpyAsync(d_list, list.data(), sizeof(int) * list.size(), H2D, st));
    if (a.n_nodes) SVO_HIP(ctx, hipMemcpyAsync(d_nn, a.n_nodes, sizeof(int) * P, H2D, st));
    if (a.n_edges) SVO_HIP(ctx, hipMemcpyAsync(d_ne, a.n_edges, sizeof(int) * P, H2D, st));
    // (start and list are pageable: the copies above have left them before they return)
    SVO_HIP(ctx, hipStreamSynchronize(st));
    b.P = a.P, b.max_nodes = a.max_nodes, b.max_edges = a.max_edges;
    b.delta = a.delta;
    b.max_iterations = a.max_iterations, b.max_cg = a.max_cg;
    return SVO_OK;
}

}  // namespace

extern "C" {

int svo_pose_graph_edge(const double* Ti, const double* Tj, double* Z) {
    if (!Ti || !Tj || !Z) return SVO_ERR_ARG;
    double out[12];
    pg_relative(Ti, Tj, out);
    for (int k = 0; k < 12; k++) Z[k] = out[k];
    return SVO_OK;
}

int svo_pose_graph_optimize(svo_ctx* ctx, int n_problems, int max_nodes, int max_edges, const int* n_nodes,
                            const int* n_edges, const double* poses, const uint8_t* fixed, const int* edge_ij,
                            const double* edge_Z, const double* edge_info, double huber_delta, int max_iterations,
                            int max_cg, double* poses_out, double* costs, int* iterations, int* cg_iterations) {
    if (!ctx) return SVO_ERR_ARG;
    const Args a{n_problems, max_nodes, max_edges, n_nodes, n_edges, poses, fixed, edge_ij,
                 edge_Z, edge_info, huber_delta, max_iterations, max_cg};
    if (const char* why = bad_args(a)) return set_error(ctx, SVO_ERR_ARG, "svo_pose_graph_optimize: %s", why);
    if (n_problems > 0 && max_nodes > 0 && !poses_out)
        return set_error(ctx, SVO_ERR_ARG, "svo_pose_graph_optimize: poses_out null");
    if (n_problems == 0) return SVO_OK;
    const size_t P = (size_t)n_problems;
    PoseGraphBatch b;
    if (int rc = stage(ctx, a, false, nullptr, b)) return rc;
    hipStream_t st = ctx->stream;
    SVO_HIP(ctx, launch_pose_graph(b, st));
    const auto D2H = hipMemcpyDeviceToHost;
    if (max_nodes) SVO_HIP(ctx, hipMemcpyAsync(poses_out, b.poses_out, sizeof(double) * 12 * P * max_nodes, D2H, st));
    if (costs) SVO_HIP(ctx, hipMemcpyAsync(costs, b.costs, sizeof(double) * 2 * P, D2H, st));
    if (iterations) SVO_HIP(ctx, hipMemcpyAsync(iterations, b.iterations, sizeof(int) * P, D2H, st));
    if (cg_iterations) SVO_HIP(ctx, hipMemcpyAsync(cg_iterations, b.cg_iterations, sizeof(int) * P, D2H, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    return SVO_OK;
}

int svo_pose_graph_linearize(svo_ctx* ctx, int n_problems, int max_nodes, int max_edges, const int* n_nodes,
                             const int* n_edges, const double* poses, const uint8_t* fixed, const int* edge_ij,
                             const double* edge_Z, const double* edge_info, double huber_delta, double* cost,
                             double* edge_e, double* edge_w, double* edge_Ji, double* edge_Jj, double* node_sums) {
    if (!ctx) return SVO_ERR_ARG;
    const Args a{n_problems, max_nodes, max_edges, n_nodes, n_edges, poses, fixed, edge_ij,
                 edge_Z, edge_info, huber_delta, 0, 1};
    if (const char* why = bad_args(a)) return set_error(ctx, SVO_ERR_ARG, "svo_pose_graph_linearize: %s", why);
    if (n_problems == 0) return SVO_OK;
    const size_t P = (size_t)n_problems, nn = P * max_nodes, ne = P * max_edges;
    const View v{cost, edge_e, edge_w, edge_Ji, edge_Jj, node_sums};
    PoseGraphBatch b;
    if (int rc = stage(ctx, a, false, &v, b)) return rc;
    hipStream_t st = ctx->stream;
    // the view's device arrays start as the caller's: what the kernel does not write stays
    const auto H2D = hipMemcpyHostToDevice;
    const auto D2H = hipMemcpyDeviceToHost;
    struct {
        double* host;
        double* dev;
        size_t n;
    } arr[5] = {{edge_e, b.lin_e, 6 * ne}, {edge_w, b.lin_w, ne}, {edge_Ji, b.lin_Ji, 36 * ne},
                {edge_Jj, b.lin_Jj, 36 * ne}, {node_sums, b.lin_node, 27 * nn}};
    for (auto& x : arr)
        if (x.host && x.n) SVO_HIP(ctx, hipMemcpyAsync(x.dev, x.host, sizeof(double) * x.n, H2D, st));
    SVO_HIP(ctx, launch_pose_graph(b, st));
    for (auto& x : arr)
        if (x.host && x.n) SVO_HIP(ctx, hipMemcpyAsync(x.host, x.dev, sizeof(double) * x.n, D2H, st));
    std::vector<double> c2(2 * P);
    SVO_HIP(ctx, hipMemcpyAsync(c2.data(), b.costs, sizeof(double) * 2 * P, D2H, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    if (cost)
        for (size_t p = 0; p < P; p++) cost[p] = c2[2 * p];
    return SVO_OK;
}

int svo_pose_graph_time(svo_ctx* ctx, int n_problems, int max_nodes, int max_edges, const int* n_nodes,
                        const int* n_edges, const double* poses, const uint8_t* fixed, const int* edge_ij,
                        const double* edge_Z, const double* edge_info, double huber_delta, int max_iterations,
                        int max_cg, int reps, double* ms, int* iterations, int* cg_iterations) {
    if (!ctx) return SVO_ERR_ARG;
    const Args a{n_problems, max_nodes, max_edges, n_nodes, n_edges, poses, fixed, edge_ij,
                 edge_Z, edge_info, huber_delta, max_iterations, max_cg};
    if (const char* why = bad_args(a)) return set_error(ctx, SVO_ERR_ARG, "svo_pose_graph_time: %s", why);
    if (n_problems <= 0 || max_nodes <= 0 || reps <= 0 || !ms)
        return set_error(ctx, SVO_ERR_ARG, "svo_pose_graph_time: bad arguments");
    PoseGraphBatch b;
    // every launch starts from the staged poses: the results go to a block of their own
    if (int rc = stage(ctx, a, true, nullptr, b)) return rc;
    hipStream_t st = ctx->stream;
    hipEvent_t e0, e1;
    SVO_HIP(ctx, hipEventCreate(&e0));
    SVO_HIP(ctx, hipEventCreate(&e1));
    hipError_t e = launch_pose_graph(b, st);  // untimed first
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int i = 0; i < reps && e == hipSuccess; i++) e = launch_pose_graph(b, st);
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float t = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    SVO_HIP(ctx, e);
    *ms = t / reps;
    const size_t P = (size_t)n_problems;
    const auto D2H = hipMemcpyDeviceToHost;
    if (iterations) SVO_HIP(ctx, hipMemcpyAsync(iterations, b.iterations, sizeof(int) * P, D2H, st));
    if (cg_iterations) SVO_HIP(ctx, hipMemcpyAsync(cg_iterations, b.cg_iterations, sizeof(int) * P, D2H, st));
    SVO_HIP(ctx, hipStreamSynchronize(st));
    return SVO_OK;
}

}  // extern "C"
