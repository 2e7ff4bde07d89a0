// Pose-graph optimisation (§10): the node poses of one problem from its relative-
// pose edges, the whole Levenberg-Marquardt -- linearisation, damping, the
// preconditioned conjugate gradients, the trial and its verdict -- run by one
// workgroup of 256 threads inside a single launch. The edge, its Jacobians, the
// robust cost and the terms an edge adds are pose_graph_model.hpp's; the LM rules,
// the pose update and the block reduction are reproj_model.hpp's. All f64.
//
// The order of every sum (include/svo_gpu.h, svo_pose_graph_optimize):
//   - the cost and every dot product: thread t adds entries t, t + 256, ... in
//     ascending order, the 64 lanes of a wave by wave_sum, the four waves by
//     wave_fold;
//   - a node's 21 + 6 sums: its incident edges in ascending edge index, whichever
//     end the node is, starting from the first edge's term (-0 + term);
//   - a row of A p: the damped diagonal block's product, then the incident edges'
//     blocks in that order, each block's row formed first and then added.
// Nothing outside the problem enters an order.
//
// Memory: the conjugate gradients' five vectors x, r, z, p, A p (5 x 6 x 512
// doubles, 120 KB) and the incidence lists (each entry with the node at the
// edge's other end, 17 KB) live in LDS, 137 KB of the CU's 160: the kernel's 500
// registers leave room for one workgroup per CU whatever it declares. The poses,
// the per-edge terms, the node sums and the preconditioner's factors are in the
// batch's scratch. Control: every branch that leads to a barrier tests a
// kernel argument or a value folded from LDS words behind a barrier and made
// scalar with readfirstlane. Loops are bounded: the LM loop by max_iterations, the
// lambda retry by kMaxRetry, the conjugate gradients by max_cg.
#include "pose_graph.hpp"

namespace svo {

namespace {

constexpr int kBlock = 256;
// lambda x10 from its floor 1e-12 passes 1e16 after 28 steps
constexpr int kMaxRetry = 32;

struct Shared {
    double p[6 * SVO_PG_MAX_NODES];
    double z[6 * SVO_PG_MAX_NODES];
    double x[6 * SVO_PG_MAX_NODES];
    double r[6 * SVO_PG_MAX_NODES];
    double Ap[6 * SVO_PG_MAX_NODES];
    uint32_t adj[2 * SVO_PG_MAX_EDGES];           // 2*edge + end | the other end's node << 12
    uint16_t adj_start[SVO_PG_MAX_NODES + 1];     // node n owns adj[adj_start[n] .. adj_start[n + 1])
    double S[2][4][1];  // the waves' partial sums, two sets used in turn
    int F[2][4];
};

// one problem's slice of the batch
struct Problem {
    int N, E;
    size_t ns, es;  // the strides of node / chol and of terms
    const uint8_t* fixed;
    const int* ij;
    const double* Z;
    const double* info;
    double *cur, *trial, *terms, *node, *chol;
};

__device__ __forceinline__ int uniform(bool b) { return __builtin_amdgcn_readfirstlane((int)b); }

// The block's sum of v in the stated order, the same double in every thread. One
// barrier: the set written here is read again only after the next call's barrier.
__device__ __forceinline__ double block_sum(double v, Shared& sh, int& par) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh.S[par][threadIdx.x >> 6][0] = v;
    __syncthreads();
    const double s = wave_fold<1>(sh.S[par], 0);
    par ^= 1;
    return s;
}

__device__ __forceinline__ int block_any(bool b, Shared& sh, int& par) {
    const int a = __any(b);
    if ((threadIdx.x & 63) == 0) sh.F[par][threadIdx.x >> 6] = a;
    __syncthreads();
    const int s = sh.F[par][0] | sh.F[par][1] | sh.F[par][2] | sh.F[par][3];
    par ^= 1;
    return __builtin_amdgcn_readfirstlane(s);
}

// thread t's share of sum a[k] b[k], k < n
__device__ __forceinline__ double dot_part(const double* a, const double* b, int n) {  // (both in LDS)
    double s = (int)threadIdx.x < n ? -0.0 : 0.0;
    for (int k = threadIdx.x; k < n; k += kBlock) s += a[k] * b[k];
    return s;
}

// The cost at `poses`; with `full` also every edge's terms and every node's sums
// (visible to the block on return); with `view` the test view's per-edge outputs.
// Every thread calls it, and `poses` is visible to the block on entry.
__device__ __forceinline__ double linearize(const PoseGraphBatch& B, const Problem& q, const double* poses, bool full,
                                            bool view, Shared& sh, int& par) {
    const int t = threadIdx.x;
    double c = t < q.E ? -0.0 : 0.0;
    for (int e = t; e < q.E; e += kBlock) {
        const int i = min(max(q.ij[2 * e], 0), q.N - 1), j = min(max(q.ij[2 * e + 1], 0), q.N - 1);
        double Ti[12], Tj[12], Z[12], info[21];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            Ti[k] = poses[12 * (size_t)i + k];
            Tj[k] = poses[12 * (size_t)j + k];
            Z[k] = q.Z[12 * (size_t)e + k];
        }
#pragma unroll
        for (int k = 0; k < 21; k++) info[k] = q.info[21 * (size_t)e + k];
        double err[6], Ji[36], Jj[36], w, cost;
        pg_edge_eval(Ti, Tj, Z, info, B.delta, err, Ji, Jj, w, cost);
        c += cost;
        if (full) pg_edge_terms(info, w, err, Ji, Jj, q.terms + e, q.es);
        if (view) {
            const size_t at = (size_t)blockIdx.x * B.max_edges + e;
            if (B.lin_w) B.lin_w[at] = w;
#pragma unroll
            for (int k = 0; k < 6; k++)
                if (B.lin_e) B.lin_e[6 * at + k] = err[k];
#pragma unroll
            for (int k = 0; k < 36; k++) {
                if (B.lin_Ji) B.lin_Ji[36 * at + k] = Ji[k];
                if (B.lin_Jj) B.lin_Jj[36 * at + k] = Jj[k];
            }
        }
    }
    const double cost = block_sum(c, sh, par);  // (its barrier: the terms are written)
    if (full) {
        for (int item = t; item < 27 * q.N; item += kBlock) {
            const int k = item / q.N, n = item - k * q.N;
            const int a0 = sh.adj_start[n], a1 = sh.adj_start[n + 1];
            double s = a1 > a0 ? -0.0 : 0.0;
            for (int a = a0; a < a1; a++) {
                const int code = sh.adj[a] & 4095;
                s += q.terms[(36 + 27 * (code & 1) + k) * q.es + (code >> 1)];
            }
            q.node[k * q.ns + n] = s;
        }
        __syncthreads();
    }
    return cost;
}

// entry (a, b) of a node's damped diagonal block
__device__ __forceinline__ double damped(const Problem& q, int n, int a, int b, double lambda) {
    const int lo = min(a, b), hi = max(a, b);
    const double h = q.node[(size_t)(6 * lo - lo * (lo - 1) / 2 + (hi - lo)) * q.ns + n];
    return a == b ? h + lambda * (h > 0 ? h : 1e-12) : h;
}

// A p over the free nodes, A = H + lambda D: row k = 6 n + c by thread k mod 256
__device__ __forceinline__ void mat_vec(const Problem& q, Shared& sh, double lambda) {
    for (int k = threadIdx.x; k < 6 * q.N; k += kBlock) {
        const int n = k / 6, c = k - 6 * n;
        double acc = 0.0;
        if (!q.fixed[n]) {
            acc = damped(q, n, c, 0, lambda) * sh.p[6 * n];
#pragma unroll
            for (int d = 1; d < 6; d++) acc += damped(q, n, c, d, lambda) * sh.p[6 * n + d];
            const int a1 = sh.adj_start[n + 1];
            for (int a = sh.adj_start[n]; a < a1; a++) {
                const uint32_t entry = sh.adj[a];
                const int e = (entry & 4095) >> 1, end = entry & 1, m = entry >> 12;
                // end 0: row c of J_i' W J_j; end 1: row c of its transpose
                const int first = end ? c : 6 * c, step = end ? 6 : 1;
                double s = q.terms[(size_t)first * q.es + e] * sh.p[6 * m];
#pragma unroll
                for (int d = 1; d < 6; d++) s += q.terms[(size_t)(first + step * d) * q.es + e] * sh.p[6 * m + d];
                acc += s;
            }
        }
        sh.Ap[k] = acc;
    }
}

// The factor of node n's damped block from q.chol
__device__ __forceinline__ void load_factor(const Problem& q, int n, double L[36]) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            if (j <= i) {
                L[6 * i + j] = q.chol[(size_t)k * q.ns + n];
                k++;
            } else {
                L[6 * i + j] = 0;
            }
        }
}

__global__ __launch_bounds__(kBlock) void pose_graph_kernel(PoseGraphBatch B) {
    __shared__ Shared sh;
    const int p = blockIdx.x, t = threadIdx.x;
    int par = 0, fpar = 0;
    // ---- the problem's slice (every value below is uniform over the block)
    Problem q;
    q.N = B.n_nodes ? min(max(B.n_nodes[p], 0), B.max_nodes) : B.max_nodes;
    q.E = B.n_edges ? min(max(B.n_edges[p], 0), B.max_edges) : B.max_edges;
    if (q.N == 0) q.E = 0;
    q.ns = (size_t)B.max_nodes, q.es = (size_t)B.max_edges;
    const size_t node_at = (size_t)p * B.max_nodes, edge_at = (size_t)p * B.max_edges;
    q.fixed = B.fixed + node_at;
    q.ij = B.edge_ij + 2 * edge_at;
    q.Z = B.edge_Z + 12 * edge_at;
    q.info = B.edge_info + 21 * edge_at;
    const int* inc_start = B.inc_start + (size_t)p * (B.max_nodes + 1);
    const int* inc_list = B.inc_list + 2 * edge_at;
    q.cur = B.cur + 12 * node_at;
    q.trial = B.trial + 12 * node_at;
    q.terms = B.terms + (size_t)kPgEdgeTerms * edge_at;
    q.node = B.node + 27 * node_at;
    q.chol = B.chol + 21 * node_at;
    const double* in = B.poses_in + 12 * node_at;
    const int n6 = 6 * q.N, n12 = 12 * q.N;

    // ---- the poses, and the scan for values that are not finite
    bool bad = false;
    for (int k = t; k < n12; k += kBlock) {
        const double v = in[k];
        q.cur[k] = v;
        bad = bad || !isfinite(v);
    }
    for (int k = t; k < 12 * q.E; k += kBlock) bad = bad || !isfinite(q.Z[k]);
    for (int k = t; k < 21 * q.E; k += kBlock) bad = bad || !isfinite(q.info[k]);
    // the incidence lists into LDS, each entry with the node at the other end
    for (int n = t; n <= q.N; n += kBlock) sh.adj_start[n] = (uint16_t)min(max(inc_start[n], 0), 2 * q.E);
    for (int a = t; a < 2 * q.E; a += kBlock) {
        const int code = min(max(inc_list[a], 0), 2 * q.E - 1);
        const int m = min(max(q.ij[2 * (code >> 1) + (1 - (code & 1))], 0), q.N - 1);
        sh.adj[a] = (uint32_t)code | (uint32_t)m << 12;
    }
    const int any_bad = block_any(bad, sh, fpar);  // (its barrier: cur and the lists are written)

    const bool view = B.lin_e || B.lin_w || B.lin_Ji || B.lin_Jj;
    const double c_first = linearize(B, q, q.cur, true, view, sh, par);
    const int poisoned = any_bad || uniform(!isfinite(c_first));
    if (B.lin_node)
        for (int item = t; item < 27 * q.N; item += kBlock) {
            const int k = item / q.N, n = item - k * q.N;
            B.lin_node[27 * (node_at + n) + k] = q.node[k * q.ns + n];
        }

    double c0 = c_first, lambda = kLmLambda0;
    int its = 0, cgs = 0;
    if (!poisoned) {
        for (int it = 0; it < B.max_iterations; it++) {
            its = it + 1;
            // ---- (H + lambda D) x = -g over the free nodes; lambda up while not positive definite
            int solved = 0;
            for (int rt = 0; rt < kMaxRetry && !solved; rt++) {
                if (!uniform(lambda < kLmCeiling)) break;
                bool npd = false;
                for (int n = t; n < q.N; n += kBlock) {
                    double L[36], b[6], zz[6];
                    const bool free_node = !q.fixed[n];
                    if (free_node) {
                        npd = npd || !pg_chol6(q.node + n, q.ns, lambda, L);
                        int k = 0;
#pragma unroll
                        for (int i = 0; i < 6; i++)
#pragma unroll
                            for (int j = 0; j <= i; j++) q.chol[(size_t)(k++) * q.ns + n] = L[6 * i + j];
#pragma unroll
                        for (int k2 = 0; k2 < 6; k2++) b[k2] = -q.node[(size_t)(21 + k2) * q.ns + n];
                        pg_chol6_solve(L, b, zz);
                    }
#pragma unroll
                    for (int k2 = 0; k2 < 6; k2++) {
                        sh.x[6 * n + k2] = 0.0;
                        sh.r[6 * n + k2] = free_node ? b[k2] : 0.0;
                        sh.z[6 * n + k2] = sh.p[6 * n + k2] = free_node ? zz[k2] : 0.0;
                    }
                }
                int not_pd = block_any(npd, sh, fpar);  // (its barrier: x, r, z, p are written)
                if (!not_pd) {
                    const double rz0 = block_sum(dot_part(sh.r, sh.z, n6), sh, par);
                    double rz = rz0;
                    int conv = uniform(rz <= kPgCgTol * kPgCgTol * rz0);
                    for (int cg = 0; cg < B.max_cg && !conv; cg++) {
                        mat_vec(q, sh, lambda);
                        const double pAp = block_sum(dot_part(sh.p, sh.Ap, n6), sh, par);  // (thread t reads its own A p)
                        cgs++;
                        if (uniform(!(pAp > 0) || !isfinite(pAp))) {
                            not_pd = 1;
                            break;
                        }
                        const double alpha = rz / pAp;
                        for (int n = t; n < q.N; n += kBlock) {
                            double L[36], r[6], zz[6];
                            const bool free_node = !q.fixed[n];
#pragma unroll
                            for (int k = 0; k < 6; k++) {
                                sh.x[6 * n + k] += alpha * sh.p[6 * n + k];
                                r[k] = sh.r[6 * n + k] - alpha * sh.Ap[6 * n + k];
                                sh.r[6 * n + k] = r[k];
                            }
                            if (free_node) {
                                load_factor(q, n, L);
                                pg_chol6_solve(L, r, zz);
                            }
#pragma unroll
                            for (int k = 0; k < 6; k++) sh.z[6 * n + k] = free_node ? zz[k] : 0.0;
                        }
                        __syncthreads();
                        const double rzn = block_sum(dot_part(sh.r, sh.z, n6), sh, par);
                        const double beta = rzn / rz;
                        rz = rzn;
                        conv = uniform(rz <= kPgCgTol * kPgCgTol * rz0);
                        if (!conv) {
                            for (int k = t; k < n6; k += kBlock) sh.p[k] = sh.z[k] + beta * sh.p[k];
                            __syncthreads();
                        }
                    }
                }
                if (not_pd)
                    lambda *= kLmUp;
                else
                    solved = 1;
            }
            if (!solved) break;  // gave up
            // ---- the step rule over the whole state, the trial poses
            double part = t < n6 ? -0.0 : 0.0;
            for (int k = t; k < n6; k += kBlock) part += sh.x[k] * sh.x[k];
            const double dx2 = block_sum(part, sh, par);
            part = t < 3 * q.N ? -0.0 : 0.0;
            for (int k = t; k < 3 * q.N; k += kBlock) {
                const double v = q.cur[12 * (k / 3) + 9 + k % 3];
                part += v * v;
            }
            const double t2 = block_sum(part, sh, par);
            if (uniform(lm_step_is_small(dx2, t2))) break;
            for (int n = t; n < q.N; n += kBlock) {
                double xi[6], T[12], out[12];
#pragma unroll
                for (int k = 0; k < 12; k++) T[k] = q.cur[12 * (size_t)n + k];
                if (!q.fixed[n]) {
#pragma unroll
                    for (int k = 0; k < 6; k++) xi[k] = sh.x[6 * n + k];
                    se3_left_update(xi, T, out);
                }
#pragma unroll
                for (int k = 0; k < 12; k++) q.trial[12 * (size_t)n + k] = q.fixed[n] ? T[k] : out[k];
            }
            __syncthreads();
            const double c1 = linearize(B, q, q.trial, false, false, sh, par);
            const auto [accept, stop] = lm_verdict(c0, c1, lambda);
            if (uniform(accept)) {
                for (int k = t; k < n12; k += kBlock) q.cur[k] = q.trial[k];
                __syncthreads();
                c0 = linearize(B, q, q.cur, true, false, sh, par);  // (c1's bits: the same edges in the same order)
            }
            if (uniform(stop)) break;
        }
    }

    // ---- results
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double* out = B.poses_out + 12 * node_at;
    for (int k = t; k < n12; k += kBlock) out[k] = q.cur[k];  // (a problem not iterated on: the bits it came with)
    if (t == 64) {
        B.costs[2 * (size_t)p] = poisoned ? nan : c_first;
        B.costs[2 * (size_t)p + 1] = poisoned ? nan : c0;
        B.iterations[p] = its;
        B.cg_iterations[p] = cgs;
    }
}

}  // namespace

hipError_t launch_pose_graph(const PoseGraphBatch& b, hipStream_t st) {
    if (b.P < 0 || b.max_nodes < 0 || b.max_nodes > SVO_PG_MAX_NODES || b.max_edges < 0 ||
        b.max_edges > SVO_PG_MAX_EDGES || b.max_iterations < 0 || b.max_iterations > SVO_PG_MAX_ITERATIONS ||
        b.max_cg < 1 || b.max_cg > SVO_PG_MAX_CG)
        return hipErrorInvalidValue;
    if (b.P == 0) return hipSuccess;
    if (!b.poses_in || !b.poses_out || !b.fixed || !b.edge_ij || !b.edge_Z || !b.edge_info || !b.inc_start ||
        !b.inc_list || !b.cur || !b.trial || !b.terms || !b.node || !b.chol || !b.costs || !b.iterations ||
        !b.cg_iterations)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_graph_kernel, dim3(b.P), dim3(kBlock), 0, st, b);
    return hipGetLastError();
}

}  // namespace svo
