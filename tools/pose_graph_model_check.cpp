// Stand-alone host check of the pose-graph rule (svo_amd/csrc/pose_graph_model.hpp),
// meant for a sanitizer build on the build machine:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ \
//       -I<rocm>/include -Isvo_amd/csrc tools/pose_graph_model_check.cpp -o tools/bin/pose_graph_model_check
//   tools/bin/pose_graph_model_check < commands
// It evaluates what its standard input asks for and prints every double with %a
// (tests/test_pose_graph_cpu.py and test_pose_graph_gpu.py write the commands and
// compare). Numbers are read by strtod, so hex floats, nan and inf are input too.
//   edge DELTA TI[12] TJ[12] Z[12] INFO[21]
//       -> "e e[6] w cost", "Ji [36]", "Jj [36]"
//   rel TI[12] TJ[12]        -> "rel" + the 12 of T_j T_i^-1
//   graph DELTA MAXIT MAXCG N E   then N lines T[12] FIXED, then E lines I J Z[12] INFO[21]
//       -> per edge the three lines of `edge`, per node "node" + its 27 sums over its
//       incident edges in ascending edge index from -0, "cost" + the edges' costs
//       added in index order; with MAXIT > 0 then the Levenberg-Marquardt of
//       include/svo_gpu.h (svo_pose_graph_optimize) with every sum serial: per
//       iteration "it EVENT RETRIES c_cur c_trial CG" (EVENT a = accept, r = reject,
//       g = give up, s = small step), then "costs first final ITS CGS" and per node
//       "pose" + its 12.
// Exit status 0 only if every command parsed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pose_graph_model.hpp"

using namespace svo;

namespace {

bool number(double& v) {
    char tok[128];
    if (scanf("%127s", tok) != 1) return false;
    char* end;
    v = strtod(tok, &end);
    return end != tok && *end == 0;
}

bool numbers(double* v, int n) {
    for (int i = 0; i < n; i++)
        if (!number(v[i])) return false;
    return true;
}

void print(const char* tag, const double* v, int n) {
    printf("%s", tag);
    for (int i = 0; i < n; i++) printf(" %a", v[i]);
    printf("\n");
}

struct Graph {
    int N = 0, E = 0;
    double delta = 0;
    std::vector<double> T, Z, info;
    std::vector<int> fixed, ij;
    std::vector<std::vector<int>> inc;  // per node 2*edge + end, ascending
    std::vector<double> terms, node;    // E x kPgEdgeTerms, N x 27
};

// the cost; with `full` the edges' terms and the nodes' sums; with `show` the edges' lines
double linearize(Graph& g, const std::vector<double>& T, bool full, bool show) {
    double c = g.E ? -0.0 : 0.0;
    for (int k = 0; k < g.E; k++) {
        double e[6], Ji[36], Jj[36], w, cost;
        const double* info = &g.info[21 * (size_t)k];
        pg_edge_eval(&T[12 * (size_t)g.ij[2 * k]], &T[12 * (size_t)g.ij[2 * k + 1]], &g.Z[12 * (size_t)k], info, g.delta,
                     e, Ji, Jj, w, cost);
        c += cost;
        if (full) pg_edge_terms(info, w, e, Ji, Jj, &g.terms[(size_t)kPgEdgeTerms * k], 1);
        if (show) {
            const double o[8] = {e[0], e[1], e[2], e[3], e[4], e[5], w, cost};
            print("e", o, 8);
            print("Ji", Ji, 36);
            print("Jj", Jj, 36);
        }
    }
    if (full)
        for (int n = 0; n < g.N; n++)
            for (int k = 0; k < 27; k++) {
                double s = g.inc[n].empty() ? 0.0 : -0.0;
                for (int code : g.inc[n]) s += g.terms[(size_t)kPgEdgeTerms * (code >> 1) + 36 + 27 * (code & 1) + k];
                g.node[27 * (size_t)n + k] = s;
            }
    return c;
}

double dot(const std::vector<double>& a, const std::vector<double>& b) {
    double s = a.empty() ? 0.0 : -0.0;
    for (size_t k = 0; k < a.size(); k++) s += a[k] * b[k];
    return s;
}

double damped(const Graph& g, int n, int a, int b, double lambda) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const double h = g.node[27 * (size_t)n + 6 * lo - lo * (lo - 1) / 2 + (hi - lo)];
    return a == b ? h + lambda * (h > 0 ? h : 1e-12) : h;
}

// the damped system by PCG: false if not positive definite
bool solve(const Graph& g, double lambda, int max_cg, std::vector<double>& x, int& cgs) {
    const int n6 = 6 * g.N;
    std::vector<double> L(36 * (size_t)g.N), r(n6), z(n6), p(n6), Ap(n6);
    x.assign(n6, 0.0);
    for (int n = 0; n < g.N; n++) {
        if (g.fixed[n]) continue;
        if (!pg_chol6(&g.node[27 * (size_t)n], 1, lambda, &L[36 * (size_t)n])) return false;
        for (int k = 0; k < 6; k++) r[6 * n + k] = -g.node[27 * (size_t)n + 21 + k];
        pg_chol6_solve(&L[36 * (size_t)n], &r[6 * n], &z[6 * n]);
    }
    p = z;
    const double rz0 = dot(r, z);
    double rz = rz0;
    for (int it = 0; it < max_cg && !(rz <= kPgCgTol * kPgCgTol * rz0); it++) {
        for (int k = 0; k < n6; k++) {
            const int n = k / 6, c = k % 6;
            double acc = 0.0;
            if (!g.fixed[n]) {
                acc = damped(g, n, c, 0, lambda) * p[6 * n];
                for (int d = 1; d < 6; d++) acc += damped(g, n, c, d, lambda) * p[6 * n + d];
                for (int code : g.inc[n]) {
                    const int e = code >> 1, end = code & 1, m = g.ij[2 * e + (1 - end)];
                    const double* t = &g.terms[(size_t)kPgEdgeTerms * e];
                    const int first = end ? c : 6 * c, step = end ? 6 : 1;
                    double s = t[first] * p[6 * m];
                    for (int d = 1; d < 6; d++) s += t[first + step * d] * p[6 * m + d];
                    acc += s;
                }
            }
            Ap[k] = acc;
        }
        const double pAp = dot(p, Ap);
        cgs++;
        if (!(pAp > 0) || !std::isfinite(pAp)) return false;
        const double alpha = rz / pAp;
        for (int n = 0; n < g.N; n++) {
            for (int k = 6 * n; k < 6 * n + 6; k++) {
                x[k] += alpha * p[k];
                r[k] -= alpha * Ap[k];
            }
            if (!g.fixed[n]) pg_chol6_solve(&L[36 * (size_t)n], &r[6 * n], &z[6 * n]);
        }
        const double rzn = dot(r, z), beta = rzn / rz;
        rz = rzn;
        if (!(rz <= kPgCgTol * kPgCgTol * rz0))
            for (int k = 0; k < n6; k++) p[k] = z[k] + beta * p[k];
    }
    return true;
}

bool graph(double delta, int max_it, int max_cg, int N, int E) {
    if (N < 0 || E < 0 || N > 4096 || E > 16384 || max_cg < 1) return false;
    Graph g;
    g.N = N, g.E = E, g.delta = delta;
    g.T.resize(12 * (size_t)N), g.fixed.resize(N), g.inc.resize(N);
    g.Z.resize(12 * (size_t)E), g.info.resize(21 * (size_t)E), g.ij.resize(2 * (size_t)E);
    g.terms.resize((size_t)kPgEdgeTerms * E), g.node.resize(27 * (size_t)N);
    for (int n = 0; n < N; n++) {
        double f;
        if (!numbers(&g.T[12 * (size_t)n], 12) || !number(f)) return false;
        g.fixed[n] = f != 0;
    }
    for (int k = 0; k < E; k++) {
        double ij[2];
        if (!numbers(ij, 2) || !numbers(&g.Z[12 * (size_t)k], 12) || !numbers(&g.info[21 * (size_t)k], 21)) return false;
        const int i = (int)ij[0], j = (int)ij[1];
        if (i < 0 || i >= N || j < 0 || j >= N || i == j) return false;
        g.ij[2 * k] = i, g.ij[2 * k + 1] = j;
        g.inc[i].push_back(2 * k);
        g.inc[j].push_back(2 * k + 1);
    }
    std::vector<double> cur = g.T, trial(g.T.size()), x;
    const double c_first = linearize(g, cur, true, true);
    for (int n = 0; n < N; n++) print("node", &g.node[27 * (size_t)n], 27);
    print("cost", &c_first, 1);
    if (max_it <= 0) return true;
    double c0 = c_first, lambda = kLmLambda0;
    int its = 0, cgs = 0;
    for (int it = 0; it < max_it; it++) {
        its = it + 1;
        bool ok = false;
        int retries = 0;
        const int cg0 = cgs;
        while (lambda < kLmCeiling) {
            if ((ok = solve(g, lambda, max_cg, x, cgs))) break;
            lambda *= kLmUp;
            retries++;
        }
        if (!ok) {
            printf("it g %d %a nan %d\n", retries, c0, cgs - cg0);
            break;
        }
        double dx2 = x.empty() ? 0.0 : -0.0, t2 = N ? -0.0 : 0.0;
        for (double v : x) dx2 += v * v;
        for (int k = 0; k < 3 * N; k++) t2 += cur[12 * (k / 3) + 9 + k % 3] * cur[12 * (k / 3) + 9 + k % 3];
        if (lm_step_is_small(dx2, t2)) {
            printf("it s %d %a nan %d\n", retries, c0, cgs - cg0);
            break;
        }
        for (int n = 0; n < N; n++) {
            if (g.fixed[n])
                memcpy(&trial[12 * (size_t)n], &cur[12 * (size_t)n], 12 * sizeof(double));
            else
                se3_left_update(&x[6 * n], &cur[12 * (size_t)n], &trial[12 * (size_t)n]);
        }
        const double c1 = linearize(g, trial, false, false);
        const LmVerdict v = lm_verdict(c0, c1, lambda);
        printf("it %s %d %a %a %d\n", v.accept ? "a" : "r", retries, c0, c1, cgs - cg0);
        if (v.accept) {
            cur = trial;
            c0 = linearize(g, cur, true, false);
        }
        if (v.stop) break;
    }
    printf("costs %a %a %d %d\n", c_first, c0, its, cgs);
    for (int n = 0; n < N; n++) print("pose", &cur[12 * (size_t)n], 12);
    return true;
}

}  // namespace

int main() {
    char cmd[32];
    bool ok = true;
    while (ok && scanf("%31s", cmd) == 1) {
        double a[64];
        if (!strcmp(cmd, "edge")) {
            if ((ok = numbers(a, 58))) {
                double o[8], Ji[36], Jj[36];
                pg_edge_eval(a + 1, a + 13, a + 25, a + 37, a[0], o, Ji, Jj, o[6], o[7]);
                print("e", o, 8);
                print("Ji", Ji, 36);
                print("Jj", Jj, 36);
            }
        } else if (!strcmp(cmd, "rel")) {
            if ((ok = numbers(a, 24))) {
                double Z[12];
                pg_relative(a, a + 12, Z);
                print("rel", Z, 12);
            }
        } else if (!strcmp(cmd, "graph")) {
            ok = numbers(a, 5) && graph(a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4]);
        } else {
            ok = false;
        }
    }
    if (!ok) {
        fprintf(stderr, "pose_graph_model_check: bad input\n");
        return 1;
    }
    printf("pose_graph_model_check: ok\n");
    return 0;
}
