// Stand-alone host check of the reprojection model and the LM rules
// (svo_amd/csrc/reproj_model.hpp), meant for a sanitizer build on the build machine:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -Isvo_amd/csrc \
//       tools/reproj_model_check.cpp -o tools/bin/reproj_model_check
//   tools/bin/reproj_model_check < commands
// It evaluates what its standard input asks for and prints every double with %a
// (tests/test_reproj_model_cpu.py writes the commands and compares). Numbers are
// read by strtod, so hex floats, nan and inf are input too. One command per line:
//   lin S DELTA BASELINE N   then 12 numbers of T, then N lines X Y Z U V UR
//       S = 1: the stereo instantiation, 0: the monocular one (UR ignored). Prints
//       "obs KIND r0 r1 r2 w cost J[18]" per observation (what obs_eval did not
//       write prints as 0) and "sums" + the 28 sums added in index order from +0.
//   upd XI[6] T[12]          -> "upd" + the 12 of exp(xi^) T, computed apart and in place
//   solve LAMBDA NE[28]      -> "solve OK x[6]"
//   verdict C0 C1 LAMBDA     -> "verdict ACCEPT STOP lambda"
//   small DX2 T2             -> "small 0|1"
// Exit status 0 only if every command parsed and the in-place update kept the bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "reproj_model.hpp"

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

template <bool kStereo>
bool lin(double delta, double baseline, int n) {
    double T[12], e[kNE] = {0};
    if (!numbers(T, 12)) return false;
    const Cam cam{718.856, 718.856, 607.1928, 185.2157, delta, baseline};
    for (int i = 0; i < n; i++) {
        double in[6];
        if (!numbers(in, 6)) return false;
        const float u[2] = {(float)in[3], (float)in[4]}, ur = (float)in[5];
        // r[0..2], w, cost, J: exactly as large as the instantiation's rows
        std::vector<double> J(6 * kRows<kStereo>, 0.0);
        double o[5] = {0, 0, 0, 0, 0};
        const int kind = obs_eval<kStereo>(cam, T, in, u, kStereo ? &ur : nullptr, o[0], o[1], o[2], o[3], o[4], J.data());
        if (kind) {
            normal_terms<kStereo, true>(kind == 2, o[3], o[0], o[1], o[2], J.data(), e);
            e[27] += o[4];
        }
        printf("obs %d", kind);
        print("", o, 5);
        J.resize(18, 0.0);
        print("J", J.data(), 18);
    }
    print("sums", e, kNE);
    return true;
}

}  // namespace

int main() {
    char cmd[32];
    bool ok = true;
    while (ok && scanf("%31s", cmd) == 1) {
        double a[40];
        if (!strcmp(cmd, "lin")) {
            ok = numbers(a, 4) && (a[0] != 0 ? lin<true>(a[1], a[2], (int)a[3]) : lin<false>(a[1], a[2], (int)a[3]));
        } else if (!strcmp(cmd, "upd")) {
            if ((ok = numbers(a, 18))) {
                double out[12], T[12];
                memcpy(T, a + 6, sizeof(T));
                se3_left_update(a, T, out);
                se3_left_update(a, T, T);
                ok = !memcmp(T, out, sizeof(T));
                print("upd", out, 12);
            }
        } else if (!strcmp(cmd, "solve")) {
            if ((ok = numbers(a, 29))) {
                double x[6] = {0, 0, 0, 0, 0, 0};
                const bool pd = lm_solve6(a + 1, a[0], x);
                printf("solve %d", (int)pd);
                print("", x, 6);
            }
        } else if (!strcmp(cmd, "verdict")) {
            if ((ok = numbers(a, 3))) {
                const LmVerdict v = lm_verdict(a[0], a[1], a[2]);
                printf("verdict %d %d %a\n", (int)v.accept, (int)v.stop, a[2]);
            }
        } else if (!strcmp(cmd, "small")) {
            if ((ok = numbers(a, 2))) printf("small %d\n", (int)lm_step_is_small(a[0], a[1]));
        } else {
            ok = false;
        }
    }
    if (!ok) {
        fprintf(stderr, "reproj_model_check: bad input\n");
        return 1;
    }
    printf("reproj_model_check: ok\n");
    return 0;
}
