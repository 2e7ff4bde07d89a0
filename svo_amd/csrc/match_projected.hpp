// Matching map points to a frame by projection (svo_match_projected; the rules:
// DESIGN.md section 3f): the keypoints of every problem binned into a uniform
// cell grid, every point projected and compared with the keypoints of the cells
// its window touches, and the points' bids for keypoints resolved into pairs
// (match_projected.hip). No HIP include in the layout part: tools/layout_check.cpp
// builds it with the host compiler.
#pragma once

#include <cstddef>
#include <cstdint>

#include "layout.hpp"
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "svo_gpu.h"
#endif

namespace svo {

constexpr int kProjMaxCells = 4096;     // cells of one problem's grid (their counts are scanned in LDS)
constexpr int kProjMaxStride = 1 << 20;  // a key is (distance << 20) | index
constexpr uint32_t kProjNoKey = 0xffffffffu;

// The cell grid of a w x h frame: square cells of 2^shift pixels, the smallest
// power of two >= 8 that leaves at most kProjMaxCells cells; gw x gh of them.
struct ProjGrid {
    int shift, gw, gh;
    constexpr int cells() const { return gw * gh; }
};
inline ProjGrid proj_grid(int w, int h) {
    ProjGrid g{3, 0, 0};
    for (;; g.shift++) {
        g.gw = (int)((((long long)w - 1) >> g.shift) + 1);
        g.gh = (int)((((long long)h - 1) >> g.shift) + 1);
        if ((long long)g.gw * g.gh <= kProjMaxCells) return g;
    }
}

// The search's scratch for n_problems problems of k_stride keypoint rows each:
// per problem the cells' first entries (cells + 1 ints, an exclusive scan of the
// cell counts), the usable keypoints' indices sorted by cell, and one claim word
// per keypoint: the smallest key (distance << 20 | point) that bid for it.
struct ProjScratch {
    int* cell_start = nullptr;   // [p][cells + 1]
    int* sorted = nullptr;       // [p][k_stride]
    uint32_t* claim = nullptr;   // [p][k_stride]
};
template <class C>  // (a Carver, or layout_check.cpp's probe)
void proj_scratch_layout(C& c, ProjScratch& s, size_t n_problems, size_t k_stride, const ProjGrid& g) {
    s.cell_start = c.template take<int>(n_problems * ((size_t)g.cells() + 1));
    s.sorted = c.template take<int>(n_problems * k_stride);
    s.claim = c.template take<uint32_t>(n_problems * k_stride);
}

#ifdef __HIPCC__
// null, or the reason svo_match_projected refuses the frame size or the parameters
const char* proj_params_refused(int w, int h, const svo_proj_match_params* prm);

// One call's arrays, all on the device. Problem p reads the points of set
// p_set[p] (xyz / pdesc at set * p_stride, n_pts[set] of them) and the keypoints
// of set k_set[p] (kxy / kdesc at set * k_stride, n_kp[set]); a null map: set p.
// Its pose is poses + 12 p; its outputs are rows p: idx / dist / proj
// [p][p_stride][2] (each nullable), pairs [p][k_stride][2] with n_pairs [p]
// (nullable together).
struct ProjMatch {
    const int* n_pts;
    const int* n_kp;
    int p_stride, k_stride;
    const double* xyz;
    const uint32_t* pdesc;
    const float* kxy;
    const uint32_t* kdesc;
    const double* poses;
    const int* p_set;  // nullable
    const int* k_set;  // nullable
    double fx, fy, cx, cy;
    int w, h;
    float radius;
    int max_dist, ratio_pct;
    ProjGrid grid;
    ProjScratch scr;
    int lanes;  // lanes per point of proj_match_kernel: 16, or anything else for 1 (the default)
    int* idx;
    int* dist;
    float* proj;
    int* pairs;
    int* n_pairs;
};
// proj_bin_kernel: the grid, the sorted list and the cleared claim words of every problem
hipError_t launch_proj_bin(const ProjMatch& m, int n_problems, hipStream_t st);
// proj_match_kernel: idx / dist / proj and the bids; max_pts bounds the grid
// (blocks past a problem's count return at once). m.lanes picks the launch shape;
// the results do not depend on it.
hipError_t launch_proj_match(const ProjMatch& m, int n_problems, int max_pts, hipStream_t st);
// proj_pairs_kernel: the claimed keypoints in ascending index (m.pairs non-null)
hipError_t launch_proj_pairs(const ProjMatch& m, int n_problems, hipStream_t st);
#endif

}  // namespace svo
