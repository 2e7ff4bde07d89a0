// ORB detection shared by svo_orb_detect (one frame) and the batched front end
// (one frame per sequence, SVO_FE use_orb): level geometry, the host's
// per-level selection (computeKeyPoints' runByImageBorder + retainBest), and the
// batched device pipeline (orb_detect.cpp, orb.hip).
#pragma once

#include <functional>
#include <vector>

#include "common.hpp"

namespace svo {

struct OrbGeometry {
    int nlev = 0;
    int lw[kMaxLevels], lh[kMaxLevels], pitch[kMaxLevels], kcap[kMaxLevels], nf[kMaxLevels];
    float lscale[kMaxLevels];
    int maxcap = 0, maxh = 0, maxnseg = 0;
    // INTER_LINEAR_EXACT tables of levels 1.. (x offsets, x coefficients, y offsets,
    // y coefficients, each level at tab_at[l])
    std::vector<uint32_t> tabs;
    size_t tab_at[kMaxLevels] = {0};
};

// false: parameters outside what the detector supports (err names the reason)
bool orb_geometry(int W, int H, const svo_orb_params& p, OrbGeometry& g, const char** err);

// computeKeyPoints' selection from the per-level FAST keypoints kps[l][0..n[l])
// (level coordinates) and, with HARRIS, their responses resp[l]: runByImageBorder,
// retainBest(2 n_l) by FAST response, retainBest(n_l) by Harris response, level
// order, pt *= s_l. Writes min(total, cap) keypoints; returns the total.
int orb_select(const OrbGeometry& g, const svo_orb_params& p, const svo_keypoint* const* kps,
               const float* const* resp, const int* n, svo_keypoint* out, int* octave, int cap);

// ORB detection of one frame per sequence for the batched front end. The level
// images, masks, FAST scratch and keypoints of all sequences live in one
// allocation; detect() runs the device stages batched over the sequences (scale
// pyramid + mask pyramid, FAST per level, Harris) and the host selection per
// sequence (par(S, fn): fn(s) for every s, possibly in parallel), then writes the
// selected keypoints (level-0 coordinates) to out[s * cap_out ..] and their counts
// to nout[s] on the device. Synchronous on the host.
struct OrbBatch;
OrbBatch* orb_batch_create(int S, int W, int H, const svo_orb_params& p);
void orb_batch_destroy(OrbBatch* ob);
// lv0[s]: level 0 (the frame) of sequence s. Mask: boxes of +-half around
// box_counts[s] points of box_pts + 2 s box_stride (device), or none when box_pts
// is null. overflow[s] (host, nullable): keypoints beyond cap_out.
hipError_t orb_batch_detect(OrbBatch* ob, const ImgLevel* lv0, const float* box_pts, const int* box_counts,
                            int box_stride, int box_max, float half, svo_keypoint* out, int* nout, int cap_out,
                            hipStream_t st, const std::function<void(int, const std::function<void(int)>&)>& par,
                            int* overflow);

// svo_orb_detect's workspace (scratch slot kScratchOrb) and the scale and mask pyramids built in it
struct OrbLevels {
    OrbGeometry g;
    size_t mask_off[kMaxLevels];
    PyrDesc lev;             // the levels (level 0 = the caller's image)
    uint8_t* dmask;          // level masks at mask_off[l] (rows of lw[l]); null without a mask
    PyrDesc* ddesc;          // device: [l].lv[0] = level l
    unsigned long long* bits;
    int *rowcnt, *rowoff;
    svo_keypoint* dkp;       // [nlev][maxcap]
    int* dn;
    float* dresp;            // [nlev][maxcap]
};
// The two halves of svo_orb_detect (orb_detect.cpp), shared with svo_orb_level
// and the descriptor entry points (orb_describe.cpp): the pyramids queued on the
// context's stream, then detection and selection on them (synchronous).
int orb_build_levels(svo_ctx* ctx, const svo_image* img, const svo_orb_params* prm, const uint8_t* mask,
                     const char* who, OrbLevels& o);
int orb_detect_levels(svo_ctx* ctx, const svo_orb_params* prm, OrbLevels& o, svo_keypoint* out, int* octave, int cap,
                      int* n_out);

// ORB descriptors (orb_describe.hip; the rules: DESIGN.md section 3d).
constexpr int kOrbPatternPoints = 512;
// One keypoint as the kernels take it: the level pixel, or level < 0 for a
// keypoint too close to its level's border (zero descriptor, angle -1).
struct OrbDescKp {
    int cx, cy, level, pad;
};
struct OrbDirection {  // c = m10 / hyp, s = m01 / hyp (1, 0 without a gradient)
    double c, s;
};
// The host tables of a descriptor pass (orb_describe.cpp): the pattern to use (the
// caller's, checked, or the default one for a null pattern_xy) into pat[1024], the
// hp + 1 half row widths into umax[16], the validity border into *reach. Returns
// null, or the reason patch_size / pattern_xy are refused.
const char* orb_describe_tables(int patch_size, const int8_t* pattern_xy, int8_t* pat, int* umax, int* reach);
// every level of `levels` blurred into the level of the same size of `blurred`
hipError_t launch_orb_blur(const PyrDesc& levels, const PyrDesc& blurred, hipStream_t st);
// hp: half patch; umax: hp + 1 ints on the device
hipError_t launch_orb_angle(const PyrDesc& levels, const OrbDescKp* kp, int n, int hp, const int* umax,
                            OrbDirection* dir, float* angle, hipStream_t st);
// blurred: the levels of launch_orb_blur as a PyrDesc; pattern: 512 (x, y) int8 on
// the device; reach: the clamp of a steered offset (never binding, see the kernel)
hipError_t launch_orb_brief(const PyrDesc& blurred, const OrbDescKp* kp, int n, const int8_t* pattern,
                            const OrbDirection* dir, int reach, uint8_t* desc, hipStream_t st);
// Hamming 2-NN (match.hip): problem p (blockIdx.y) matches queries q + p*q_stride*32
// (nq[p] of them) against train t + p*t_stride*32 (nt[p]); idx / dist [p][q_stride][2].
// q_set / t_set (device, [p], nullable): problem p matches query set q_set[p]
// against train set t_set[p] instead -- descriptors at set * stride * 32, counts
// nq[set] / nt[set] -- and still writes rows p of idx / dist: problems that share
// a set do not replicate it (the place memory's query, frontend_places.cpp)
hipError_t launch_hamming_knn2(const uint32_t* q, const uint32_t* t, const int* nq, const int* nt, int q_stride,
                               int t_stride, int n_problems, int max_nq, int* idx, int* dist, hipStream_t st,
                               const int* q_set = nullptr, const int* t_set = nullptr);
// svo_match_filter per problem (match_filter.hip): the ratio test and the
// cross-check on launch_hamming_knn2's rows, then a stable compaction: the kept
// (q, t) pairs in ascending q into pairs [p][q_stride][2], their count into
// n_pairs[p]. idx_tq (rows [p][t_stride][2]) null: no cross-check. q_set / t_set as
// above name the sets whose counts nq / nt bound problem p. An index outside
// [0, nt) never passes (svo_match_filter_batch rejects it beforehand).
hipError_t launch_match_filter(const int* idx_qt, const int* dist_qt, const int* idx_tq, const int* nq,
                               const int* nt, int q_stride, int t_stride, int n_problems, int ratio_pct, int* pairs,
                               int* n_pairs, hipStream_t st, const int* q_set = nullptr,
                               const int* t_set = nullptr);

hipError_t launch_orb_resize(const uint8_t* src, int spitch, const uint8_t* smask, int sw, uint8_t* dst, int dpitch,
                             uint8_t* dmask, int dw, int dh, const int* xofs, const uint32_t* xc, const int* yofs,
                             const uint32_t* yc, hipStream_t st);
// every sequence's level: src[s].lv[0] -> dst[s].lv[0] (all of size dw x dh), masks
// smask + s * smask_stride (width sw) -> dmask + s * dmask_stride (nullable)
hipError_t launch_orb_resize_batched(const PyrDesc* src, const PyrDesc* dst, const uint8_t* smask,
                                     size_t smask_stride, int sw, uint8_t* dmask, size_t dmask_stride, int dw, int dh,
                                     int nseq, const int* xofs, const uint32_t* xc, const int* yofs,
                                     const uint32_t* yc, hipStream_t st);
hipError_t launch_orb_harris(const PyrDesc& levels, int nlevels, const svo_keypoint* kps, const int* n, int cap,
                             int max_n, float* resp, hipStream_t st);
// levels[l * nseq + s].lv[0]: level l of sequence s; kps / resp [l][s][cap], n [l][s]
hipError_t launch_orb_harris_batched(const PyrDesc* levels, int nlevels, int nseq, const svo_keypoint* kps,
                                     const int* n, int cap, int max_n, float* resp, hipStream_t st);

}  // namespace svo
