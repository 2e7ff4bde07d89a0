// Pyramidal Lucas-Kanade sparse optical flow for gfx950: all pyramid levels in one
// launch. This file is the host entry (launch_lk, lk_supported, lk_apply_env); the
// kernels, one family per file, each with its launch wrapper:
//   lk_multi.hip    lk_multi_kernel  four features per wave: the two product calls
//   lk_cvq.hip      lk_cvq_kernel    the same lane map, OpenCV's float summation order
//   lk_fast.hip     lk_fast_kernel   one feature per wave, compile-time windows
//   lk_generic.hip  lk_kernel        one feature per wave, any window
//   lk_cv.hip       lk_cv_kernel     lk_kernel's map, OpenCV's float summation order
// with lk_device.hpp (what more than one of them uses: OpenCV's rules, each stated
// once), lk_quad.hpp (the first two) and lk_strip.hpp (the last two).
//
// Replaces cv::calcOpticalFlowPyrLK at R:src/tracking.cpp:160-165 (temporal,
// 21x21, maxLevel 3, {COUNT+EPS, 50, 1e-3}, OPTFLOW_LK_GET_MIN_EIGENVALS) and
// :101-105 (stereo, 11x11, maxLevel 3, {COUNT+EPS, 30, 1e-3}, flags 0).
// Semantics follow OpenCV 4.x lkpyramid.cpp LKTrackerInvoker: identical
// fixed-point sampling (W_BITS 14, I stored x32, CV_DESCALE), identical float
// solve, exit and oscillation rules, identical status/err rules.
//
// MI355X design:
//  * A feature's levels are independent of every other feature, so the whole
//    coarse-to-fine pass is one launch: no grid sync between levels.
//  * The Scharr derivatives of the previous image come from its derivative
//    pyramid (scharr.hip / pyr_scharr_kernel: packed Ix | Iy << 16 per pixel,
//    stored x4, zero-padded borders as OpenCV's derivative levels), built once
//    per frame and reused by every LK call on it (OpenCV recomputes it per
//    call); the prev / next u8 pyramid levels are stored with 32-px REFLECT_101
//    borders (kPyrPad), so window reads near the image edge are branch-free.
#include "lk_device.hpp"

#include <cstdlib>

namespace svo {

void lk_apply_env(LKParams& p) {
    const char* gen = std::getenv("SVO_LK_GENERIC");
    p.generic = gen && gen[0] == '1' ? 1 : 0;
    const char* quad = std::getenv("SVO_LK_QUAD");
    p.quad = quad && quad[0] == '0' ? 0 : 1;
}

bool lk_supported(int win_w, int win_h) {
    if (win_w < 3 || win_h < 3 || win_w + 2 * JM > 64 || win_w + 3 > 64) return false;
    // a lane's strip: up to 64 rows (windows wider than 32 px have one strip per
    // column), its int32 partial sums bounded by 64 * 8160 * 4080 < 2^31; at most
    // 2048 px, the bound of the float SAD sum (2048 * 8160 < 2^24)
    int groups = 64 / win_w;
    int rpg = (win_h + groups - 1) / groups;
    return rpg <= 64 && win_w * win_h <= 2048;
}

hipError_t launch_lk(const LKBatch& b, int nseq, int max_n, const LKParams& lp, hipStream_t st) {
    if (max_n <= 0 || nseq <= 0) return hipSuccess;
    const auto square = [&](int n) { return lp.win_w == n && lp.win_h == n; };
    // four features per wave: the reference's two windows; the SAD error (flags 0 +
    // want_err) stays on the one-feature-per-wave kernels
    const bool quad = !lp.generic && lp.quad && !(lp.want_err && !(lp.flags & SVO_LK_GET_MIN_EIGENVALS));
    if (lp.cv_order) {
        // OpenCV's float summation order
        if (quad && (square(21) || square(11))) return launch_lk_cvq(b, nseq, max_n, lp, st);
        return launch_lk_cv(b, nseq, max_n, lp, st);
    }
    if (!lp.generic) {
        if (quad && square(21)) return launch_lk_multi_temporal(b, nseq, max_n, lp, st);
        // the stereo call's 11 x 11 (findLeftFeaturesInRight, no err)
        if (quad && square(11)) return launch_lk_multi_stereo(b, nseq, max_n, lp, st);
        if (square(21) || square(11) || square(15) || square(31)) return launch_lk_fast(b, nseq, max_n, lp, st);
    }
    return launch_lk_generic(b, nseq, max_n, lp, st);
}

}  // namespace svo
