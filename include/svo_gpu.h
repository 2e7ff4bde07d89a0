/*
 * svo_gpu.h -- C ABI of the MI355X-native ikryukov/svo front end (libsvo_gpu.so).
 *
 * This is the drop-in boundary for the four OpenCV calls the reference's
 * Tracking makes on its hot path:
 *
 *   reference call (R: = ikryukov/svo)                         replaced by
 *   ---------------------------------------------------------  ------------------------------
 *   buildOpticalFlowPyramid inside calcOpticalFlowPyrLK          svo_image_upload /
 *     R:src/tracking.cpp:101, :160                               svo_image_build_pyramid
 *   mDetector->detect(img, kps, mask)  (FastFeatureDetector)     svo_fast_detect
 *     R:src/tracking.cpp:82 (created :54-57)
 *   cv::rectangle(mask, p-(10,10), p+(10,10), 0, FILLED)         svo_mask_boxes
 *     R:src/tracking.cpp:76-79
 *   FeatureSet::bucketingFeatures  R:src/bucket.cpp:24-68        svo_bucket_features
 *   cv::calcOpticalFlowPyrLK(...)  R:src/tracking.cpp:101-105,   svo_calc_optical_flow_pyr_lk
 *     :160-165
 *   PnPRansacCallback::computeError + findInliers (inside        svo_pnp_residuals
 *     cv::solvePnPRansac, R:src/tracking.cpp:191-196)
 *   cv::solvePnPRansac(..., SOLVEPNP_SQPNP)                      svo_solve_pnp_ransac
 *     R:src/tracking.cpp:191-196
 *   cv::solvePnP(..., SOLVEPNP_SQPNP)  (solvePnPRansac's final   svo_solve_pnp_sqpnp
 *     fit on the inliers, R:src/tracking.cpp:191-196)
 *   cv::triangulatePoints + convertPointsFromHomogeneous          svo_triangulate_points
 *     R:src/tracking.cpp:125-131
 *   (not in the reference, which is fed rectified pairs:)
 *   cv::initUndistortRectifyMap(..., CV_16SC2, ...)              svo_init_undistort_rectify_map
 *   cv::remap(..., INTER_LINEAR, BORDER_CONSTANT, 0)             svo_remap / svo_image_upload_raw /
 *                                                                svo_frontend_set_rectification
 *   (not in the reference: a row search for findLeftFeaturesInRight, R:src/tracking.cpp:94-152,
 *   on rectified pairs)                                          svo_stereo_match_rows /
 *                                                                svo_frontend_set_stereo_matcher
 *   (not in the reference: the same search around the feature's
 *   disparity one frame ago, a right column for every tracked
 *   feature of every frame of the window)                        svo_stereo_match_rows_guided /
 *                                                                svo_stereo_row_priors /
 *                                                                svo_frontend_set_stereo_tracking
 *
 * Conventions (no exceptions cross this ABI; no torch types):
 *   - Host memory is caller-owned. Device memory is owned by the context.
 *   - Every int-returning entry point returns SVO_OK (0) or a negative error
 *     class; svo_last_error(ctx) holds the message. Where OpenCV would throw a
 *     cv::Exception from CV_Assert (bad window, maxLevel < 0, < 4 PnP points),
 *     the call returns SVO_ERR_ARG and writes nothing.
 *   - One svo_ctx per (device, HIP stream, camera sequence). A context is not
 *     thread-safe; distinct contexts may be used concurrently from different
 *     threads and devices.
 *   - Points are float (x, y) pairs laid out exactly like std::vector<cv::Point2f>.
 */
#ifndef SVO_GPU_H
#define SVO_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_OK 0
#define SVO_ERR_ARG (-1)      /* argument outside the OpenCV contract */
#define SVO_ERR_HIP (-2)      /* HIP runtime error */
#define SVO_ERR_CAPACITY (-3) /* a fixed capacity was exceeded */
#define SVO_ERR_NODEVICE (-4) /* no HIP device / extension not usable */

/* cv::TermCriteria type bits and cv::calcOpticalFlowPyrLK flags */
#define SVO_TERM_COUNT 1
#define SVO_TERM_EPS 2
#define SVO_LK_USE_INITIAL_FLOW 4
#define SVO_LK_GET_MIN_EIGENVALS 8
/* Not an OpenCV flag: sum LK's normal equations in OpenCV's own float order
 * (LKTrackerInvoker's SSE build: four float lanes + a scalar tail, then its
 * lane reduction) instead of exactly. With it the results are those of
 * cv::calcOpticalFlowPyrLK's x86 build bit for bit; without it the sums are
 * exact integers rounded once (order-independent). */
#define SVO_LK_OPENCV_ORDER 0x10000

typedef struct svo_ctx svo_ctx;
typedef struct svo_image svo_image; /* a device-resident 8U image + its pyramid */

typedef struct svo_keypoint {
    float x, y;     /* cv::KeyPoint::pt */
    float response; /* cv::KeyPoint::response (FAST score with NMS, else 0) */
} svo_keypoint;

/* ------------------------------------------------------------ context */
int svo_ctx_create(int device, svo_ctx** out);
void svo_ctx_destroy(svo_ctx* ctx);
const char* svo_last_error(const svo_ctx* ctx);
int svo_ctx_synchronize(svo_ctx* ctx);
/* Build identification, e.g. "svo_gpu gfx950 hip 7.2". */
const char* svo_version(void);

/* ------------------------------------------------------------ images / pyramids
 * An svo_image holds a W x H 8U image and up to `max_levels` pyrDown levels in
 * one device allocation (level l is ((w_{l-1}+1)/2, (h_{l-1}+1)/2), OpenCV
 * pyrDown, BORDER_REFLECT_101). The number of levels a given LK call uses is
 * clamped exactly as buildOpticalFlowPyramid clamps it for that call's window. */
int svo_image_create(svo_ctx* ctx, int w, int h, int max_levels, svo_image** out);
void svo_image_destroy(svo_ctx* ctx, svo_image* img);
/* H2D copy of level 0 (row stride in bytes) and pyramid build. */
int svo_image_upload(svo_ctx* ctx, svo_image* img, const uint8_t* gray, int stride);
/* Colour ingest (R:include/async_image_loader.h:63-69, imread + cvtColor(
 * COLOR_BGR2GRAY)): H2D of a host 8UC3 BGR image (row stride in bytes >= 3w)
 * through a pinned double buffer, grey conversion written straight into level
 * 0 (OpenCV's fixed-point weights, bit-exact), then the pyramid build. Returns
 * once the copy is queued: `bgr` may be reused immediately. */
int svo_image_upload_bgr(svo_ctx* ctx, svo_image* img, const uint8_t* bgr, int stride);
/* Rectification of raw camera frames on the device. The reference never
 * rectifies (KITTI odometry ships rectified pairs); a rig of real lenses needs
 * cv::initUndistortRectifyMap + cv::remap on both eyes of every frame first.
 *
 * svo_rect_maps: one camera's map pair, device-resident -- exactly the two arrays
 * cv::initUndistortRectifyMap(..., CV_16SC2, map1, map2) or cv::convertMaps
 * produce (any camera model: fisheye or thin-prism users hand in OpenCV's own
 * maps): map1 int16 [h][w][2] = (sx, sy), map2 uint16 [h][w] < 1024 holding the
 * fractions a = map2 & 31 (x) and b = map2 >> 5 (y) in 1/32 pixel. raw_w x raw_h:
 * the camera's frame, w x h: the rectified image. SVO_ERR_ARG (nothing written):
 * null arguments, raw_w or raw_h < 2, w or h < 1, a map2 value >= 1024. */
typedef struct svo_rect_maps svo_rect_maps;
int svo_rect_maps_create(svo_ctx* ctx, int raw_w, int raw_h, int w, int h, const int16_t* map1,
                         const uint16_t* map2, svo_rect_maps** out);
void svo_rect_maps_destroy(svo_ctx* ctx, svo_rect_maps* maps);
/* cv::initUndistortRectifyMap(K, dist, R, newK, Size(w, h), CV_16SC2, map1, map2)
 * for the rational model dist = (k1, k2, p1, p2, k3, k4, k5, k6), on the host (no
 * context; once per rig): f64 in the order of OpenCV's scalar loop (iR = (newK
 * R)^-1 by cofactors, running sums along a row), coordinates rounded half to
 * even at 1/32 pixel. One deviation: the int16 cast of map1 saturates where
 * OpenCV's truncates, so a coordinate far outside stays outside. SVO_ERR_ARG
 * (nothing written): null arguments, w or h < 1, det(newK R) zero or not finite. */
int svo_init_undistort_rectify_map(const double K[9], const double dist[8], const double R[9], const double newK[9],
                                   int w, int h, int16_t* map1, uint16_t* map2);
/* cv::remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) of an 8U
 * raw_w x raw_h host image into a w x h host image (rows stride / dst_stride bytes
 * apart), through the kernel the entry points below use: with tap(i, j) = src[sy +
 * i][sx + j] inside the image and 0 outside,
 *   dst = ((32-a)(32-b) tap(0,0) + a(32-b) tap(0,1) + (32-a)b tap(1,0) + ab tap(1,1) + 512) >> 10,
 * OpenCV's fixed-point arithmetic restated without its weight table (DESIGN.md
 * section 3b). bgr != 0: src is 8UC3 and every tap its grey value first, i.e.
 * cv::cvtColor(BGR2GRAY) then cv::remap. Synchronous. */
int svo_remap(svo_ctx* ctx, const uint8_t* src, int stride, int bgr, const svo_rect_maps* maps, uint8_t* dst,
              int dst_stride);
/* svo_image_upload / svo_image_upload_bgr from a raw frame: H2D of the raw_w x
 * raw_h frame, svo_remap's rule written straight into level 0, then the pyramid
 * build. Returns once the frame has left `raw` (kernel and pyramid still queued).
 * SVO_ERR_ARG: the image is not the maps' w x h, stride below a raw row. */
int svo_image_upload_raw(svo_ctx* ctx, svo_image* img, const uint8_t* raw, int stride, int bgr,
                         const svo_rect_maps* maps);
/* Rebuild levels 1..max_levels from the device-resident level 0. */
int svo_image_build_pyramid(svo_ctx* ctx, svo_image* img);
int svo_image_level_size(const svo_image* img, int level, int* w, int* h);
int svo_image_download_level(svo_ctx* ctx, const svo_image* img, int level, uint8_t* dst, int stride);
/* The Scharr derivatives of pyramid level `level` (built pyramid required) as the
 * LK kernels read them: calcSharrDeriv (inside calcOpticalFlowPyrLK,
 * R:src/tracking.cpp:101, :160) scaled by 4, int16 ix / iy of that level's w x h
 * with `stride` elements per row; either output may be null. */
int svo_image_scharr_level(svo_ctx* ctx, const svo_image* img, int level, int16_t* ix, int16_t* iy, int stride);

/* ------------------------------------------------------------ FAST
 * cv::FastFeatureDetector(threshold, nonmaxSuppression, TYPE_9_16)::detect(
 * image, keypoints, mask): keypoints in OpenCV's raster emission order, NMS
 * strict-greater over 8 neighbours, then runByPixelsMask. mask: host W*H u8
 * (row stride w) or NULL. Writes min(n, cap) keypoints; *n_out = n. */
int svo_fast_detect(svo_ctx* ctx, const svo_image* img, int threshold, int nonmax,
                    const uint8_t* mask, svo_keypoint* out, int cap, int* n_out);
/* Kernel-level view for parity tests: per-pixel FAST score (0 = no corner)
 * and corner flag, both W*H u8. */
int svo_fast_score_map(svo_ctx* ctx, const svo_image* img, int threshold,
                       uint8_t* score, uint8_t* corner);
/* ------------------------------------------------------------ ORB: detection
 * The reference's shipped default detector (use_orb: 1, R:configs/config.yaml:20-27):
 * cv::ORB::create(nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel, WTA_K,
 * scoreType, patchSize, fastThreshold) at R:src/tracking.cpp:33-50, used through
 * detect(img, keypoints, mask) at :82. Keypoints in OpenCV's order (level by level,
 * retainBest's order within a level), pt scaled to level 0; response = Harris (or
 * FAST) score; octave optional (may be NULL). Angles are not computed here (the
 * reference keeps positions only, R:src/tracking.cpp:85); svo_orb_compute below
 * computes them with the descriptors. firstLevel must be 0. */
#define SVO_ORB_HARRIS_SCORE 0
#define SVO_ORB_FAST_SCORE 1
typedef struct svo_orb_params {
    int nfeatures;        /* R:configs/config.yaml:22 (150) */
    float scale_factor;   /* 1.2 */
    int nlevels;          /* 8 (<= 8) */
    int edge_threshold;   /* the reference passes patch_size (31) */
    int first_level;      /* 0 */
    int wta_k;            /* 4 in the reference; unused by detect; the descriptors support 2 only */
    int score_type;       /* SVO_ORB_HARRIS_SCORE */
    int patch_size;       /* 31 */
    int fast_threshold;   /* 20 */
} svo_orb_params;
int svo_orb_detect(svo_ctx* ctx, const svo_image* img, const svo_orb_params* params,
                   const uint8_t* mask, svo_keypoint* out, int* octave, int cap, int* n_out);
/* Test and debug only (parity tests of the scale and mask pyramids): builds the
 * pyramids exactly as svo_orb_detect does, by the same code, and copies out level
 * `level`: out_img lw*lh u8 (tight rows), out_mask the same or NULL (left unwritten
 * without a mask). Level 0 is the caller's image and mask; the masks of levels
 * 1.. are thresholded (255 or 0). *lw, *lh: the level's size (either may be NULL;
 * out_img must hold at least W*H bytes if the size is not known beforehand).
 * SVO_ERR_ARG: level outside [0, nlevels), or parameters svo_orb_detect rejects. */
int svo_orb_level(svo_ctx* ctx, const svo_image* img, const svo_orb_params* params, const uint8_t* mask,
                  int level, uint8_t* out_img, uint8_t* out_mask, int* lw, int* lh);

/* ------------------------------------------------------------ ORB: descriptors and matching
 * Not in the reference (it only detects): where cv::ORB::compute / detectAndCompute
 * and cv::BFMatcher(NORM_HAMMING)::knnMatch(k = 2) would stand in a port, for
 * relocalisation against a map of described points. Every rule is stated in
 * DESIGN.md section 3d and restated in numpy by tests/orb_describe_reference.py;
 * parity with OpenCV's own bits is NOT pinned (its learned pattern is data the
 * caller passes; its u8 GaussianBlur weights and its float cos/sin steering differ).
 *
 * For a keypoint (x, y, octave) as svo_orb_detect returns it, hp = patch_size / 2:
 *   level pixel  cx = cvRound(x * (1.f / lscale[octave])) in f32, cy likewise
 *   validity     reach = cvRound(hp sqrt 2); valid iff reach <= cx <= lw - 1 - reach and
 *                the same for cy; else valid = 0, a zero descriptor, angle -1
 *   moments      m10 = sum u I, m01 = sum v I on the UNBLURRED level over |v| <= hp,
 *                |u| <= umax[|v|] (OpenCV's umax table), exact integers
 *   direction    hyp = sqrt((double)(m10^2 + m01^2)), c = m10 / hyp, s = m01 / hyp in
 *                f64 (c = 1, s = 0 without a gradient); angle = atan2(m01, m10) in
 *                degrees [0, 360), informational only
 *   blur         every level once, separable 7 taps {18,34,49,54,49,34,18} / 256,
 *                REFLECT_101: h = sum w p, out = (sum w h + 32768) >> 16
 *   steering     pattern point (px, py): ix = rint(px c - py s), iy = rint(px s + py c)
 *                in f64, half to even; sample = blurred[cy + iy][cx + ix]
 *   bits         WTA_K 2: bit j of byte i = sample(pattern[16i + 2j]) < sample(pattern[16i + 2j + 1])
 * pattern_xy: 512 points (x, y) int8, each in [-hp, hp] (OpenCV's bit_pattern_31_
 * for patch_size 31 if the caller has it), or NULL for svo_orb_default_pattern.
 * SVO_ERR_ARG (nothing written): patch_size even or outside [5, 31], wta_k != 2,
 * first_level != 0, a pattern entry outside [-hp, hp], an octave outside
 * [0, nlevels), negative counts, parameters svo_orb_detect rejects. */
#define SVO_ORB_DESC_BYTES 32
/* OpenCV's pattern for patchSize != 31 (makeRandomPattern): cv::RNG(0x34985739),
 * x = uniform(-hp, hp + 1) then y likewise, 512 points. Host only, no context. */
int svo_orb_default_pattern(int patch_size, int8_t pattern_xy[1024]);
/* Test view (host only): the hp + 1 entries of umax; writes min(hp + 1, cap), *n = hp + 1. */
int svo_orb_umax(int patch_size, int* umax, int cap, int* n);
/* desc n*32 bytes, angle n floats or NULL, valid n bytes. n = 0 is valid. */
int svo_orb_compute(svo_ctx* ctx, const svo_image* img, const svo_orb_params* params, const int8_t* pattern_xy,
                    const svo_keypoint* kp, const int* octave, int n, uint8_t* desc, float* angle, uint8_t* valid);
/* svo_orb_detect, then svo_orb_compute of its keypoints on the same pyramid (built
 * once). kp / octave / *n_out as svo_orb_detect writes them (octave and angle may be
 * NULL); desc, angle, valid for the min(n, cap) keypoints written. */
int svo_orb_detect_and_compute(svo_ctx* ctx, const svo_image* img, const svo_orb_params* params, const uint8_t* mask,
                               const int8_t* pattern_xy, svo_keypoint* kp, int* octave, uint8_t* desc, float* angle,
                               uint8_t* valid, int cap, int* n_out);
/* Test view, as svo_orb_level: level `level` of the blurred pyramid the descriptors sample. */
int svo_orb_blur_level(svo_ctx* ctx, const svo_image* img, const svo_orb_params* params, int level, uint8_t* out,
                       int* lw, int* lh);
/* Hamming 2-NN of 32-byte descriptors, n_problems independent problems: problem p
 * matches queries q + p*q_stride*32 (nq[p] of them) against train t + p*t_stride*32
 * (nt[p]). For query i of problem p, idx[(p*q_stride + i)*2 + k] and dist[...] hold
 * the best (k = 0) and second-best (k = 1) train index and distance (popcount of
 * the xor, 0..256) by strict < while the train index rises: ties go to the lowest
 * index. A missing neighbour (nt[p] of 0 or 1) is idx -1, dist 257. Rows past nq[p]
 * are not written. SVO_ERR_ARG: negative counts, a count above its stride, more
 * than 65535 problems. n_problems = 0 is valid. */
int svo_match_hamming(svo_ctx* ctx, int n_problems, const int* nq, const int* nt, int q_stride, int t_stride,
                      const uint8_t* q, const uint8_t* t, int* idx, int* dist);
/* Ratio test and cross-check on svo_match_hamming's output of one problem (host
 * only, integers): keep (q, t = idx_qt[2q]) iff t >= 0, and (ratio_pct != 0)
 * idx_qt[2q+1] >= 0 with dist1 * 100 < ratio_pct * dist2, and (idx_tq != NULL: the
 * reverse match, nt rows) idx_tq[2t] == q. Pairs in ascending q; writes min(n, cap)
 * pairs, *n_out = n. SVO_ERR_ARG (nothing written): negative counts or ratio, an
 * index >= nt. */
int svo_match_filter(const int* idx_qt, const int* dist_qt, int nq, const int* idx_tq, int nt, int ratio_pct,
                     int* pairs, int cap, int* n_out);
/* svo_match_filter on the device, for n_problems problems at once, in the layout of
 * svo_match_hamming's outputs: idx_qt / dist_qt rows (p*q_stride + q)*2 of the
 * forward match (nq[p] live rows, train count nt[p]), idx_tq rows (p*t_stride + t)*2
 * of the reverse match (nt[p] live rows) or NULL for no cross-check. Per problem the
 * kept pairs (q, t) in ascending q go to pairs[(p*q_stride + i)*2 ..], i < n_pairs[p]
 * (at most nq[p]); rows past n_pairs[p] are not written. One block per problem, a
 * stable compaction by wave ballots. SVO_ERR_ARG (nothing written): negative counts
 * or ratio, a count above its stride, more than 65535 problems, null arrays, a live
 * idx_qt entry >= nt[p]. n_problems = 0 is valid. */
int svo_match_filter_batch(svo_ctx* ctx, int n_problems, const int* nq, const int* nt, int q_stride, int t_stride,
                           const int* idx_qt, const int* dist_qt, const int* idx_tq, int ratio_pct, int* pairs,
                           int* n_pairs);
/* Measurement only (tools/orb_describe_bench.py): HIP-event time per launch, in ms,
 * over `reps` back-to-back launches after a warm-up, no transfers. svo_orb_describe_time:
 * detects up to cap keypoints of img (*n_kp), then ms[0] orb_blur_kernel (all levels),
 * ms[1] orb_angle_kernel, ms[2] orb_brief_kernel on them, default pattern.
 * svo_match_hamming_time: hamming_knn2_kernel on the uploaded problems. */
int svo_orb_describe_time(svo_ctx* ctx, const svo_image* img, const svo_orb_params* params, int cap, int reps,
                          double ms[3], int* n_kp);
int svo_match_hamming_time(svo_ctx* ctx, int n_problems, const int* nq, const int* nt, int q_stride, int t_stride,
                           const uint8_t* q, const uint8_t* t, int reps, double* ms);
/* Matching map points to a frame by projection: where
 * ORBmatcher::SearchByProjection would stand in a port. Problem p of n_problems
 * has n_pts[p] points xyz + (p*p_stride + i)*3 (f64, world) with descriptors pdesc
 * + (p*p_stride + i)*32, n_kp[p] keypoints kxy + (p*k_stride + j)*2 (f32 pixels)
 * with descriptors kdesc + (p*k_stride + j)*32, and a pose poses + 12 p: T = [R
 * row-major | t], world -> camera. K4 = (fx, fy, cx, cy); w x h: the frame.
 *  1. Projection, f64, in this order: px = T0 X + T1 Y + T2 Z + T9 summed left to
 *     right, py (T3 T4 T5 T10) and pz (T6 T7 T8 T11) likewise; iz = 1 / pz,
 *     u = fx (px iz) + cx, v = fy (py iz) + cy; uf = (float)u, vf = (float)v.
 *     proj = (uf, vf) if pz > 0, else (-1, -1). The point is visible iff pz > 0 and
 *     0 <= uf < (float)w and 0 <= vf < (float)h (a NaN fails).
 *  2. Keypoint j is usable iff 0 <= kx < (float)w and 0 <= ky < (float)h (a NaN is
 *     not). It is a candidate of a visible point iff it is usable and fabsf(kx - uf)
 *     <= radius and fabsf(ky - vf) <= radius in f32: a square window, edge included.
 *  3. d = popcount(pdesc_i xor kdesc_j). The best candidate is the smallest (d, j)
 *     taken lexicographically, the second best the next smallest: idx[(p*p_stride +
 *     i)*2 + k] and dist[...] as svo_match_hamming's, a missing neighbour -1 / 257; a
 *     point that is not visible or has no candidate gets (-1, -1) and (257, 257).
 *  4. Point i bids for j = idx[i][0] iff j >= 0, dist[i][0] <= max_dist, and
 *     ratio_pct == 0 or there is no second neighbour or dist[i][0] * 100 < ratio_pct
 *     * dist[i][1] (a single candidate passes). Each keypoint goes to the bidder
 *     with the smallest (d, i). pairs[(p*k_stride + k)*2 ..] = (j, i) in ascending
 *     j, k < n_pairs[p]: the keypoint first, as the frame comes first in
 *     svo_frontend_places_query's pairs.
 * Nothing depends on the search structure: every choice is a minimum over keys.
 * Rows past the counts are not written. Any of idx, dist, proj, pairs may be NULL
 * to skip it; n_pairs is required with pairs. SVO_ERR_ARG (nothing written): a null
 * context or params, negative counts, a count above its stride, more than 65535
 * problems, a stride above 2^20, w or h < 1, radius not finite or <= 0, max_dist
 * outside [0, 256], ratio_pct < 0, a null required array while any count is
 * positive. n_problems = 0 is valid. */
typedef struct svo_proj_match_params {
    float radius;  /* half side of the search window in pixels; default 4 */
    int max_dist;  /* a best distance above this does not bid; default 64 */
    int ratio_pct; /* ratio test in percent, 0 = off; default 80 */
} svo_proj_match_params;
int svo_match_projected(svo_ctx* ctx, int n_problems, const int* n_pts, const int* n_kp, int p_stride, int k_stride,
                        const double* xyz, const uint8_t* pdesc, const float* kxy, const uint8_t* kdesc,
                        const double* poses, const double* K4, int w, int h, const svo_proj_match_params* params,
                        int* idx, int* dist, float* proj, int* pairs, int* n_pairs);
/* Measurement only (tools/match_projected_bench.py), as svo_match_hamming_time: ms
 * per launch of ms[0] proj_bin_kernel, ms[1] proj_match_kernel, ms[2]
 * proj_pairs_kernel on the uploaded problems. */
int svo_match_projected_time(svo_ctx* ctx, int n_problems, const int* n_pts, const int* n_kp, int p_stride,
                             int k_stride, const double* xyz, const uint8_t* pdesc, const float* kxy,
                             const uint8_t* kdesc, const double* poses, const double* K4, int w, int h,
                             const svo_proj_match_params* params, int reps, double ms[3]);
/* T = [R(rvec) | tvec] as svo_match_projected takes it (cv::Rodrigues; host only,
 * no context): what svo_solve_pnp_ransac returns, turned into a pose. */
int svo_pose_from_rvec(const double rvec[3], const double tvec[3], double T[12]);

/* R:src/tracking.cpp:76-79: W*H mask of 255 with a filled box of +-half around
 * each point (cvRound corners, inclusive, clipped). Host output. */
int svo_mask_boxes(svo_ctx* ctx, int w, int h, const float* pts_xy, int n, float half,
                   uint8_t* mask);

/* ------------------------------------------------------------ bucketing
 * FeatureSet::bucketingFeatures(image(w,h), bucket_size, features_per_bucket)
 * with the reference's exact output (R:src/bucket.cpp:24-106 quirks included).
 * ages may be NULL (all 0, as appendNewFeatures sets them). */
int svo_bucket_features(svo_ctx* ctx, const float* xy, const int* ages, int n, int img_w,
                        int img_h, int bucket_size, int per_bucket, float* xy_out,
                        int* ages_out, int cap, int* n_out);

/* ------------------------------------------------------------ LK
 * cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err,
 * Size(win_w, win_h), max_level, TermCriteria(crit_type, max_count, epsilon),
 * flags, min_eig_threshold). next_xy is read as the initial guess when
 * SVO_LK_USE_INITIAL_FLOW is set. err may be NULL. Pyramids must have been
 * built with at least the levels this window allows. */
int svo_calc_optical_flow_pyr_lk(svo_ctx* ctx, const svo_image* prev, const svo_image* next,
                                 const float* prev_xy, int n, float* next_xy,
                                 uint8_t* status, float* err, int win_w, int win_h,
                                 int max_level, int crit_type, int max_count, double epsilon,
                                 int flags, double min_eig_threshold);
/* The same call as two launches, points [0, split) and [split, n) (0 <= split <= n;
 * 0 or n: one launch): a point's result does not depend on the launch it is in, so
 * the outputs equal svo_calc_optical_flow_pyr_lk's bit for bit (the batched front
 * end tracks a keyframe's new features in a launch of their own). */
int svo_calc_optical_flow_pyr_lk_split(svo_ctx* ctx, const svo_image* prev, const svo_image* next,
                                       const float* prev_xy, int n, int split, float* next_xy,
                                       uint8_t* status, float* err, int win_w, int win_h,
                                       int max_level, int crit_type, int max_count,
                                       double epsilon, int flags, double min_eig_threshold);
/* Gauss-Newton iterations executed by the last LK call, summed over points and
 * levels (the "LK iters/s" metric numerator). */
int64_t svo_lk_last_iterations(const svo_ctx* ctx);

/* ------------------------------------------------------------ stereo rows
 * (not in the reference, whose findLeftFeaturesInRight is an 11x11 LK that
 * recovers disparities up to about 70 px:) "row SAD", the stereo match of a
 * RECTIFIED pair as a bounded search along the left point's own row. Exact
 * integer arithmetic up to the sub-pixel step. Per left point (x, y), images L
 * and R of w x h read at level 0 with its stored REFLECT_101 border:
 *  1. xi = cvRound(x), yi = cvRound(y) (half to even); outside the image: status 0.
 *  2. candidates: the integers d in [max(d_min, xi - (w - 1)), min(d_max, xi)]
 *     (the right centre xi - d stays inside); fewer than 3: status 0.
 *  3. cost(d) = sum over i, j in [-r, r] of |L[yi+i][xi+j] - R[yi+i][xi-d+j]|.
 *  4. d* = the smallest d of minimal cost; the first or last candidate: status 0.
 *  5. max_cost > 0 and cost(d*) > max_cost: status 0.
 *  6. uniq_pct > 0: with second = the least cost over candidates |d - d*| >= 2
 *     (if there is one), status 0 unless cost(d*) * 100 < uniq_pct * second.
 *  7. c-, c0, c+ = the costs at d* - 1, d*, d* + 1; den = c- + c+ - 2 c0 (>= 0);
 *     delta = 0 if den == 0, else float(c- - c+) / float(2 den) (one float32
 *     division); xr = x - (float(d*) + delta) in float32; yr = y.
 *  8. next_xy = (xr, yr) with status 1, (x, y) with status 0; disparity = d* and
 *     cost = c0, both 0 with status 0.
 * SVO_ERR_ARG (nothing written): radius outside 1..7, d_min < -16, d_max > 255,
 * d_max - d_min + 1 outside 3..256, uniq_pct outside 0..100, max_cost < 0. */
typedef struct svo_stereo_rows_params {
    int radius;   /* patch (2 radius + 1)^2; default 5 */
    int d_min;    /* lowest disparity searched; default -1 */
    int d_max;    /* highest disparity searched; default 128 */
    int uniq_pct; /* uniqueness test in percent, 0 = off; default 80 */
    int max_cost; /* reject a best cost above this, 0 = off; default 0 */
} svo_stereo_rows_params;
/* left / right: images of equal size whose level 0 is uploaded (any upload call
 * writes the border). n = 0 is valid. disparity / cost (n ints each) may be NULL.
 * SVO_ERR_ARG (nothing written) in addition: a null ctx, image, params, pts_xy,
 * next_xy or status (n > 0), n < 0, sizes that differ. */
int svo_stereo_match_rows(svo_ctx* ctx, const svo_image* left, const svo_image* right, const float* pts_xy, int n,
                          const svo_stereo_rows_params* params, float* next_xy, uint8_t* status, int* disparity,
                          int* cost);

/* Guided row SAD: svo_stereo_match_rows where point i searches its own range
 * [d_min_i, d_max_i] in place of [d_min, d_max]:
 *   d_prior[i] == SVO_STEREO_NO_PRIOR: [d_min, d_max];
 *   otherwise [max(d_min, d_prior[i] - guide), min(d_max, d_prior[i] + guide)],
 *   evaluated without overflow (every other int is a valid prior).
 * Steps 1-8 above run with that range and nothing else changes, so: a range that
 * step 2 leaves fewer than 3 candidates of gives status 0; a best cost at either
 * end of the guided range gives status 0 (the prior was wrong, or the minimum
 * lies outside); the uniqueness test sees the guided candidates only.
 * d_prior == NULL, or guide == 0 with any priors, returns svo_stereo_match_rows'
 * outputs. SVO_ERR_ARG (nothing written): whatever svo_stereo_match_rows
 * refuses, guide outside 0..15. */
#define SVO_STEREO_NO_PRIOR INT32_MIN
int svo_stereo_match_rows_guided(svo_ctx* ctx, const svo_image* left, const svo_image* right, const float* pts_xy,
                                 int n, const svo_stereo_rows_params* params, const int* d_prior, int guide,
                                 float* next_xy, uint8_t* status, int* disparity, int* cost);
/* The prior of a tracked feature: its disparity one frame ago. Per feature i,
 * mid[i] is looked up in prev_mid (prev_n ids, strictly increasing, as a window
 * slot's are); found at j with prev_ur[j] >= 0: d_prior[i] = cvRound(prev_xy[2j] -
 * prev_ur[j]) (one float32 subtraction, rounded half to even), or
 * SVO_STEREO_NO_PRIOR where that is not finite or outside +-32767; absent, or
 * prev_ur[j] < 0, or prev_n == 0: SVO_STEREO_NO_PRIOR. n = 0 is valid.
 * SVO_ERR_ARG (nothing written): null ctx, n < 0, prev_n < 0, a null array of a
 * count > 0. */
int svo_stereo_row_priors(svo_ctx* ctx, const int* mid, int n, const int* prev_mid, const float* prev_xy,
                          const float* prev_ur, int prev_n, int* d_prior);

/* ------------------------------------------------------------ PnP
 * Batched reprojection residual: M hypotheses (R row-major 3x3, t 3: 12
 * doubles each) x N points. Equals PnPRansacCallback::computeError (projectPoints
 * with K, zero distortion, CV_32F output; err = |ipt - ppt|^2 in float) and
 * findInliers (err <= thresh2). err (M*N floats), mask (M*N bytes), counts (M)
 * may each be NULL. obj_xyz are floats (OpenCV converts Point3d to CV_32F). */
int svo_pnp_residuals(svo_ctx* ctx, const float* obj_xyz, const float* img_xy, int n,
                      const double* hyp_Rt, int m, const double K[9], float thresh2,
                      float* err, uint8_t* mask, int* counts);

/* cv::solvePnPRansac(obj(Point3d), img(Point2f), K, zeros(1,4), rvec, tvec,
 * useExtrinsicGuess=false, iterations, reproj_err, confidence, inliers,
 * SOLVEPNP_SQPNP). Returns 1 (model found), 0 (no model) or < 0 (error).
 * inliers: capacity n ints, written in ascending order. */
int svo_solve_pnp_ransac(svo_ctx* ctx, const double* obj_xyz, const float* img_xy, int n,
                         const double K[9], int iterations, float reproj_err,
                         double confidence, double rvec[3], double tvec[3], int* inliers,
                         int* n_inliers);

/* cv::solvePnP(obj(Point3d), img(Point2f), K, zeros(1,4), rvec, tvec, false,
 * SOLVEPNP_SQPNP): the fit solvePnPRansac ends with (calib3d/src/sqpnp.cpp's cost
 * and solution search; host only, no context). Returns 1 (pose found), 0
 * (SQPnP's asserts -- degenerate points -- or no solution in front of the
 * camera) or SVO_ERR_ARG (null pointers, n < 3). */
int svo_solve_pnp_sqpnp(const double* obj_xyz, const float* img_xy, int n, const double K[9], double rvec[3],
                        double tvec[3]);

/* RANSAC's minimal solver alone: SOLVEPNP_EPNP on 5 points, the model estimator
 * solvePnPRansac runs per hypothesis (R:src/tracking.cpp:191-196), for m subsets
 * given as 25 floats each (obj xyz x5, then img xy x5, as the front end gathers
 * them). device = 0: the host solver the RANSAC uses (OpenCV's epnp.cpp with its
 * Jacobi SVDs, bit-identical to the oracle's restatement; no context needed);
 * device = 1: one 64-lane wave per subset on the GPU (epnp_wave.hpp), a QL-based
 * variant kept off the path; device = 2: that variant's host twin (bit-identical
 * to device 1; no context needed); device = 3 / 4 / 5: the device = 0 solver
 * forced to its scalar / AVX2-lane / AVX-512-lane form (SVO_ERR_NODEVICE when the
 * CPU lacks the instruction set); device = 6: the device = 0 solver on the GPU, one
 * lane per subset (epnp_lane.hip; bit-identical to device 0). Rt: m x 12 doubles
 * (R row-major, t); ok: m ints (0: non-finite model). */
int svo_epnp_subsets(svo_ctx* ctx, const float* subsets, int m, const double K[9], int device, double* Rt,
                     int* ok);

/* The batched front end's RANSAC kernels, one launch each (test entry points; the
 * front end does not call them). S sequences of up to cap points: obj f32
 * [S][cap][3], img f32 [S][cap][2], counts[S] points each (slots past a count are
 * not read). Each returns SVO_ERR_ARG before anything is launched or written: a
 * null ctx (svo_sqpnp_fit with device = 0 needs none) or a null array with S > 0,
 * S / cap / words_cap < 0, a count outside [0, cap] or with more than words_cap
 * words of 32 bits. S = 0 is valid.
 *
 * svo_pnp_score: the scoring of a RANSAC round (pnp_score_kernel, one block per
 * hypothesis and sequence): hyps f64 [S][m_stride][12] (R row-major, t), the first
 * m rows of every sequence scored as svo_pnp_residuals scores them (err <=
 * thresh2); bits u32 [S][m_stride][words_cap], bit i & 31 of word i / 32 = point i
 * an inlier, and cnt i32 [S][m_stride], the inliers per row. bits and cnt are read
 * as well: rows >= m and words >= (count + 31) / 32 come back as given. Also
 * SVO_ERR_ARG: m < 0, m_stride < 1, m > m_stride. */
int svo_pnp_score(svo_ctx* ctx, const float* obj, const float* img, const int* counts, int S, int cap,
                  const double* hyps, int m, int m_stride, const double K[9], float thresh2, uint32_t* bits,
                  int words_cap, int* cnt);

/* svo_sqpnp_stats: SQPnP's 40 sufficient statistics (svo_sqpnp_fit's input) of the
 * points of every sequence whose bit is set in bits u32 [S][words_cap]
 * (suffstats_kernel: one 256-thread block per sequence; thread k sums its points
 * k, k + 256, ... in order, a 64-lane xor butterfly, then ((w0 + w1) + w2) + w3):
 * stats f64 [S][40] = n, sum x, sum y, sum (x^2 + y^2), sum c X for c in (1, x, y,
 * x^2 + y^2), sum c X X^T (6 unique entries each), (x, y) = ((u - cx) / fx, (v -
 * cy) / fy). Bits at or above a count are ignored. */
int svo_sqpnp_stats(svo_ctx* ctx, const float* obj, const float* img, const int* counts, int S, int cap,
                    const uint32_t* bits, int words_cap, const double K[9], double* stats);

/* svo_sqpnp_fit: the final SQPnP fit of every sequence from its statistics and
 * the pose the front end reports. mode[S]: 0 no model (pose6 = 0, pose12 the
 * identity), 1 fit on the points of `bits` (R [S][9], t [S][3]: the RANSAC model,
 * kept where SQPnP asserts or finds nothing in front of the camera), 2 given (rv
 * [S][3], t: passed through). device = 1: the device fit (launch_sqpnp_fit);
 * device = 0: what the front end's host pool runs (RansacSeq::fit, then
 * Frame::pose()). pose6 [S][6] = (rvec, tvec), pose12 [S][12] = camera -> world
 * (R^T row-major, -R^T t). Also SVO_ERR_ARG: a mode outside 0..2, device outside
 * 0..1. */
int svo_sqpnp_fit(svo_ctx* ctx, const double* stats, const int* mode, const double* R, const double* t,
                  const double* rv, const float* obj, const int* counts, int S, int cap, const uint32_t* bits,
                  int words_cap, int device, double* pose6, double* pose12);

/* svo_trig_pa (test view): the sin / cos / acos of the final fit's rotation vector and
 * Frame::pose() (trig_pa.hpp: double-double in plain arithmetic, the same
 * operations on host and device) on n arguments. fn = 0: out[2 i] = sin x_i, out[2 i
 * + 1] = cos x_i (0 <= x <= 8; outside, the maths library's); fn = 1: out[2 i] =
 * acos x_i, out[2 i + 1] = 0. device = 0: on the host (no context needed); 1: on
 * the GPU. SVO_ERR_ARG: n < 0, fn outside 0..1, device outside 0..1, a null array
 * with n > 0, device = 1 without a context. */
int svo_trig_pa(svo_ctx* ctx, const double* x, int n, int fn, int device, double* out);

/* ------------------------------------------------------------ triangulation
 * cv::triangulatePoints(P1, P2, pts1, pts2, points4D) then
 * cv::convertPointsFromHomogeneous (R:src/tracking.cpp:125-131). P1, P2: 3x4
 * row-major float (cv::Matx34f). Per point the DLT null vector of the 4x4
 * system, unit length with w >= 0 (OpenCV's sign is arbitrary and cancels),
 * rounded to float -> xyzw (4n, may be NULL); xyz = xyzw[0:3] * (1/w) in float
 * (3n, may be NULL). */
int svo_triangulate_points(svo_ctx* ctx, const float P1[12], const float P2[12], const float* pts1,
                           const float* pts2, int n, float* xyzw, float* xyz);

/* ------------------------------------------------------------ reprojection cost (§8 a11)
 * The north star's "ceres reprojection cost": Ceres is linked by the reference
 * but never called (R:CMakeLists.txt:22,33), so there is no
 * reference implementation; pinned by finite differences.
 * P problems of up to max_n points each (obj: P*max_n*3 doubles, img:
 * P*max_n*2 floats, counts: P or NULL = max_n each), poses: P x 12 doubles
 * ([R|t], world -> camera, R row-major). Per point: r = pi(K (R X + t)) - u and
 * J = dr/dxi (2x6 row-major) for T <- exp(xi^) T, xi = (rho, phi). normal:
 * P x 28 = H (upper triangle of sum w J^T J, row-major, 21), g (sum w J^T r,
 * 6), cost (sum of rho(|r|)); w, rho: Huber with delta > 0, else least
 * squares. Points behind the camera contribute 0. Outputs may be NULL;
 * results are deterministic (fixed reduction order). */
int svo_reprojection_jacobians(svo_ctx* ctx, const double* obj_xyz, const float* img_xy, const int* counts,
                               int n_problems, int max_n, const double* poses, const double K[9],
                               double huber_delta, double* res, double* jac, double* normal);
/* Host Levenberg-Marquardt over SE(3) (motion-only bundle adjustment), one
 * batched GPU evaluation per iteration for all P problems. poses: in/out.
 * costs (P, final cost) and iterations may be NULL. */
int svo_refine_poses(svo_ctx* ctx, const double* obj_xyz, const float* img_xy, const int* counts, int n_problems,
                     int max_n, const double K[9], double huber_delta, int max_iterations, double* poses,
                     double* costs, int* iterations);
/* Motion-only refinement from stereo observations, on the device (§8 a11d): the
 * pose of each problem from its observations with the points held constant
 * (ORB-SLAM's motion-only BA), svo_refine_poses' Levenberg-Marquardt rule by
 * rule -- lambda from 1e-4; A_ii += lambda (A_ii > 0 ? A_ii : 1e-12); Cholesky,
 * lambda x10 up to 1e16 while not positive definite, then the problem ends; the
 * step rule |dx| < 1e-12 (1 + |t|); T <- exp(xi^) T; accept if c1 <= c0, then
 * lambda <- max(0.1 lambda, 1e-12) and stop if c0 - c1 <= 1e-15 c0; else lambda
 * x10, stop at 1e16 -- kept per problem and run, all of it, by one workgroup in
 * one launch: one upload, one launch, one download, whatever max_iterations is.
 * Inputs as svo_reprojection_jacobians' plus img_ur (P*max_n floats): the right
 * image's column of each observation, < 0 for a monocular one, and the rig's
 * baseline. Every observation is evaluated as svo_bundle_adjust_stereo states it
 * below (the third residual and its pose-Jacobian row, the Huber norm over the
 * residual the observation has, Pz <= 0 contributes nothing, ur < 0 exactly
 * svo_reprojection_jacobians' evaluation); the points do not move. All
 * arithmetic is double. The 28 sums (H 21, g 6, cost) of a problem of n
 * observations are formed in one order: thread t of 256 adds observations t,
 * t + 256, ... in ascending order (starting from the first one's terms; an
 * observation that contributes nothing adds +0); the 64 lanes of each wave are
 * summed by the xor butterfly 32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) +
 * w2) + w3. For n <= 256 and img_ur all negative that is
 * svo_reprojection_jacobians' normal, bit for bit. The order depends on nothing
 * outside the problem (not on n_problems, max_n or the other problems), so a
 * problem gets the same bits alone and in any batch, run after run.
 * poses: in/out. costs: P x 2 (initial, final). iterations: P, the iterations
 * each problem began, the one that gives up or stops on the step rule included
 * (svo_bundle_adjust's convention). normal: P x 28 = H, g, cost at the returned
 * pose; H is the undamped sum w J^T J, the pose's information matrix (its
 * inverse is the covariance of xi for unit pixel noise). All three may be NULL.
 * max_iterations == 0 is a pure linearisation: poses keep their bits, both costs
 * are equal, iterations are 0. Values that are not finite follow
 * svo_bundle_adjust's rule: a problem with a NaN or an infinity in its pose, or
 * within its count in its points, img_xy or img_ur, or whose initial cost is not
 * finite, is not iterated on; its pose keeps its bits, its costs and its normal
 * are NaN, its iteration count is 0, and the other problems get what they get
 * alone. n_problems == 0 or max_n == 0: SVO_OK (max_n == 0: every problem is the
 * empty one, cost 0, pose bits kept). SVO_ERR_ARG (nothing written):
 * svo_refine_poses' bad arguments; img_ur NULL with work to do; baseline not
 * finite or <= 0; max_iterations outside 0 .. SVO_REFINE_MAX_ITERATIONS (the
 * bound that keeps a launch finite on any input). */
#define SVO_REFINE_MAX_ITERATIONS 1000
int svo_refine_poses_stereo(svo_ctx* ctx, const double* obj_xyz, const float* img_xy, const float* img_ur,
                            const int* counts, int n_problems, int max_n, const double K[9], double baseline,
                            double huber_delta, int max_iterations, double* poses, double* costs, int* iterations,
                            double* normal);
/* svo_refine_poses_stereo's launch timed with HIP events: reps launches after one
 * warm-up, each from `poses` (which stay as they are), ms per whole LM launch
 * (ms_device). Beside it the wall time per call of svo_refine_poses (ms_host: the
 * host loop, one round trip per iteration) on the same img_xy from the same
 * poses with the same max_iterations, reps calls after one warm-up; it ignores
 * img_ur. SVO_ERR_ARG in addition: nothing to run, reps <= 0, an output NULL. */
int svo_refine_poses_time(svo_ctx* ctx, const double* obj_xyz, const float* img_xy, const float* img_ur,
                          const int* counts, int n_problems, int max_n, const double K[9], double baseline,
                          double huber_delta, int max_iterations, const double* poses, int reps, double* ms_device,
                          double* ms_host);

/* ------------------------------------------------------------ pose-graph optimisation (§10)
 * The back end behind place recognition: the poses of many frames from relative-
 * pose measurements between them, odometry edges and loop edges alike, by a robust
 * least squares over all poses at once. P problems of up to max_nodes <=
 * SVO_PG_MAX_NODES nodes and max_edges <= SVO_PG_MAX_EDGES edges each; n_nodes /
 * n_edges: P counts, or NULL = the maximum (a ragged batch, as svo_bundle_adjust's).
 * Node i is a pose T_i = [R|t], world -> camera, 12 doubles, R row-major (poses:
 * P*max_nodes*12). fixed (P*max_nodes bytes): non-zero holds the node; a problem
 * with no fixed node is allowed -- the damping makes the system solvable, and the
 * result keeps whatever gauge the start had. An edge (edge_ij: P*max_edges pairs
 * i, j; edge_Z: 12 doubles; edge_info: 21 doubles) measures Z ~ T_j T_i^-1 with the
 * symmetric 6x6 information matrix Omega, given as its upper triangle row-major in
 * the order (rho, phi): the first 21 entries of svo_refine_poses_stereo's normal,
 * so a refined pose's information is handed in as it is.
 *   A = T_j T_i^-1, E = A Z^-1 = [R_e | t_e], e = (t_e, log R_e);
 *   log R = f(th) v, v = 1/2 vee(R - R'), th = acos(clamp((tr R - 1)/2, -1, 1)),
 *   f = th / sin th, and 1 + th^2/6 for th < 1e-4; acos, sin and cos in plain
 *   arithmetic (svo_trig_pa's), so an edge's terms are the same bits on host and
 *   device. The rule is for th < pi: at th = pi, f is 2.6e16 (the sine of the
 *   double nearest pi), every term stays finite and the edge is not refused.
 *   Jacobians for T <- exp(xi^) T, xi = (rho, phi):
 *   D = [[I, -[t_e]x], [0, Jl^-1(log R_e)]], Jl^-1(p) = I - 1/2 [p]x + k [p]x^2,
 *   k = 1/th^2 - (1 + cos th)/(2 th sin th), and 1/12 for th < 1e-4;
 *   J_j = D, J_i = -D Ad(A), Ad(A) = [[R_A, [t_A]x R_A], [0, R_A]].
 *   Cost: q = e' Omega e, s = sqrt(q), Huber on s with huber_delta (<= 0: none):
 *   w = 1 or delta/s, cost q/2 or delta (s - delta/2). q < 0 (an indefinite Omega)
 *   adds nothing: w = 0, cost 0.
 * Levenberg-Marquardt per problem, svo_refine_poses' control: lambda from 1e-4;
 * H_kk += lambda (H_kk > 0 ? H_kk : 1e-12) on every diagonal entry; the step rule
 * |dx| < 1e-12 (1 + |t|) over the whole state (dx of every node, t of every node);
 * T <- exp(xi^) T per free node; accept on c1 <= c0, lambda <- max(0.1 lambda,
 * 1e-12), stop once c0 - c1 <= 1e-15 c0; else lambda x10, stop at 1e16. The
 * damped system over the free nodes is solved by conjugate gradients with the
 * block-Jacobi preconditioner (the Cholesky factor of each node's damped 6x6 block,
 * svo_refine_poses' arithmetic), from x = 0, until r'z <= (1e-8)^2 r0'z0 or max_cg
 * products; at that cap the step is used as it stands and the verdict decides. A
 * diagonal block that is not positive definite, or a p'Ap that is not positive or
 * not finite, counts as "not positive definite": lambda x10 and solve again, up to
 * 1e16, where the problem ends. All of it runs in one workgroup of one launch, in
 * double, with one summation order:
 *   - a node's diagonal block (21) and gradient (6) are the sums over its incident
 *     edges in ascending edge index, whichever end it is, starting from the first
 *     edge's term;
 *   - row k of the matrix-vector product is the node's damped diagonal block's
 *     product first, then its incident edges' blocks in that order;
 *   - every dot product and the cost: thread t of 256 adds entries t, t + 256, ...
 *     in ascending order; the 64 lanes of a wave by the xor butterfly 32, ..., 1;
 *     the four waves as ((w0 + w1) + w2) + w3.
 * Nothing outside the problem enters an order (not n_problems, max_nodes,
 * max_edges or the other problems): a problem gets the same bits alone and in any
 * batch, run after run. poses_out (P*max_nodes*12) may be poses. costs: P x 2
 * (initial, final); iterations: P, the LM iterations each problem began;
 * cg_iterations: P, the matrix-vector products of the whole run; each may be NULL.
 * max_iterations == 0: the poses keep their bits and both costs are equal. A
 * problem with a value that is not finite in a node pose, or within its count in
 * edge_Z or edge_info, or whose first cost is not finite, is not iterated on: its
 * poses keep their bits, its costs are NaN, its iteration counts 0, and the other
 * problems get what they get alone; whatever lies beyond the counts is not read.
 * SVO_ERR_ARG (nothing launched, nothing written): sizes or counts out of range, a
 * required pointer NULL, max_iterations outside 0 .. SVO_PG_MAX_ITERATIONS, max_cg
 * outside 1 .. SVO_PG_MAX_CG (the bounds that keep a launch finite), an edge
 * within its count with an index outside 0 .. n_nodes - 1 or with i == j.
 * The launch uses 137 KB of LDS per workgroup (the conjugate gradients' vectors
 * and the incidence lists) and, per problem at the caps, 1.8 MB of scratch beside
 * its inputs (720 bytes per edge and 576 per node). */
#define SVO_PG_MAX_NODES 512
#define SVO_PG_MAX_EDGES 2048
#define SVO_PG_MAX_ITERATIONS 200
#define SVO_PG_MAX_CG 4096
int svo_pose_graph_optimize(svo_ctx* ctx, int n_problems, int max_nodes, int max_edges, const int* n_nodes,
                            const int* n_edges, const double* poses, const uint8_t* fixed, const int* edge_ij,
                            const double* edge_Z, const double* edge_info, double huber_delta, int max_iterations,
                            int max_cg, double* poses_out, double* costs, int* iterations, int* cg_iterations);
/* The test view: the first linearisation at the given poses, nothing moved. cost
 * (P); per edge e (P*max_edges*6), w (P*max_edges), J_i and J_j (P*max_edges*36,
 * row-major); per node its 21 + 6 sums (P*max_nodes*27). Any output may be NULL;
 * entries beyond a problem's counts are left as they were. A problem with a value
 * that is not finite still returns what the arithmetic gives. */
int svo_pose_graph_linearize(svo_ctx* ctx, int n_problems, int max_nodes, int max_edges, const int* n_nodes,
                             const int* n_edges, const double* poses, const uint8_t* fixed, const int* edge_ij,
                             const double* edge_Z, const double* edge_info, double huber_delta, double* cost,
                             double* edge_e, double* edge_w, double* edge_Ji, double* edge_Jj, double* node_sums);
/* svo_pose_graph_optimize's launch timed with HIP events: reps launches after one
 * warm-up, each from `poses` (which stay as they are) -> ms per whole launch.
 * iterations / cg_iterations (P each, may be NULL): the last launch's counts.
 * SVO_ERR_ARG in addition: nothing to run, reps <= 0, ms NULL. */
int svo_pose_graph_time(svo_ctx* ctx, int n_problems, int max_nodes, int max_edges, const int* n_nodes,
                        const int* n_edges, const double* poses, const uint8_t* fixed, const int* edge_ij,
                        const double* edge_Z, const double* edge_info, double huber_delta, int max_iterations,
                        int max_cg, int reps, double* ms, int* iterations, int* cg_iterations);
/* Z = T_j T_i^-1 (12 doubles each), the measurement an edge (i, j) holds when the
 * two poses agree with it: built with the solver's own arithmetic, so such an
 * edge's error is zero to rounding. Host only; -1 on a NULL argument. */
int svo_pose_graph_edge(const double* Ti, const double* Tj, double* Z);

/* ------------------------------------------------------------ windowed bundle adjustment
 * Poses and points together: the back end the reference promises (Map::run's
 * "TODO optimization part here", R:src/map.cpp) and never builds. P problems,
 * each with up to max_cams <= SVO_BA_MAX_CAMS cameras (poses: P*max_cams*12
 * doubles, world -> camera as above; fixed: P*max_cams bytes, non-zero = held
 * constant), up to max_points points (P*max_points*3 doubles) and up to max_obs
 * monocular observations in any order (obs_cam / obs_point: indices within the
 * problem, obs_xy: 2 floats). n_cams / n_points / n_obs: P counts each, or NULL
 * = the maximum. Residual, Huber weight, cost and the Pz <= 0 rule per
 * observation are those of svo_reprojection_jacobians. A camera may observe a
 * point more than once: every observation enters the sums (one W_ij per pair),
 * and together they count as one camera. A point seen by fewer than two distinct
 * cameras in front of it is held constant (its observations still constrain
 * their cameras; two observations by one camera give no depth), so is a point
 * whose damped 3x3 block is not positive definite (for that iteration); a free
 * camera with no observation in front of it is treated as fixed. Every stage runs
 * on the device with a fixed summation order: the results do not depend on the
 * order of the observations beyond a stable sort by (point, camera), and two
 * runs give the same bits. SVO_ERR_ARG (nothing written): sizes or counts out of
 * range, max_cams above SVO_BA_MAX_CAMS, an observation naming a camera or point
 * outside its problem, NULL where data is required. */
#define SVO_BA_MAX_CAMS 16
/* Levenberg-Marquardt (svo_refine_poses' control: lambda from 1e-4, x0.1 down to
 * 1e-12 on success, x10 on failure up to 1e16, the same stopping rules), per
 * problem. poses, points: in/out. costs: P x 2 (initial, final), iterations: P
 * (LM iterations each problem began: one that ends because the reduced system
 * stays not positive definite up to lambda = 1e16, or on the step-size rule,
 * counts like one that ends in a verdict); both may be NULL. Values that are not
 * finite are not an error (the call returns SVO_OK) and stay within their
 * problem: a problem with a NaN or an infinity among its poses, points or
 * observations (within its counts), or whose initial cost is not finite, is not
 * iterated on. Its poses and points come back with the bits they came with, both
 * its costs are NaN and its iteration count is 0; the other problems of the batch
 * get what they get alone. */
int svo_bundle_adjust(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs, const int* n_cams,
                      const int* n_points, const int* n_obs, double* poses, const uint8_t* fixed, double* points,
                      const int* obs_cam, const int* obs_point, const float* obs_xy, const double K[9],
                      double huber_delta, int max_iterations, double* costs, int* iterations);
/* One linearisation and one solve at damping lambda, stage by stage (any output
 * may be NULL). Per camera U (P*max_cams*21, upper triangle of sum w Jc^T Jc,
 * row-major) and gc (6); per point V (P*max_points*6, upper triangle of sum w
 * Jp^T Jp, Jp = Jc[:, :3] R) and gp (3); cost (P). The reduced system over the
 * free cameras in index order, n = 6 n_free[p]: S (P x 6 max_cams x 6 max_cams,
 * row-major, the leading n x n block, zero elsewhere) = U + lambda diag U - sum_i
 * W_ij V*_i^-1 W_ik^T and b (P x 6 max_cams) = -gc + sum_i W_ij V*_i^-1 gp_i. The
 * step: dc (P*max_cams*6, zero for cameras outside the reduced system), dp
 * (P*max_points*3, zero for constant points); status (P): 1 = S not positive
 * definite (dc and dp are zero; S and b are returned all the same). Values that
 * are not finite are not looked for here: they give what IEEE arithmetic gives,
 * within their problem. */
int svo_ba_linearize(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs, const int* n_cams,
                     const int* n_points, const int* n_obs, const double* poses, const uint8_t* fixed,
                     const double* points, const int* obs_cam, const int* obs_point, const float* obs_xy,
                     const double K[9], double huber_delta, double lambda, double* U, double* gc, double* V,
                     double* gp, double* cost, double* S, double* b, double* dc, double* dp, int* n_free,
                     int* status);
/* Stereo observations: svo_bundle_adjust / svo_ba_linearize with the right
 * image's column per observation, obs_ur (P*max_obs floats), of a rectified pair
 * whose right camera's centre lies at +baseline on the left camera's x axis.
 * With P = R X + t an observation with obs_ur >= 0 has a third residual
 *   r2 = fx (Px - baseline) / Pz + cx - obs_ur
 * with the pose-Jacobian row (left perturbation, xr = (Px - baseline) / Pz)
 *   [fx/Pz, 0, -fx xr/Pz, -fx xr y, fx (1 + xr x), -fx y]
 * and the point-Jacobian row Jc[2, :3] R. In every sum its terms follow the two
 * left rows' (U, gc, V, gp, W_ij stay 6x6, 6, 3x3, 3 and 6x3). The Huber weight and
 * the cost take the norm of the residual the observation has: 3 components for
 * a stereo observation, 2 for a monocular one. obs_ur < 0 marks a monocular
 * observation (a measured column is never negative): it is evaluated exactly as
 * by the monocular entries, so a call whose obs_ur are all negative returns their
 * bits. The Pz <= 0 rule is unchanged (such an observation contributes nothing
 * and counts nothing). A stereo observation in front of its camera counts as two
 * views of its point: within a (point, camera) run of duplicates the count is
 * one, plus one if any observation of the run is stereo, so a point with a single
 * stereo observation is free. Every other rule above holds as it stands (positive
 * definiteness, a free camera without observations, duplicates summed into one
 * W_ij, fixed summation order). svo_bundle_adjust_stereo's scan for values that
 * are not finite covers obs_ur within a problem's counts. SVO_ERR_ARG (nothing
 * written) in addition: obs_ur NULL; baseline not finite or <= 0. */
int svo_bundle_adjust_stereo(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs,
                             const int* n_cams, const int* n_points, const int* n_obs, double* poses,
                             const uint8_t* fixed, double* points, const int* obs_cam, const int* obs_point,
                             const float* obs_xy, const float* obs_ur, double baseline, const double K[9],
                             double huber_delta, int max_iterations, double* costs, int* iterations);
int svo_ba_linearize_stereo(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs,
                            const int* n_cams, const int* n_points, const int* n_obs, const double* poses,
                            const uint8_t* fixed, const double* points, const int* obs_cam, const int* obs_point,
                            const float* obs_xy, const float* obs_ur, double baseline, const double K[9],
                            double huber_delta, double lambda, double* U, double* gc, double* V, double* gp,
                            double* cost, double* S, double* b, double* dc, double* dp, int* n_free, int* status);
/* The staging order of one problem's observations (host code, no GPU): the
 * stable sort by (point, camera). order[k] = index of the k-th staged
 * observation; pt_off (n_points + 1): point i owns staged positions
 * [pt_off[i], pt_off[i + 1]); cam_idx[cam_off[j] .. cam_off[j + 1]) (cam_off:
 * n_cams + 1): camera j's staged positions, ascending. */
int svo_ba_sort_observations(const int* obs_cam, const int* obs_point, int n_obs, int n_cams, int n_points,
                             int* order, int* pt_off, int* cam_off, int* cam_idx);
/* The same staging on the device, from observations that arrive as n_cams lists
 * per problem, one per camera, each with strictly increasing point ids (the
 * batched front end's feature lists): ids (P*n_cams*cap), xy (P*n_cams*cap*2),
 * counts (P*n_cams, 0 .. cap). The (point, camera) order is then a merge of
 * sorted lists, found by binary searches without a sort or an atomic. Outputs
 * per problem, strides max_obs = max_points = n_cams*cap, any may be NULL: what
 * svo_ba_sort_observations gives for the same observations listed camera by
 * camera with the points numbered by ascending id -- ocam / oxy (the staged
 * observations' cameras and pixels), pt_off (P*(n_cams*cap + 1), n_obs behind
 * the last point), cam_off (P*(n_cams + 1)), cam_idx -- plus cam_pt (the point of
 * the observation cam_idx names), pt_id (each point's id), n_points and n_obs
 * (P). Zero behind a problem's last observation / point. SVO_ERR_ARG (nothing
 * written): n_cams outside 1 .. SVO_BA_MAX_CAMS, a count outside 0 .. cap, a
 * negative id, a list that is not strictly increasing. */
int svo_ba_stage_lists(svo_ctx* ctx, int n_problems, int n_cams, int cap, const int* counts, const int* ids,
                       const float* xy, int* ocam, float* oxy, int* pt_off, int* cam_off, int* cam_idx, int* cam_pt,
                       int* pt_id, int* n_points, int* n_obs);
/* svo_ba_stage_lists with the right column beside each pixel: ur (P*n_cams*cap,
 * in the lists' order, < 0 = none) comes back as our (P*n_cams*cap, nullable) in
 * staged order, as oxy does; everything else is svo_ba_stage_lists'. SVO_ERR_ARG
 * in addition: ur NULL. */
int svo_ba_stage_lists_stereo(svo_ctx* ctx, int n_problems, int n_cams, int cap, const int* counts, const int* ids,
                              const float* xy, const float* ur, int* ocam, float* oxy, float* our, int* pt_off,
                              int* cam_off, int* cam_idx, int* cam_pt, int* pt_id, int* n_points, int* n_obs);
/* The device staging chain (svo_ba_stage_lists' kernels into a block sized from
 * the staged counts, as svo_frontend_bundle_adjust runs it) timed with HIP
 * events: reps runs after one warm-up, ms per chain (ms_device). Beside it what
 * the host's staging of the same lists costs, wall time: the lists' download
 * (ms_host_readback) and svo_bundle_adjust's sort and uploads (ms_host_stage). */
int svo_ba_time_staging(svo_ctx* ctx, int n_problems, int n_cams, int cap, const int* counts, const int* ids,
                        const float* xy, int reps, double* ms_device, double* ms_host_readback,
                        double* ms_host_stage);
/* One LM iteration's launch chain (linearise, eliminate, solve, update, trial
 * cost) timed with HIP events: reps runs after one warm-up, ms per iteration. */
int svo_ba_time_iteration(svo_ctx* ctx, int n_problems, int max_cams, int max_points, int max_obs, const int* n_cams,
                          const int* n_points, const int* n_obs, const double* poses, const uint8_t* fixed,
                          const double* points, const int* obs_cam, const int* obs_point, const float* obs_xy,
                          const double K[9], double huber_delta, double lambda, int reps, double* ms_per_iteration);

/* ------------------------------------------------------------ batched front end
 * The reference's per-frame loop (Tracking::startStereo, R:src/tracking.cpp:232-276:
 * trackFrames -> calculatePose -> keyframe extractFeatures + findLeftFeaturesInRight
 * + triangulateNewMapPoints) for n_seq independent stereo sequences advanced in
 * lockstep: every kernel launch covers the whole batch, all state (left / right
 * pyramids, features, map points) stays in HBM, and only the RANSAC minimal solver
 * (EPnP) and the final SQPnP-objective fit run on the host between GPU launches.
 * A keyframe's new features are the first (n_features - n) masked FAST corners,
 * matched in the right image (stereo LK), filtered (status, |yR - yL| <
 * y_threshold), triangulated with P_left / P_right (z > 0) and moved to the world
 * frame by the frame's estimated pose. Which frames are keyframes: keyframe_rule
 * SVO_KF_EVERY (every frame, topping the set up to n_features: the benchmark's
 * upper bound) or SVO_KF_REFERENCE (Tracking::nextFrame, R:src/tracking.cpp:68-69:
 * frame 0, and a frame whose predecessor was no keyframe and kept fewer than
 * features_to_track features; it takes every masked corner, n_features being
 * the feature capacity). */
#define SVO_KF_EVERY 0
#define SVO_KF_REFERENCE 1
typedef struct svo_frontend svo_frontend;

typedef struct svo_frontend_config {
    int width, height;      /* frame size */
    int n_seq;              /* sequences per batch */
    int n_frames;           /* frames kept resident per sequence. It also sizes the map:
                               CAP * (n_frames + 2) points per sequence, CAP = n_features
                               rounded up to 64. A resident run never fills it; a streamed
                               ring (queue_frames, e.g. n_frames 4) does on a long run, and
                               the keyframe that would overflow it first reclaims the slots
                               of features no longer tracked (the live points move to the
                               front, in order), so a run of any length follows the same
                               loop. svo_frontend_map_points reads live features only. */
    int n_features;         /* features kept per frame (top-up target), e.g. 2000 */
    int max_level;          /* LK maxLevel, R:src/tracking.cpp:163 -> 3 */
    int win;                /* LK window, :163 -> 21 */
    int lk_max_count;       /* :157 -> 50 */
    double lk_epsilon;      /* :157 -> 1e-3 */
    double min_eig;         /* OpenCV default 1e-4 */
    int lk_flags;           /* :164 -> SVO_LK_GET_MIN_EIGENVALS */
    int fast_threshold;     /* R:configs/config.yaml:30 -> 20 */
    int fast_nonmax;        /* R:include/config_reader.h:37 -> 1 */
    float mask_half;        /* R:src/tracking.cpp:78 -> 10 */
    int bucket_size;        /* 0 = no bucketing (the reference never calls it) */
    int per_bucket;
    int pnp_iterations;     /* R:src/tracking.cpp:195 -> 100 */
    float pnp_reproj;       /* -> 8.0 */
    double pnp_confidence;  /* -> 0.999 */
    double K[9];            /* camera matrix (float-rounded, as the Matx33f K) */
    int host_threads;       /* RANSAC host threads; 0 = auto */
    int timing;             /* 1 = per-phase HIP events; 2 = only LK, pyramid, FAST; 3 = only LK */
    int keyframe_rule;      /* SVO_KF_EVERY (default) or SVO_KF_REFERENCE */
    int features_to_track;  /* SVO_KF_REFERENCE threshold, R:configs/config.yaml:15 -> 70 */
    /* stereo keyframe path (R:src/tracking.cpp:94-152) */
    float P_left[12];       /* mProjectionMatrixLeft (KITTI calib P2, R:src/main.cpp:25-28), row-major 3x4 */
    float P_right[12];      /* mProjectionMatrixRight (P3, :29-32) */
    float y_threshold;      /* R:configs/config.yaml:16 -> 40 */
    /* (the next four are ignored once svo_frontend_set_stereo_matcher is called) */
    int stereo_win;         /* R:src/tracking.cpp:104 -> 11 */
    int stereo_max_level;   /* -> 3 */
    int stereo_max_count;   /* :97 -> 30 */
    double stereo_epsilon;  /* -> 1e-3 */
    /* keyframe detector (R:src/tracking.cpp:33-57): 0 = FAST(fast_threshold,
     * fast_nonmax); 1 = cv::ORB with `orb` (the shipped config, use_orb: 1,
     * R:configs/config.yaml:19-27) -- ORB keypoints (level-0 coordinates, level
     * order) replace FAST's as the keyframe's candidates; detected only on the
     * steps where some sequence takes a keyframe, through the serial keyframe path
     * (no speculative stereo LK, no FAST pre-detection, no bucketing) */
    int use_orb;
    svo_orb_params orb;
} svo_frontend_config;

typedef struct svo_frontend_stats {
    int64_t lk_iterations;  /* GN iterations this step (all sequences, levels) */
    int64_t tracked;        /* features with status 1 after LK */
    int64_t inliers;        /* PnP inliers kept */
    int64_t added;          /* new features from the keyframe top-up */
    int64_t features;       /* features after the step */
    int64_t hypotheses;     /* RANSAC hypotheses scored on the GPU */
    double host_ms_hyp;     /* host wall time generating hypotheses (EPnP) */
    double host_ms_fit;     /* host wall time in the final fits */
    double host_ms_wait;    /* host wall time blocked on the GPU (= the three waits below) */
    int64_t keyframes;      /* sequences whose frame was a keyframe this step */
    /* per-step diagnostics (what a slow step spent its time on) */
    double host_ms_wait_post;   /* waiting for the post-LK results (LK + compaction) */
    double host_ms_wait_score;  /* waiting for the RANSAC scoring launches, all rounds */
    double host_ms_wait_kf;     /* waiting for the keyframe at the step's end */
    double host_ms_enqueue;     /* issuing the step's launches (incl. the next front half) */
    double host_ms_step;        /* the whole call */
    int64_t ransac_rounds;      /* host <-> GPU RANSAC rounds (chunks) */
    int64_t max_hypotheses;     /* most hypotheses any one sequence scored */
    int64_t serial_keyframe;    /* 1: the speculative stereo LK missed, serial keyframe ran */
    int64_t full_copy;          /* 1: the full point copy was waited for (long RANSAC / n <= 5) */
    int64_t kf_overflow;        /* SVO_KF_REFERENCE: masked corners a keyframe left out for
                                   lack of capacity (n_features); 0 = every corner taken,
                                   as extractFeatures (R:src/tracking.cpp:74-92); with use_orb
                                   it includes the ORB keypoints its detector dropped at the
                                   candidate capacity */
    double host_ms_orb;         /* use_orb: the keyframe's ORB detection (device stages and the
                                   host's retainBest, synchronous on the FAST stream) */
    int64_t spec_margin;        /* the speculative stereo LK's margin over the expected top-up
                                   (spec_margin + the last step's largest RANSAC / LK losses) */
} svo_frontend_stats;

int svo_frontend_create(svo_ctx* ctx, const svo_frontend_config* cfg, svo_frontend** out);
void svo_frontend_destroy(svo_frontend* fe);
/* Stereo pair t of sequence seq (left / right grey, same stride): level-0 uploads
 * (H2D, untimed; R:include/async_image_loader.h:57-69 delivers the pair). */
int svo_frontend_set_frame(svo_frontend* fe, int seq, int t, const uint8_t* left, const uint8_t* right,
                           int stride);
/* Same from BGR 8UC3 frames (svo_image_upload_bgr's conversion). */
int svo_frontend_set_frame_bgr(svo_frontend* fe, int seq, int t, const uint8_t* left_bgr,
                               const uint8_t* right_bgr, int stride);
/* Raw frames: from this call on svo_frontend_set_frame, svo_frontend_set_frame_bgr
 * and svo_frontend_queue_frames take the cameras' raw frames (the maps' raw_w x
 * raw_h, which may differ from the config's size: stride checks and copies use it)
 * and level 0 of every slot is cv::remap of them with that eye's maps (svo_remap's
 * rule; BGR: grey taps), in place of cv::initUndistortRectifyMap + cv::remap on
 * the host. The streamed path rectifies where it converted, on the upload stream
 * with the same events; the resident path stages the raw pair first (raw frames
 * are not kept). Nothing downstream of level 0 changes; a front end that never
 * calls this launches exactly what it did. Once, before the first set_frame,
 * queue_frames or init; the maps must outlive the front end. SVO_ERR_ARG: called
 * later or twice, maps whose w x h is not the config's, eyes of different raw
 * sizes, null arguments. */
int svo_frontend_set_rectification(svo_frontend* fe, const svo_rect_maps* left, const svo_rect_maps* right);
/* Row SAD as the keyframe's stereo match: from this call on every stereo match of
 * the front end (the speculative one and the serial keyframe's) is
 * svo_stereo_match_rows' rule with these parameters in place of the stereo LK, on
 * the same stream behind the same events, into the same buffers. The frames must
 * be rectified (a match is looked for on the left point's row only; y_threshold
 * always passes). stereo_win, stereo_max_level, stereo_max_count and
 * stereo_epsilon of the configuration are ignored while the matcher is set.
 * Nothing else changes; a front end that never calls this launches exactly what
 * it did. Once, before the first set_frame, queue_frames or init. SVO_ERR_ARG:
 * called later or twice, null arguments, parameters svo_stereo_match_rows rejects. */
int svo_frontend_set_stereo_matcher(svo_frontend* fe, const svo_stereo_rows_params* params);
/* Streamed frames (R:include/async_image_loader.h:36-69: the loader hands each
 * stereo pair to Tracking as it arrives; here a whole step's worth at once):
 * queue frame t of every sequence -- left[s] / right[s] (grey, or BGR 8UC3 when
 * bgr != 0: cv::cvtColor(BGR2GRAY) on the device), rows `stride` bytes apart --
 * as asynchronous H2D copies on the front end's upload stream into ring slot
 * t % n_frames, converted into level 0 there; frame t's pyramid builds wait for
 * it. Returns at once: the host buffers must stay untouched until
 * svo_frontend_upload_wait(fe, t) (page-locked memory, svo_pinned_alloc, gives
 * full PCIe rate; sequences whose buffers follow each other in memory go in one
 * copy). Ring discipline (n_frames >= 4): before init, any frame; after it,
 * frame t is queued before step t - 2 is called (t >= last step + 3) and no
 * earlier than step t - n_frames + 1 returned (t <= last step + n_frames - 1):
 * a loop queues frames 0 .. 2, calls init(0), then queue(t + 2), step(t). A frame
 * at or before the last step restarts the loop (everything queued is finished and
 * forgotten; queue frames t0 .. t0 + 2 and init(t0) again). set_frame(seq, t)
 * after streaming makes slot t hold frame t, resident. The copy into a slot waits
 * on the device for the last read of the slot's previous frame. */
int svo_frontend_queue_frames(svo_frontend* fe, int t, const uint8_t* const* left, const uint8_t* const* right,
                              int stride, int bgr);
int svo_frontend_upload_wait(svo_frontend* fe, int t);
int svo_pinned_alloc(size_t bytes, void** out);
void svo_pinned_free(void* p);
/* Build every resident frame's pyramid now (else each step builds its own). */
int svo_frontend_prebuild_pyramids(svo_frontend* fe);
/* First keyframe: FAST (+bucket) on frame t0 of every sequence, map points. */
int svo_frontend_init(svo_frontend* fe, int t0);
/* One step: frame t-1 -> t for every sequence (pyramid of t, temporal LK,
 * compaction, PnP RANSAC, outlier removal, masked FAST top-up). */
int svo_frontend_step(svo_frontend* fe, int t, svo_frontend_stats* stats);
/* Wait for every stream of the front end (a step returns with the next frame's
 * pyramid and the pose statistics still running) and finish the pose fits. */
int svo_frontend_synchronize(svo_frontend* fe);
int svo_frontend_pose(svo_frontend* fe, int seq, double rvec[3], double tvec[3]);
int svo_frontend_features(svo_frontend* fe, int seq, float* xy, int cap, int* n);
/* World positions (MapPoint::mWorldPos) of the current features' map points, in
 * feature order (synchronises the front end first). */
int svo_frontend_map_points(svo_frontend* fe, int seq, double* xyz, int cap, int* n);
/* The observation window: the back end's input, kept on the device. Each sequence
 * gets a ring of `window` (1 .. SVO_BA_MAX_CAMS) slots; svo_frontend_init and
 * every svo_frontend_step record the frame's feature list as the step leaves it
 * (svo_frontend_features' points with their map ids) in stream order, without a
 * host wait, and the frame's pose (world -> camera, R row-major and t: 12 doubles,
 * the solvePnPRansac model [R(rvec) | tvec]; the identity for the init frame and
 * for a frame without a model) once its final fit lands. A map reclaim (n_frames
 * above) renumbers a sequence's map ids: the slots recorded before it are no
 * longer valid, so that sequence's window shortens to the frames since the
 * reclaim and grows again. Before svo_frontend_init; SVO_ERR_ARG afterwards, or
 * with `window` out of range. A front end that never calls it runs exactly as
 * before: no kernel is added to its step. */
int svo_frontend_window_enable(svo_frontend* fe, int window);
/* The valid slots of sequence seq, oldest first (synchronises the front end
 * first): n_frames of them; frame_t (W = the enabled window), poses (W*12),
 * counts (W), ids (W*cap: map ids, strictly increasing per frame), xy (W*cap*2);
 * a frame with more than cap features is cut to cap. Any output may be NULL. */
int svo_frontend_window(svo_frontend* fe, int seq, int cap, int* n_frames, int* frame_t, double* poses, int* counts,
                        int* ids, float* xy);
/* Windowed bundle adjustment (svo_bundle_adjust's Levenberg-Marquardt, config K)
 * of every sequence from its own window, without leaving the device: the
 * observations are staged from the ring (svo_ba_stage_lists' chain), the points
 * gathered from the map by id, the oldest n_fixed valid frames held constant.
 * Refined points go back into the map, so the next step's PnP sees them; refined
 * poses go back into the window (svo_frontend_pose keeps reporting the PnP fit).
 * Host <-> device traffic: the staged counts, and the control numbers per problem
 * and iteration that svo_bundle_adjust exchanges. costs: S*2 (initial, final),
 * iterations: S, sizes: S*3 (frames, points, observations); any may be NULL.
 * The results equal svo_bundle_adjust's, bit for bit, on the same window given
 * frame by frame with the points numbered by ascending map id and max_points /
 * max_obs the batch's largest counts (finite values: the window is never read
 * on the host, so of svo_bundle_adjust's rule for values that are not finite
 * only "initial cost not finite" applies). A sequence with an empty or one-frame window
 * is a valid problem in which nothing is free: it comes back unchanged.
 * Synchronises the front end first. SVO_ERR_ARG: window not enabled, n_fixed < 0,
 * max_iterations < 0. */
int svo_frontend_bundle_adjust(svo_frontend* fe, int n_fixed, double huber_delta, int max_iterations, double* costs,
                               int* iterations, int* sizes);
/* The stereo window: svo_frontend_window_enable, and the ring also keeps one
 * float per feature and slot, the right image's column of the stereo match
 * (findLeftFeaturesInRight's LK) that created the feature, in the frame that
 * created it, and -1 in every later frame that tracks it (unless
 * svo_frontend_set_stereo_tracking, below, matches it there); the init frame's
 * features all carry theirs. With the plain svo_frontend_window_enable none of
 * this is allocated or written. SVO_ERR_ARG in addition: the configuration's
 * P_right gives no baseline -P_right[3] / P_right[0] > 0. */
int svo_frontend_window_enable_stereo(svo_frontend* fe, int window);
/* The right columns of sequence seq's valid slots in svo_frontend_window's order
 * and with its cut: ur (W*cap). SVO_ERR_ARG: no stereo window enabled. */
int svo_frontend_window_right(svo_frontend* fe, int seq, int cap, float* ur);
/* svo_frontend_bundle_adjust with the stereo term (svo_bundle_adjust_stereo) on
 * the ring's right columns, baseline = -P_right[3] / P_right[0] of the
 * configuration: a point created at the newest frame, which one camera sees, is
 * free. The results equal svo_bundle_adjust_stereo's, bit for bit, on the same
 * window built on the host from svo_frontend_window and
 * svo_frontend_window_right. SVO_ERR_ARG in addition: no stereo window enabled. */
int svo_frontend_bundle_adjust_stereo(svo_frontend* fe, int n_fixed, double huber_delta, int max_iterations,
                                      double* costs, int* iterations, int* sizes);
/* svo_refine_poses_stereo for the newest frame of every sequence, from the window
 * on the device (opt-in; needs svo_frontend_window_enable or _enable_stereo). Like
 * svo_frontend_bundle_adjust it calls svo_frontend_synchronize first and uses the
 * slots of the map's current epoch. Per sequence the problem is the newest valid
 * slot: its pixels, its right columns (a plain window: every observation
 * monocular), its pose, the map points its ids name (read in place, no gather
 * pass) and baseline = -P_right[3] / P_right[0]. The refined pose is written into
 * that slot's pose, where svo_frontend_bundle_adjust writes poses, and nowhere
 * else: the map, svo_frontend_pose and every later svo_frontend_step are unchanged
 * to the bit. The results equal svo_refine_poses_stereo's, bit for bit, on the
 * same arrays read back beforehand. A sequence without a valid slot is the empty
 * problem (cost 0, one iteration, nothing written). costs: S x 2, iterations: S,
 * counts: S (the observations used); any may be NULL; one download brings the
 * three. SVO_ERR_ARG: no window enabled; max_iterations outside 0 ..
 * SVO_REFINE_MAX_ITERATIONS; a plain window whose P_right gives no baseline > 0
 * still runs (no observation uses it). */
int svo_frontend_refine_poses(svo_frontend* fe, double huber_delta, int max_iterations, double* costs,
                              int* iterations, int* counts);
/* Stereo columns for tracked features (opt-in; RECTIFIED frames): from this call
 * on every recorded frame also matches its tracked features -- the first
 * nA - added of the list the step leaves -- between level 0 of its own left and
 * right images with svo_stereo_match_rows_guided, and the ring's right column of
 * a tracked feature is the matched column where the status is 1, -1 otherwise
 * (the frame's new features keep the column of the match that created them).
 * The prior is svo_stereo_row_priors against the window's slot of frame t - 1,
 * if that slot holds frame t - 1 and its epoch is the map's current one;
 * otherwise (after a map reclaim, a restart) no feature has a prior. guide == 0
 * skips the lookup: the full range for every feature. Features, poses, map
 * points, counts and the window's xy / ids are those of a front end that never
 * made the call, bit for bit; the match runs behind the keyframe beside the
 * record, off the step's critical path, whichever matcher the keyframe uses.
 * SVO_ERR_ARG: no stereo window enabled, called after svo_frontend_init or twice,
 * null arguments, parameters svo_stereo_match_rows rejects, guide outside 0..15. */
int svo_frontend_set_stereo_tracking(svo_frontend* fe, const svo_stereo_rows_params* params, int guide);
/* The place memory (opt-in; the rules: DESIGN.md section 3e): what ties a sequence
 * that lost its features and rebuilt them in a new world frame back to the map it
 * had. svo_frontend_init records frame t0 and every svo_frontend_step(t) with
 * (t - t0) % every == 0 records frame t, in stream order behind the step's
 * keyframe, without a host wait: every feature of the list the step leaves is
 * described at octave 0 of the frame's own level-0 left image (the descriptor of
 * svo_orb_compute with one level: cx = cvRound(x), cy = cvRound(y), moments on the
 * frame, samples on its 7-tap blur, validity border reach), and the valid ones, in
 * list order, go to slot k % slots of the sequence's ring (k: records since init)
 * with their 32 descriptor bytes, their pixels and their map points' world
 * positions: the f64 bits the map holds once the frame's own pose has moved the
 * frame's new points to the world frame (copied behind the next step's post-LK or
 * the next synchronize, ahead of anything that could renumber or refine them). A
 * record keeps no map id: a later map reclaim or bundle adjustment leaves it as
 * it is. Device memory: per sequence and slot CAP * (32 + 8 + 24) bytes plus a
 * count, CAP = n_features rounded up to 64; and once per front end, per sequence,
 * one blurred frame (height rows of the width rounded up to 64), CAP * (32 + 1 + 4)
 * bytes of work and CAP * (32 + 8) bytes of query set. With streamed frames the
 * upload into an image slot waits for the record that reads it. patch_size: odd, in
 * [5, 31]; pattern_xy as svo_orb_compute's (NULL: svo_orb_default_pattern).
 * Features, poses and map points are those of a front end that never made the
 * call, bit for bit, and a front end that never makes it launches nothing more.
 * SVO_ERR_ARG: called after svo_frontend_init or twice, slots outside
 * 1 .. SVO_PLACES_MAX_SLOTS, every < 1, a patch_size or pattern svo_orb_compute rejects. */
#define SVO_PLACES_MAX_SLOTS 16
int svo_frontend_places_enable(svo_frontend* fe, int slots, int every, int patch_size, const int8_t* pattern_xy);
/* Test view of one record (synchronises the front end first): *frame_t (-1: the
 * slot holds none, *n = 0), *n entries, and the first min(*n, cap) of desc (32
 * bytes each), xy (2 floats), xyz (3 doubles). Any output may be NULL.
 * SVO_ERR_ARG: no place memory enabled, seq or slot out of range, cap < 0. */
int svo_frontend_place(svo_frontend* fe, int seq, int slot, int* frame_t, int* n, uint8_t* desc, float* xy,
                       double* xyz, int cap);
/* Relocalise the frame of the last step (or of init) against the records whose
 * frame lies in [t_lo, t_hi], for the sequences with which[s] != 0 (NULL: all);
 * the outputs of the others are not touched. Synchronises the front end. The query
 * set is that frame's current feature list, described, valid, compacted as a
 * record is. Per searched record: svo_match_hamming in both directions and
 * svo_match_filter's rule with ratio_pct and (cross_check != 0) the cross-check,
 * for every (sequence, record) in one launch per direction and one of the filter.
 * The best record has the most pairs, ties to the oldest frame; with fewer than
 * max(min_pairs, 4) pairs there is no result. Otherwise svo_solve_pnp_ransac with
 * the configuration's K, pnp_iterations, pnp_reproj, pnp_confidence on the pairs in
 * ascending query index (the record's xyz, the query's xy): [R(rvec) | tvec] maps
 * the record's world to the camera. Per sequence s: frame_t[s] the best record's
 * frame (-1: no result), n_pairs[s] the best record's pair count (also when it
 * gave no result; 0 with nothing searched), n_inliers[s], ok[s] (1: a model),
 * rvec[3s ..], tvec[3s ..] (zero without a model). Optional (NULL to skip):
 * slot_pairs[s*slots + k] the pair count of slot k (-1: not searched), pairs[(s*cap
 * + i)*2 ..] the best record's pairs (query index, record index) in the compacted
 * lists and inliers[s*cap + i] the RANSAC's inliers as indices into them, each cut
 * to cap. SVO_ERR_ARG: no place memory enabled, before svo_frontend_init, a null
 * required output, t_lo > t_hi, ratio_pct < 0, min_pairs < 0, cap < 0. */
int svo_frontend_places_query(svo_frontend* fe, const uint8_t* which, int t_lo, int t_hi, int ratio_pct,
                              int cross_check, int min_pairs, int* frame_t, int* n_pairs, int* n_inliers, int* ok,
                              double* rvec, double* tvec, int* slot_pairs, int* pairs, int* inliers, int cap);
/* Measurement only (tools/places_bench.py): HIP-event times in ms of ms[0] one
 * record (blur, describe, compaction, point copy: the newest record written again
 * from the same inputs, so nothing changes) and ms[1] a query's device half (the
 * query set, both matches, the filter) over every sequence and the records in
 * [t_lo, t_hi]; *n_problems (nullable): the (sequence, record) problems matched.
 * SVO_ERR_ARG in addition to the query's: the last step's frame is not the newest record. */
int svo_frontend_places_time(svo_frontend* fe, int t_lo, int t_hi, int ratio_pct, int cross_check, double ms[2],
                             int* n_problems);
/* The second look at a query's pose, for every sequence
 * with which[s] != 0 (NULL: all) and frame_t[s] >= 0; the outputs of the others
 * are not touched. The record of frame frame_t[s] is projected under [R(rvec + 3s)
 * | tvec + 3s] and matched by svo_match_projected's rules (the configuration's K,
 * the frame's size, params) against the query set of the last step's frame, built
 * as svo_frontend_places_query builds it; all sequences in one launch chain. Then
 * svo_solve_pnp_ransac with the front end's PnP settings on the widened pairs in
 * ascending query index (the record's xyz, the query's xy). Synchronises the front
 * end and writes nothing into it. Per sequence: n_pairs[s], n_inliers[s], ok[s],
 * rvec_out[3s ..], tvec_out[3s ..] (zero without a model; they may alias rvec /
 * tvec); optional pairs[(s*cap + i)*2 ..] = (query index, record index) and
 * inliers[s*cap + i] as the query's, each cut to cap. A sequence whose frame_t is
 * no longer in its ring, or with fewer than 4 pairs, gets ok = 0 (and n_pairs = 0
 * for the former). SVO_ERR_ARG: as the query's, a null frame_t / rvec / tvec, and
 * params svo_match_projected rejects. */
int svo_frontend_places_widen(svo_frontend* fe, const uint8_t* which, const int* frame_t, const double* rvec,
                              const double* tvec, const svo_proj_match_params* params, int* n_pairs, int* n_inliers,
                              int* ok, double* rvec_out, double* tvec_out, int* pairs, int* inliers, int cap);
/* Accumulated per-phase device time (ms) and launch counts since create/reset:
 * phases: 0 pyramid (left + Scharr), 1 lk, 2 post_lk, 3 stereo_lk, 4 pnp_score,
 * 5 tail (keyframe), 6 fast, 7 bucket, 8 append, 9 pyramid_right. Returns the number
 * of phases. */
int svo_frontend_phase_times(svo_frontend* fe, double* ms, int64_t* launches, int cap);
void svo_frontend_reset_times(svo_frontend* fe);
/* The Scharr derivatives (svo_image_scharr_level's layout) of frame t of sequence
 * seq as the front end's fused pyrDown + Scharr pass built them; frame t must be
 * one of the last three frames whose pyramid was built (the derivative pyramids
 * are triple-buffered): after svo_frontend_init(t0) frame t0, after
 * svo_frontend_step(t) frames t and t + 1. Synchronises the front end first. */
int svo_frontend_scharr_level(svo_frontend* fe, int seq, int t, int level, int16_t* ix, int16_t* iy, int stride);
/* Level `level` of frame t's left (right = 0) or right (right = 1) pyramid with
 * its stored REFLECT_101 border: (h + 2 * SVO_PYR_PAD) rows of (w + 2 *
 * SVO_PYR_PAD) bytes at `stride`, pixel (0, 0) of the level at row / column
 * SVO_PYR_PAD (the LK kernels read the border instead of testing coordinates).
 * Same frames as svo_frontend_scharr_level (right: the frame of the last step or
 * init). Synchronises the front end first. */
#define SVO_PYR_PAD 32
int svo_frontend_pyramid_level(svo_frontend* fe, int seq, int t, int right, int level, uint8_t* out, int stride);
/* The pyramid + Scharr launch chain of frame t (every sequence) timed alone on the
 * context stream: reps rebuilds (identical contents) after one warm-up, HIP
 * events around them; ms per chain. Synchronises the front end first. */
int svo_frontend_time_pyramid(svo_frontend* fe, int t, int reps, double* ms_per_launch);
/* The streamed path's level-0 write of the left eye (every sequence) timed alone the
 * same way, from the staging block as the last svo_frontend_queue_frames left it
 * (its stride, grey or BGR) into ring slot t % n_frames: rectify != 0 the
 * rectifying kernel with the left maps, 0 the plain copy / conversion kernel
 * (the staged frames must be at least the config's size). Synchronises the front
 * end first; the slot's image is overwritten. SVO_ERR_ARG: nothing was queued,
 * rectify without svo_frontend_set_rectification. */
int svo_frontend_time_ingest(svo_frontend* fe, int t, int rectify, int reps, double* ms_per_launch);
/* The front end's FAST detection of frame t (every sequence; FAST-9 + cornerScore +
 * NMS without the box mask, i.e. the pre-detection stage: extractFeatures' detector,
 * R:src/tracking.cpp:82) timed alone the same way; ms per launch (row-count reset +
 * detection kernel). Synchronises the front end first; the next step re-detects. */
int svo_frontend_time_fast(svo_frontend* fe, int t, int reps, double* ms_per_launch);

/* Host cores for a front end's RANSAC / pose-fit pool when several ranks (one
 * process per GPU) share a node: this process's allowed CPUs ordered by NUMA
 * node are split among the local ranks, each rank taking its share of the node
 * its GPU sits on (gpu_node[r] = NUMA node of local rank r's GPU, or null to
 * split the whole ordered list by rank). Writes at most cap CPU ids to cpus and
 * their count to n; the sets of distinct local ranks are disjoint whenever the
 * node has at least one CPU per rank. svo_frontend_create pins its pool with
 * this plan (LOCAL_RANK / LOCAL_WORLD_SIZE from the environment, as
 * torch.distributed.run sets them) and sizes it to the set (at most 16). */
int svo_host_cpu_plan(int local_rank, int local_world, const int* gpu_node, int* cpus, int cap, int* n);
/* The CPUs a front end's pool threads are pinned to (empty: not pinned). */
int svo_frontend_host_cpus(svo_frontend* fe, int* cpus, int cap, int* n);
/* The HIP streams a front end runs on (LK, FAST, copies; hipStream_t as void*):
 * the context's, shared by every front end created on it, so a long-lived
 * process that creates and destroys front ends binds one fixed set of hardware
 * queues. */
int svo_frontend_streams(svo_frontend* fe, void** streams, int cap, int* n);
/* Self-test of the front end's host pool (no GPU): `jobs` jobs of changing sizes
 * with primes between them on `threads` threads; *bad = tasks run other than
 * exactly once, or after their job returned (0 when the pool is correct). */
int svo_pool_selftest(int threads, int jobs, int64_t* bad);

#ifdef __cplusplus
}
#endif
#endif /* SVO_GPU_H */
