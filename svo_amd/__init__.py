"""svo_amd -- MI355X-native front end of ikryukov/svo (Python host side).

Thin ctypes layer over the C ABI of ``svo_amd/lib/libsvo_gpu.so``
(``include/svo_gpu.h``). The names mirror the OpenCV calls the reference's
``Tracking`` makes (R: = ikryukov/svo):

=================================  ===========================================
svo_amd                            reference call site
=================================  ===========================================
``Context.image`` (pyramid)         pyramid built inside calcOpticalFlowPyrLK,
                                    R:src/tracking.cpp:101, :160
``FastFeatureDetector.detect``      mDetector->detect(img, kps, mask),
                                    R:src/tracking.cpp:82 (created :54-57)
``Context.mask_boxes``              cv::rectangle(mask, ...), :76-79
``Context.bucket_features``         FeatureSet::bucketingFeatures,
                                    R:src/bucket.cpp:24-68
``Context.calc_optical_flow_pyr_lk``  cv::calcOpticalFlowPyrLK, :101-105, :160-165
``Context.pnp_residuals``           PnPRansacCallback::computeError+findInliers
``Context.solve_pnp_ransac``        cv::solvePnPRansac(..., SQPNP), :191-196
``Context.orb_detect_and_compute``  (not in the reference) cv::ORB::detectAndCompute
``Context.match_hamming``           (not in the reference) BFMatcher::knnMatch(k = 2)
=================================  ===========================================

There is no CPU fallback: every compute call goes through the HIP kernels and
raises ``SvoError`` if the extension or a GPU is missing.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import weakref

import numpy as np

__all__ = [
    "SvoError", "lib", "Context", "Image", "FastFeatureDetector",
    "TERM_COUNT", "TERM_EPS", "LK_USE_INITIAL_FLOW", "LK_GET_MIN_EIGENVALS", "LK_OPENCV_ORDER",
    "lib_path", "Frontend", "FrontendConfig", "FrontendStats",
    "RectMaps", "init_undistort_rectify_map", "remap", "StereoRowsParams", "STEREO_NO_PRIOR",
    "OrbParams", "ORB_DESC_BYTES", "orb_default_pattern", "orb_umax", "match_filter",
]

STEREO_NO_PRIOR = -(2 ** 31)  # SVO_STEREO_NO_PRIOR: a point of the guided row match without a prior

TERM_COUNT = 1
TERM_EPS = 2
LK_USE_INITIAL_FLOW = 4
BA_MAX_CAMS = 16  # SVO_BA_MAX_CAMS: cameras of one bundle adjustment problem
PYR_PAD = 32  # SVO_PYR_PAD: stored border of every pyramid level
LK_GET_MIN_EIGENVALS = 8
# SVO_LK_OPENCV_ORDER (not an OpenCV flag): LK's normal equations summed in OpenCV's
# own float order (its SSE build) instead of exactly -- bit-identical to
# cv::calcOpticalFlowPyrLK's x86 results (oracle ACC_SSE)
LK_OPENCV_ORDER = 0x10000

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path() -> str:
    # SVO_GPU_LIB: another build of the same library (A/B measurements)
    return os.environ.get("SVO_GPU_LIB") or os.path.join(_HERE, "lib", "libsvo_gpu.so")


# Live handles, closed at interpreter exit in dependency order (front ends and
# images before the contexts they were made on): left to __del__, a context can
# go first and its dependants then free into a destroyed context. The cyclic
# collector does the same to objects it frees together (a failed test's traceback
# holds its front end and its context; the weak sets below are cleared before
# their __del__ run), so a context also keeps the native handles of its live
# dependants (Context._deps) and destroys those first when it goes first.
_LIVE = {"frontend": weakref.WeakSet(), "image": weakref.WeakSet(), "maps": weakref.WeakSet(),
         "context": weakref.WeakSet()}


def _close_all():
    for kind in ("frontend", "image", "maps", "context"):
        for obj in list(_LIVE[kind]):
            try:
                obj.close()
            except Exception:
                pass


atexit.register(_close_all)


class SvoError(RuntimeError):
    pass


_LIB = None

_u8p = C.POINTER(C.c_uint8)
_i8p = C.POINTER(C.c_int8)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int)
_u32p = C.POINTER(C.c_uint32)
_vp = C.c_void_p

# (name, restype, argtypes) for every symbol include/svo_gpu.h declares
_SIGS = [
    ("svo_ctx_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("svo_ctx_destroy", None, [_vp]),
    ("svo_last_error", C.c_char_p, [_vp]),
    ("svo_ctx_synchronize", C.c_int, [_vp]),
    ("svo_version", C.c_char_p, []),
    ("svo_image_create", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("svo_image_destroy", None, [_vp, _vp]),
    ("svo_image_upload", C.c_int, [_vp, _vp, _u8p, C.c_int]),
    ("svo_image_upload_bgr", C.c_int, [_vp, _vp, _u8p, C.c_int]),
    ("svo_image_build_pyramid", C.c_int, [_vp, _vp]),
    ("svo_rect_maps_create", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int16),
                                       C.POINTER(C.c_uint16), C.POINTER(_vp)]),
    ("svo_rect_maps_destroy", None, [_vp, _vp]),
    ("svo_init_undistort_rectify_map", C.c_int, [_f64p, _f64p, _f64p, _f64p, C.c_int, C.c_int, C.POINTER(C.c_int16),
                                                 C.POINTER(C.c_uint16)]),
    ("svo_remap", C.c_int, [_vp, _u8p, C.c_int, C.c_int, _vp, _u8p, C.c_int]),
    ("svo_image_upload_raw", C.c_int, [_vp, _vp, _u8p, C.c_int, C.c_int, _vp]),
    ("svo_image_level_size", C.c_int, [_vp, C.c_int, _i32p, _i32p]),
    ("svo_image_download_level", C.c_int, [_vp, _vp, C.c_int, _u8p, C.c_int]),
    ("svo_image_scharr_level", C.c_int, [_vp, _vp, C.c_int, C.POINTER(C.c_int16), C.POINTER(C.c_int16), C.c_int]),
    ("svo_fast_detect", C.c_int, [_vp, _vp, C.c_int, C.c_int, _u8p, _f32p, C.c_int, _i32p]),
    ("svo_orb_detect", C.c_int, [_vp, _vp, _vp, _u8p, _f32p, _i32p, C.c_int, _i32p]),
    ("svo_orb_level", C.c_int, [_vp, _vp, _vp, _u8p, C.c_int, _u8p, _u8p, _i32p, _i32p]),
    ("svo_orb_default_pattern", C.c_int, [C.c_int, _i8p]),
    ("svo_orb_umax", C.c_int, [C.c_int, _i32p, C.c_int, _i32p]),
    ("svo_orb_compute", C.c_int, [_vp, _vp, _vp, _i8p, _f32p, _i32p, C.c_int, _u8p, _f32p, _u8p]),
    ("svo_orb_detect_and_compute", C.c_int, [_vp, _vp, _vp, _u8p, _i8p, _f32p, _i32p, _u8p, _f32p, _u8p, C.c_int,
                                             _i32p]),
    ("svo_orb_blur_level", C.c_int, [_vp, _vp, _vp, C.c_int, _u8p, _i32p, _i32p]),
    ("svo_match_hamming", C.c_int, [_vp, C.c_int, _i32p, _i32p, C.c_int, C.c_int, _u8p, _u8p, _i32p, _i32p]),
    ("svo_match_filter", C.c_int, [_i32p, _i32p, C.c_int, _i32p, C.c_int, C.c_int, _i32p, C.c_int, _i32p]),
    ("svo_match_filter_batch", C.c_int, [_vp, C.c_int, _i32p, _i32p, C.c_int, C.c_int, _i32p, _i32p, _i32p, C.c_int,
                                         _i32p, _i32p]),
    ("svo_orb_describe_time", C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _f64p, _i32p]),
    ("svo_match_hamming_time", C.c_int, [_vp, C.c_int, _i32p, _i32p, C.c_int, C.c_int, _u8p, _u8p, C.c_int, _f64p]),
    ("svo_match_projected", C.c_int, [_vp, C.c_int, _i32p, _i32p, C.c_int, C.c_int, _f64p, _u8p, _f32p, _u8p, _f64p,
                                      _f64p, C.c_int, C.c_int, _vp, _i32p, _i32p, _f32p, _i32p, _i32p]),
    ("svo_match_projected_time", C.c_int, [_vp, C.c_int, _i32p, _i32p, C.c_int, C.c_int, _f64p, _u8p, _f32p, _u8p,
                                           _f64p, _f64p, C.c_int, C.c_int, _vp, C.c_int, _f64p]),
    ("svo_pose_from_rvec", C.c_int, [_f64p, _f64p, _f64p]),
    ("svo_fast_score_map", C.c_int, [_vp, _vp, C.c_int, _u8p, _u8p]),
    ("svo_mask_boxes", C.c_int, [_vp, C.c_int, C.c_int, _f32p, C.c_int, C.c_float, _u8p]),
    ("svo_bucket_features", C.c_int, [_vp, _f32p, _i32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, _f32p, _i32p, C.c_int, _i32p]),
    ("svo_calc_optical_flow_pyr_lk", C.c_int, [_vp, _vp, _vp, _f32p, C.c_int, _f32p, _u8p, _f32p,
                                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_double, C.c_int, C.c_double]),
    ("svo_calc_optical_flow_pyr_lk_split", C.c_int, [_vp, _vp, _vp, _f32p, C.c_int, C.c_int, _f32p, _u8p, _f32p,
                                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     C.c_double, C.c_int, C.c_double]),
    ("svo_lk_last_iterations", C.c_int64, [_vp]),
    ("svo_stereo_match_rows", C.c_int, [_vp, _vp, _vp, _f32p, C.c_int, _vp, _f32p, _u8p, _i32p, _i32p]),
    ("svo_frontend_set_stereo_matcher", C.c_int, [_vp, _vp]),
    ("svo_stereo_match_rows_guided", C.c_int, [_vp, _vp, _vp, _f32p, C.c_int, _vp, _i32p, C.c_int, _f32p, _u8p, _i32p,
                                               _i32p]),
    ("svo_stereo_row_priors", C.c_int, [_vp, _i32p, C.c_int, _i32p, _f32p, _f32p, C.c_int, _i32p]),
    ("svo_frontend_set_stereo_tracking", C.c_int, [_vp, _vp, C.c_int]),
    ("svo_pnp_residuals", C.c_int, [_vp, _f32p, _f32p, C.c_int, _f64p, C.c_int, _f64p, C.c_float,
                                    _f32p, _u8p, _i32p]),
    ("svo_solve_pnp_ransac", C.c_int, [_vp, _f64p, _f32p, C.c_int, _f64p, C.c_int, C.c_float,
                                       C.c_double, _f64p, _f64p, _i32p, _i32p]),
    ("svo_epnp_subsets", C.c_int, [_vp, _f32p, C.c_int, _f64p, C.c_int, _f64p, _i32p]),
    ("svo_solve_pnp_sqpnp", C.c_int, [_f64p, _f32p, C.c_int, _f64p, _f64p, _f64p]),
    ("svo_pnp_score", C.c_int, [_vp, _f32p, _f32p, _i32p, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, _f64p, C.c_float,
                                _u32p, C.c_int, _i32p]),
    ("svo_sqpnp_stats", C.c_int, [_vp, _f32p, _f32p, _i32p, C.c_int, C.c_int, _u32p, C.c_int, _f64p, _f64p]),
    ("svo_sqpnp_fit", C.c_int, [_vp, _f64p, _i32p, _f64p, _f64p, _f64p, _f32p, _i32p, C.c_int, C.c_int, _u32p,
                                C.c_int, C.c_int, _f64p, _f64p]),
    ("svo_trig_pa", C.c_int, [_vp, _f64p, C.c_int, C.c_int, C.c_int, _f64p]),
    ("svo_triangulate_points", C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p, C.c_int, _f32p, _f32p]),
    ("svo_reprojection_jacobians", C.c_int, [_vp, _f64p, _f32p, _i32p, C.c_int, C.c_int, _f64p, _f64p,
                                             C.c_double, _f64p, _f64p, _f64p]),
    ("svo_refine_poses", C.c_int, [_vp, _f64p, _f32p, _i32p, C.c_int, C.c_int, _f64p, C.c_double, C.c_int,
                                   _f64p, _f64p, _i32p]),
    ("svo_refine_poses_stereo", C.c_int, [_vp, _f64p, _f32p, _f32p, _i32p, C.c_int, C.c_int, _f64p, C.c_double,
                                          C.c_double, C.c_int, _f64p, _f64p, _i32p, _f64p]),
    ("svo_refine_poses_time", C.c_int, [_vp, _f64p, _f32p, _f32p, _i32p, C.c_int, C.c_int, _f64p, C.c_double,
                                        C.c_double, C.c_int, _f64p, C.c_int, _f64p, _f64p]),
    ("svo_pose_graph_optimize", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f64p, _u8p, _i32p, _f64p,
                                          _f64p, C.c_double, C.c_int, C.c_int, _f64p, _f64p, _i32p, _i32p]),
    ("svo_pose_graph_linearize", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f64p, _u8p, _i32p, _f64p,
                                           _f64p, C.c_double, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]),
    ("svo_pose_graph_time", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f64p, _u8p, _i32p, _f64p, _f64p,
                                      C.c_double, C.c_int, C.c_int, C.c_int, _f64p, _i32p, _i32p]),
    ("svo_pose_graph_edge", C.c_int, [_f64p, _f64p, _f64p]),
    ("svo_bundle_adjust", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _f64p, _u8p, _f64p,
                                    _i32p, _i32p, _f32p, _f64p, C.c_double, C.c_int, _f64p, _i32p]),
    ("svo_ba_linearize", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _f64p, _u8p, _f64p,
                                   _i32p, _i32p, _f32p, _f64p, C.c_double, C.c_double, _f64p, _f64p, _f64p, _f64p,
                                   _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, _i32p]),
    ("svo_bundle_adjust_stereo", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _f64p, _u8p,
                                           _f64p, _i32p, _i32p, _f32p, _f32p, C.c_double, _f64p, C.c_double, C.c_int,
                                           _f64p, _i32p]),
    ("svo_ba_linearize_stereo", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _f64p, _u8p,
                                          _f64p, _i32p, _i32p, _f32p, _f32p, C.c_double, _f64p, C.c_double, C.c_double,
                                          _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, _i32p]),
    ("svo_ba_stage_lists_stereo", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f32p, _f32p, _i32p, _f32p,
                                            _f32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p]),
    ("svo_ba_sort_observations", C.c_int, [_i32p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p]),
    ("svo_ba_stage_lists", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f32p, _i32p, _f32p, _i32p, _i32p,
                                     _i32p, _i32p, _i32p, _i32p, _i32p]),
    ("svo_ba_time_staging", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f32p, C.c_int, _f64p, _f64p,
                                      _f64p]),
    ("svo_ba_time_iteration", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i32p, _f64p, _u8p,
                                        _f64p, _i32p, _i32p, _f32p, _f64p, C.c_double, C.c_double, C.c_int, _f64p]),
    ("svo_frontend_create", C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    ("svo_frontend_destroy", None, [_vp]),
    ("svo_frontend_set_frame", C.c_int, [_vp, C.c_int, C.c_int, _u8p, _u8p, C.c_int]),
    ("svo_frontend_set_frame_bgr", C.c_int, [_vp, C.c_int, C.c_int, _u8p, _u8p, C.c_int]),
    ("svo_frontend_set_rectification", C.c_int, [_vp, _vp, _vp]),
    ("svo_frontend_time_ingest", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _f64p]),
    ("svo_frontend_map_points", C.c_int, [_vp, C.c_int, _f64p, C.c_int, _i32p]),
    ("svo_frontend_window_enable", C.c_int, [_vp, C.c_int]),
    ("svo_frontend_window", C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _f64p, _i32p, _i32p, _f32p]),
    ("svo_frontend_bundle_adjust", C.c_int, [_vp, C.c_int, C.c_double, C.c_int, _f64p, _i32p, _i32p]),
    ("svo_frontend_window_enable_stereo", C.c_int, [_vp, C.c_int]),
    ("svo_frontend_window_right", C.c_int, [_vp, C.c_int, C.c_int, _f32p]),
    ("svo_frontend_bundle_adjust_stereo", C.c_int, [_vp, C.c_int, C.c_double, C.c_int, _f64p, _i32p, _i32p]),
    ("svo_frontend_refine_poses", C.c_int, [_vp, C.c_double, C.c_int, _f64p, _i32p, _i32p]),
    ("svo_frontend_places_enable", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _i8p]),
    ("svo_frontend_place", C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _u8p, _f32p, _f64p, C.c_int]),
    ("svo_frontend_places_query", C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p,
                                            _i32p, _i32p, _f64p, _f64p, _i32p, _i32p, _i32p, C.c_int]),
    ("svo_frontend_places_time", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _f64p, _i32p]),
    ("svo_frontend_places_widen", C.c_int, [_vp, _u8p, _i32p, _f64p, _f64p, _vp, _i32p, _i32p, _i32p, _f64p, _f64p,
                                            _i32p, _i32p, C.c_int]),
    ("svo_frontend_time_pyramid", C.c_int, [_vp, C.c_int, C.c_int, _f64p]),
    ("svo_frontend_time_fast", C.c_int, [_vp, C.c_int, C.c_int, _f64p]),
    ("svo_frontend_pyramid_level", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int]),
    ("svo_frontend_scharr_level", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int16),
                                            C.POINTER(C.c_int16), C.c_int]),
    ("svo_frontend_prebuild_pyramids", C.c_int, [_vp]),
    ("svo_frontend_queue_frames", C.c_int, [_vp, C.c_int, C.POINTER(_u8p), C.POINTER(_u8p), C.c_int, C.c_int]),
    ("svo_frontend_upload_wait", C.c_int, [_vp, C.c_int]),
    ("svo_pinned_alloc", C.c_int, [C.c_size_t, C.POINTER(_vp)]),
    ("svo_pinned_free", None, [_vp]),
    ("svo_frontend_init", C.c_int, [_vp, C.c_int]),
    ("svo_frontend_step", C.c_int, [_vp, C.c_int, _vp]),
    ("svo_frontend_synchronize", C.c_int, [_vp]),
    ("svo_frontend_pose", C.c_int, [_vp, C.c_int, _f64p, _f64p]),
    ("svo_frontend_features", C.c_int, [_vp, C.c_int, _f32p, C.c_int, _i32p]),
    ("svo_frontend_phase_times", C.c_int, [_vp, _f64p, C.POINTER(C.c_int64), C.c_int]),
    ("svo_frontend_reset_times", None, [_vp]),
    ("svo_host_cpu_plan", C.c_int, [C.c_int, C.c_int, _i32p, _i32p, C.c_int, _i32p]),
    ("svo_frontend_host_cpus", C.c_int, [_vp, _i32p, C.c_int, _i32p]),
    ("svo_frontend_streams", C.c_int, [_vp, C.POINTER(_vp), C.c_int, _i32p]),
    ("svo_pool_selftest", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int64)]),
]

SYMBOLS = [s[0] for s in _SIGS]


def solve_pnp_sqpnp(obj, img_pts, K):
    """cv::solvePnP(..., SOLVEPNP_SQPNP) -> (ok, rvec, tvec): solvePnPRansac's final
    fit (svo_solve_pnp_sqpnp, host code of the library; no GPU context)."""
    obj = _c(obj, np.float64).reshape(-1, 3)
    img_pts = _c(img_pts, np.float32).reshape(-1, 2)
    K = _c(K, np.float64).reshape(9)
    rv = np.zeros(3)
    tv = np.zeros(3)
    rc = lib().svo_solve_pnp_sqpnp(_p(obj, _f64p), _p(img_pts, _f32p), len(obj), _p(K, _f64p), _p(rv, _f64p),
                                   _p(tv, _f64p))
    if rc < 0:
        raise SvoError(f"svo_solve_pnp_sqpnp: error {rc}")
    return rc == 1, rv, tv


ORB_DESC_BYTES = 32  # SVO_ORB_DESC_BYTES
PLACES_MAX_SLOTS = 16  # SVO_PLACES_MAX_SLOTS


def orb_default_pattern(patch_size: int = 31) -> np.ndarray:
    """svo_orb_default_pattern: OpenCV's makeRandomPattern, (512, 2) int8 (x, y)
    in [-patch_size // 2, patch_size // 2]. Host code of the library; no GPU context."""
    out = np.empty((512, 2), np.int8)
    if lib().svo_orb_default_pattern(int(patch_size), _p(out, _i8p)) != 0:
        raise SvoError("svo_orb_default_pattern: patch_size must be odd and in [5, 31]")
    return out


def orb_umax(patch_size: int = 31) -> np.ndarray:
    """svo_orb_umax (test view): the circular patch's half row widths, patch_size // 2 + 1 ints."""
    out = np.empty(16, np.int32)
    n = C.c_int()
    if lib().svo_orb_umax(int(patch_size), _p(out, _i32p), 16, C.byref(n)) != 0:
        raise SvoError("svo_orb_umax: patch_size must be odd and in [5, 31]")
    return out[: n.value].copy()


def match_filter(idx_qt, dist_qt, idx_tq=None, ratio_pct: int = 80, cap=None) -> np.ndarray:
    """svo_match_filter: ratio test (ratio_pct 0 = off) and, with the reverse match
    idx_tq, cross-check on match_hamming's output -> int32 (n, 2) pairs (q, t) in
    ascending q; the first `cap` of them when cap is given. Host code; no GPU context."""
    idx_qt = _c(idx_qt, np.int32).reshape(-1, 2)
    dist_qt = _c(dist_qt, np.int32).reshape(-1, 2)
    nq = len(idx_qt)
    assert len(dist_qt) == nq
    tq = None
    nt = int(idx_qt.max()) + 1 if nq else 0
    if idx_tq is not None:
        tq = _c(idx_tq, np.int32).reshape(-1, 2)
        nt = len(tq)
    cap = nq if cap is None else int(cap)
    pairs = np.empty((max(cap, 1), 2), np.int32)
    n = C.c_int()
    rc = lib().svo_match_filter(_p(idx_qt, _i32p), _p(dist_qt, _i32p), nq, None if tq is None else _p(tq, _i32p),
                                max(nt, 0), int(ratio_pct), _p(pairs, _i32p), cap, C.byref(n))
    if rc != 0:
        raise SvoError("svo_match_filter: bad arguments (negative ratio, or an index past the reverse match)")
    return pairs[: min(n.value, cap)].copy()


def trig_pa(x, fn: str, ctx=None) -> np.ndarray:
    """svo_trig_pa (test view): the final fit's plain-arithmetic trigonometry on the arguments
    x. fn "sincos" -> (n, 2) = (sin, cos); "acos" -> (n,). ctx None: on the host; a Context:
    on its GPU."""
    x = _c(x, np.float64).reshape(-1)
    out = np.full((len(x), 2), np.nan)
    rc = lib().svo_trig_pa(None if ctx is None else ctx.handle, _p(x, _f64p), len(x), {"sincos": 0, "acos": 1}[fn],
                           0 if ctx is None else 1, _p(out, _f64p))
    if rc != 0:
        raise SvoError(f"svo_trig_pa: error {rc}")
    return out if fn == "sincos" else out[:, 0].copy()


def pose_from_rvec(rvec, tvec) -> np.ndarray:
    """svo_pose_from_rvec: T = [R(rvec) row-major | tvec], 12 doubles, world -> camera:
    a pose as match_projected takes it. Host code of the library; no GPU context."""
    rv = _c(rvec, np.float64).reshape(3)
    tv = _c(tvec, np.float64).reshape(3)
    T = np.empty(12, np.float64)
    if lib().svo_pose_from_rvec(_p(rv, _f64p), _p(tv, _f64p), _p(T, _f64p)) != 0:
        raise SvoError("svo_pose_from_rvec: bad arguments")
    return T


class PinnedBuffer:
    """Page-locked host memory (svo_pinned_alloc) viewed as a numpy array: the
    source of svo_frontend_queue_frames' H2D copies at full PCIe rate. Freed by
    close() or when the object goes away (the array view must not outlive it)."""

    def __init__(self, shape, dtype=np.uint8):
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = _vp()
        if lib().svo_pinned_alloc(nbytes, C.byref(p)) != 0 or not p.value:
            raise SvoError(f"svo_pinned_alloc({nbytes}) failed")
        self._p = p
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self.array = None
            lib().svo_pinned_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def pool_selftest(threads=8, jobs=2000):
    """svo_pool_selftest: tasks of the front end's host pool run other than exactly
    once over `jobs` jobs of changing sizes (host code, no GPU); 0 = correct."""
    bad = C.c_int64(0)
    rc = lib().svo_pool_selftest(int(threads), int(jobs), C.byref(bad))
    if rc < 0:
        raise SvoError(f"svo_pool_selftest: error {rc}")
    return int(bad.value)


def host_cpu_plan(local_rank, local_world, gpu_node=None, cap=4096):
    """svo_host_cpu_plan: this rank's share of the node's CPUs (host code, no GPU)."""
    cpus = np.zeros(cap, np.int32)
    n = C.c_int(0)
    gn = None if gpu_node is None else np.ascontiguousarray(gpu_node, np.int32)
    rc = lib().svo_host_cpu_plan(int(local_rank), int(local_world), None if gn is None else _p(gn, _i32p),
                                 _p(cpus, _i32p), cap, C.byref(n))
    if rc != 0:
        raise SvoError(f"svo_host_cpu_plan: error {rc}")
    return cpus[:min(n.value, cap)].tolist()


def lib():
    """Load libsvo_gpu.so (built by __graft_entry__.build() / make)."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise SvoError(f"HIP extension not built: {path} missing (run __graft_entry__.build())")
        L = C.CDLL(path)
        ab = bool(os.environ.get("SVO_GPU_LIB"))
        for name, res, args in _SIGS:
            if ab and not hasattr(L, name):  # an older build under A/B: its missing entry points stay unbound
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(t)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class Image:
    """A device-resident 8U image with its pyrDown pyramid (levels 0..max_levels)."""

    def __init__(self, ctx: "Context", handle, w: int, h: int, max_levels: int):
        self.ctx, self.handle, self.w, self.h, self.max_levels = ctx, handle, w, h, max_levels
        ctx._deps[handle.value] = "image"
        _LIVE["image"].add(self)

    def level(self, l: int) -> np.ndarray:
        L = lib()
        w, h = C.c_int(), C.c_int()
        if L.svo_image_level_size(self.handle, l, C.byref(w), C.byref(h)) != 0:
            raise SvoError(f"no level {l}")
        out = np.empty((h.value, w.value), np.uint8)
        self.ctx._check(L.svo_image_download_level(self.ctx.handle, self.handle, l, _p(out, _u8p), w.value))
        return out

    def scharr(self, l: int):
        """(ix, iy) of level l as the LK kernels read them: Scharr derivatives x 4
        (int16) -- svo_image_scharr_level."""
        L = lib()
        w, h = C.c_int(), C.c_int()
        if L.svo_image_level_size(self.handle, l, C.byref(w), C.byref(h)) != 0:
            raise SvoError(f"no level {l}")
        ix = np.empty((h.value, w.value), np.int16)
        iy = np.empty_like(ix)
        self.ctx._check(L.svo_image_scharr_level(self.ctx.handle, self.handle, l,
                                                 ix.ctypes.data_as(C.POINTER(C.c_int16)),
                                                 iy.ctypes.data_as(C.POINTER(C.c_int16)), w.value))
        return ix, iy

    def upload(self, gray: np.ndarray):
        gray = _c(gray, np.uint8)
        assert gray.shape == (self.h, self.w)
        self.ctx._check(lib().svo_image_upload(self.ctx.handle, self.handle, _p(gray, _u8p), self.w))

    def upload_bgr(self, bgr: np.ndarray):
        """H2D of an (h, w, 3) BGR image, grey conversion on the device (cvtColor BGR2GRAY)."""
        bgr = _c(bgr, np.uint8)
        assert bgr.shape == (self.h, self.w, 3)
        self.ctx._check(lib().svo_image_upload_bgr(self.ctx.handle, self.handle, _p(bgr, _u8p), 3 * self.w))

    def upload_raw(self, raw: np.ndarray, maps: "RectMaps"):
        """H2D of a raw camera frame ((raw_h, raw_w) grey or (raw_h, raw_w, 3) BGR),
        rectified on the device into level 0 (cv::remap with `maps`), then the pyramid
        (svo_image_upload_raw)."""
        raw = _c(raw, np.uint8)
        bgr = raw.ndim == 3
        if raw.shape != (maps.raw_h, maps.raw_w) + ((3,) if bgr else ()):
            raise SvoError(f"upload_raw: a raw frame of {maps.raw_h} x {maps.raw_w} expected, got {raw.shape}")
        self.ctx._check(lib().svo_image_upload_raw(self.ctx.handle, self.handle, _p(raw, _u8p),
                                                   raw.shape[1] * (3 if bgr else 1), int(bgr), maps.handle))

    def close(self):
        if self.handle:
            if self.ctx._deps.pop(self.handle.value, None):  # (else the context went first and took it along)
                lib().svo_image_destroy(self.ctx.handle, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_i16p = C.POINTER(C.c_int16)
_u16p = C.POINTER(C.c_uint16)


def init_undistort_rectify_map(K, dist, R, newK, w, h):
    """cv::initUndistortRectifyMap(K, dist, R, newK, (w, h), CV_16SC2) -> (map1 (h, w, 2)
    int16, map2 (h, w) uint16); dist: up to 8 coefficients (k1, k2, p1, p2, k3, k4,
    k5, k6), zero-filled (svo_init_undistort_rectify_map: host code, no GPU context)."""
    d = np.zeros(8)
    dist = np.asarray(dist, np.float64).ravel()
    if len(dist) > 8:
        raise SvoError("init_undistort_rectify_map: at most 8 distortion coefficients")
    d[:len(dist)] = dist
    K, R, newK = (_c(m, np.float64).reshape(9) for m in (K, R, newK))
    map1 = np.zeros((max(h, 0), max(w, 0), 2), np.int16)
    map2 = np.zeros((max(h, 0), max(w, 0)), np.uint16)
    rc = lib().svo_init_undistort_rectify_map(_p(K, _f64p), _p(d, _f64p), _p(R, _f64p), _p(newK, _f64p), int(w),
                                              int(h), _p(map1, _i16p), _p(map2, _u16p))
    if rc != 0:
        raise SvoError(f"svo_init_undistort_rectify_map: error {rc} (sizes, or newK R is singular)")
    return map1, map2


class RectMaps:
    """One camera's rectification maps on the device (svo_rect_maps): the CV_16SC2 /
    CV_16UC1 pair of cv::initUndistortRectifyMap or cv::convertMaps for a raw_w x raw_h
    camera; the rectified size is the maps' own."""

    def __init__(self, ctx: "Context", raw_w: int, raw_h: int, map1, map2):
        map1 = _c(map1, np.int16)
        map2 = _c(map2, np.uint16)
        if map1.ndim != 3 or map1.shape[2] != 2 or map2.shape != map1.shape[:2]:
            raise SvoError("RectMaps: map1 (h, w, 2) int16 and map2 (h, w) uint16")
        self.ctx, self.raw_w, self.raw_h = ctx, int(raw_w), int(raw_h)
        self.h, self.w = map2.shape
        hd = _vp()
        ctx._check(lib().svo_rect_maps_create(ctx.handle, self.raw_w, self.raw_h, self.w, self.h, _p(map1, _i16p),
                                              _p(map2, _u16p), C.byref(hd)))
        self.handle = hd
        ctx._deps[hd.value] = "maps"
        _LIVE["maps"].add(self)

    def close(self):
        if getattr(self, "handle", None):
            if self.ctx._deps.pop(self.handle.value, None):  # (else the context went first and took it along)
                lib().svo_rect_maps_destroy(self.ctx.handle, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def remap(ctx: "Context", src, maps: RectMaps) -> np.ndarray:
    """cv::remap(src, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) of a raw frame
    ((raw_h, raw_w) grey, or (raw_h, raw_w, 3) BGR: grey taps) through the rectifying
    kernel -> (h, w) uint8 (svo_remap)."""
    src = _c(src, np.uint8)
    bgr = src.ndim == 3
    if src.shape != (maps.raw_h, maps.raw_w) + ((3,) if bgr else ()):
        raise SvoError(f"remap: a raw frame of {maps.raw_h} x {maps.raw_w} expected, got {src.shape}")
    out = np.empty((maps.h, maps.w), np.uint8)
    ctx._check(lib().svo_remap(ctx.handle, _p(src, _u8p), src.shape[1] * (3 if bgr else 1), int(bgr), maps.handle,
                               _p(out, _u8p), maps.w))
    return out


class OrbParams(C.Structure):
    """svo_orb_params; defaults = the reference's ORB (R:configs/config.yaml:20-27,
    R:src/tracking.cpp:33-50: edgeThreshold = patch_size, firstLevel 0, WTA_K 4, HARRIS)."""
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("edge_threshold", C.c_int), ("first_level", C.c_int), ("wta_k", C.c_int),
                ("score_type", C.c_int), ("patch_size", C.c_int), ("fast_threshold", C.c_int)]

    HARRIS, FAST = 0, 1

    def __init__(self, nfeatures=150, scale_factor=1.2, nlevels=8, patch_size=31, fast_threshold=20,
                 edge_threshold=None, score_type=0, wta_k=4):
        super().__init__()
        self.nfeatures, self.scale_factor, self.nlevels = nfeatures, scale_factor, nlevels
        self.edge_threshold = patch_size if edge_threshold is None else edge_threshold
        self.first_level, self.wta_k, self.score_type = 0, wta_k, score_type
        self.patch_size, self.fast_threshold = patch_size, fast_threshold


class StereoRowsParams(C.Structure):
    """svo_stereo_rows_params: row SAD, the stereo match of a rectified pair as a
    bounded search along the left point's row (include/svo_gpu.h has the rule).
    radius 1..7 (patch (2r+1)^2), disparities d_min (>= -16) .. d_max (<= 255), at
    most 256 of them, uniq_pct 0..100 (0 = off), max_cost >= 0 (0 = off)."""
    _fields_ = [("radius", C.c_int), ("d_min", C.c_int), ("d_max", C.c_int), ("uniq_pct", C.c_int),
                ("max_cost", C.c_int)]

    def __init__(self, radius=5, d_min=-1, d_max=128, uniq_pct=80, max_cost=0):
        super().__init__(int(radius), int(d_min), int(d_max), int(uniq_pct), int(max_cost))


class ProjMatchParams(C.Structure):
    """svo_proj_match_params (include/svo_gpu.h): the search window's half side in
    pixels, the largest distance that bids, the ratio test in percent (0 = off)."""
    _fields_ = [("radius", C.c_float), ("max_dist", C.c_int), ("ratio_pct", C.c_int)]

    def __init__(self, radius=4.0, max_dist=64, ratio_pct=80):
        super().__init__(float(radius), int(max_dist), int(ratio_pct))


class Context:
    """One HIP device + stream (svo_ctx)."""

    def __init__(self, device: int = 0):
        L = lib()
        h = _vp()
        self.device = device
        rc = L.svo_ctx_create(device, C.byref(h))
        if rc != 0:
            raise SvoError(f"svo_ctx_create(device={device}) failed: {rc} (no usable HIP device?)")
        self.handle = h
        self._deps = {}  # native handle -> "frontend" / "image" of the live dependants
        _LIVE["context"].add(self)

    def _check(self, rc):
        if rc < 0:
            raise SvoError(lib().svo_last_error(self.handle).decode() or f"error {rc}")
        return rc

    def close(self):
        if getattr(self, "handle", None):
            L = lib()
            for kind in ("frontend", "image", "maps"):  # dependants still alive go first (maps outlive front ends)
                for h in [h for h, k in self._deps.items() if k == kind]:
                    if kind == "frontend":
                        L.svo_frontend_destroy(_vp(h))
                    elif kind == "maps":
                        L.svo_rect_maps_destroy(self.handle, _vp(h))
                    else:
                        L.svo_image_destroy(self.handle, _vp(h))
                    del self._deps[h]
            L.svo_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- images
    def image(self, gray: np.ndarray, max_levels: int = 4) -> Image:
        gray = _c(gray, np.uint8)
        h, w = gray.shape
        hd = _vp()
        self._check(lib().svo_image_create(self.handle, w, h, max_levels, C.byref(hd)))
        img = Image(self, hd, w, h, max_levels)
        img.upload(gray)
        return img

    def image_bgr(self, bgr: np.ndarray, max_levels: int = 4) -> Image:
        """Device image from an (h, w, 3) BGR frame (svo_image_upload_bgr)."""
        bgr = _c(bgr, np.uint8)
        h, w, c = bgr.shape
        assert c == 3
        hd = _vp()
        self._check(lib().svo_image_create(self.handle, w, h, max_levels, C.byref(hd)))
        img = Image(self, hd, w, h, max_levels)
        img.upload_bgr(bgr)
        return img

    # ---------------------------------------------------------------- FAST
    def fast_detect(self, img: Image, threshold: int = 20, nonmax: bool = True, mask=None,
                    cap: int = 1 << 20, return_count: bool = False):
        """cv::FastFeatureDetector::detect -> float32 array (n, 3): x, y, response; the
        first `cap` keypoints when there are more. return_count: (that array,
        svo_fast_detect's n_out: the number found, also when it exceeds cap)."""
        out = np.empty((cap, 3), np.float32)
        n = C.c_int()
        mp = None
        if mask is not None:
            mask = _c(mask, np.uint8)
            assert mask.shape == (img.h, img.w)
            mp = _p(mask, _u8p)
        self._check(lib().svo_fast_detect(self.handle, img.handle, int(threshold), int(bool(nonmax)), mp,
                                          _p(out, _f32p), cap, C.byref(n)))
        kp = out[: min(n.value, cap)].copy()
        return (kp, n.value) if return_count else kp

    def orb_detect(self, img: Image, params: "OrbParams" = None, mask=None, cap: int = 1 << 16):
        """cv::ORB::detect -> (float32 (n, 3) x, y, response; int32 (n,) octave)."""
        params = params or OrbParams()
        out = np.empty((cap, 3), np.float32)
        octv = np.empty(cap, np.int32)
        n = C.c_int()
        mp = None
        if mask is not None:
            mask = _c(mask, np.uint8)
            assert mask.shape == (img.h, img.w)
            mp = _p(mask, _u8p)
        self._check(lib().svo_orb_detect(self.handle, img.handle, C.byref(params), mp, _p(out, _f32p),
                                         _p(octv, _i32p), cap, C.byref(n)))
        k = min(n.value, cap)
        return out[:k].copy(), octv[:k].copy()

    def orb_level(self, img: Image, params: "OrbParams" = None, mask=None, level: int = 0):
        """Test and debug only (svo_orb_level): level `level` of the scale pyramid
        svo_orb_detect builds, and of its mask pyramid -> (image, mask or None)."""
        params = params or OrbParams()
        out = np.empty(img.h * img.w, np.uint8)  # no level is larger than level 0
        om = mp = None
        if mask is not None:
            mask = _c(mask, np.uint8)
            assert mask.shape == (img.h, img.w)
            mp = _p(mask, _u8p)
            om = np.empty(img.h * img.w, np.uint8)
        lw, lh = C.c_int(), C.c_int()
        self._check(lib().svo_orb_level(self.handle, img.handle, C.byref(params), mp, int(level), _p(out, _u8p),
                                        None if om is None else _p(om, _u8p), C.byref(lw), C.byref(lh)))
        n = lw.value * lh.value
        shape = (lh.value, lw.value)
        return out[:n].reshape(shape).copy(), None if om is None else om[:n].reshape(shape).copy()

    # ---------------------------------------------------------------- ORB descriptors, matching
    @staticmethod
    def _pattern_arg(pattern):
        if pattern is None:
            return None, None
        pattern = _c(pattern, np.int8)
        if pattern.size != 1024:
            raise SvoError("pattern: 512 points (x, y) int8 expected")
        return pattern, _p(pattern, _i8p)

    def orb_compute(self, img: Image, kp, octave, params: "OrbParams" = None, pattern=None):
        """cv::ORB::compute by the rules of DESIGN.md section 3d (svo_orb_compute): kp
        (n, 2) or (n, 3) level-0 coordinates and octave (n,) as orb_detect returns
        them -> (desc (n, 32) u8, angle (n,) f32 degrees, valid (n,) bool). pattern:
        (512, 2) int8 or None for orb_default_pattern(params.patch_size)."""
        params = params or OrbParams(wta_k=2)
        kp = np.asarray(kp, np.float32)
        kp = kp.reshape(-1, kp.shape[-1] if kp.ndim == 2 else 2)
        n = len(kp)
        k3 = np.zeros((n, 3), np.float32)
        k3[:, :2] = kp[:, :2]
        octave = _c(octave, np.int32).reshape(-1)
        if len(octave) != n:
            raise SvoError("orb_compute: one octave per keypoint expected")
        desc = np.zeros((n, ORB_DESC_BYTES), np.uint8)
        angle = np.zeros(n, np.float32)
        valid = np.zeros(n, np.uint8)
        keep, pp = self._pattern_arg(pattern)
        self._check(lib().svo_orb_compute(self.handle, img.handle, C.byref(params), pp, _p(k3, _f32p),
                                          _p(octave, _i32p), n, _p(desc, _u8p), _p(angle, _f32p), _p(valid, _u8p)))
        return desc, angle, valid.astype(bool)

    def orb_detect_and_compute(self, img: Image, params: "OrbParams" = None, mask=None, pattern=None,
                               cap: int = 1 << 16):
        """cv::ORB::detectAndCompute (svo_orb_detect_and_compute; the pyramid is built
        once) -> (kp (n, 3) f32, octave (n,) i32, desc (n, 32) u8, angle (n,) f32,
        valid (n,) bool): orb_detect's keypoints with orb_compute's output."""
        params = params or OrbParams(wta_k=2)
        kp = np.empty((cap, 3), np.float32)
        octv = np.empty(cap, np.int32)
        desc = np.zeros((cap, ORB_DESC_BYTES), np.uint8)
        angle = np.zeros(cap, np.float32)
        valid = np.zeros(cap, np.uint8)
        n = C.c_int()
        mp = None
        if mask is not None:
            mask = _c(mask, np.uint8)
            assert mask.shape == (img.h, img.w)
            mp = _p(mask, _u8p)
        keep, pp = self._pattern_arg(pattern)
        self._check(lib().svo_orb_detect_and_compute(self.handle, img.handle, C.byref(params), mp, pp, _p(kp, _f32p),
                                                     _p(octv, _i32p), _p(desc, _u8p), _p(angle, _f32p),
                                                     _p(valid, _u8p), cap, C.byref(n)))
        k = min(n.value, cap)
        return kp[:k].copy(), octv[:k].copy(), desc[:k].copy(), angle[:k].copy(), valid[:k].astype(bool)

    def orb_blur_level(self, img: Image, params: "OrbParams" = None, level: int = 0) -> np.ndarray:
        """Test and debug only (svo_orb_blur_level): level `level` of the blurred
        pyramid the descriptors sample."""
        params = params or OrbParams(wta_k=2)
        out = np.empty(img.h * img.w, np.uint8)  # no level is larger than level 0
        lw, lh = C.c_int(), C.c_int()
        self._check(lib().svo_orb_blur_level(self.handle, img.handle, C.byref(params), int(level), _p(out, _u8p),
                                             C.byref(lw), C.byref(lh)))
        return out[: lw.value * lh.value].reshape(lh.value, lw.value).copy()

    def match_hamming(self, q, t, nq=None, nt=None, idx=None, dist=None):
        """cv::BFMatcher(NORM_HAMMING)::knnMatch(k = 2) (svo_match_hamming), ties to the
        lowest train index. Single sets: q (nq, 32), t (nt, 32) u8 -> (idx (nq, 2) i32,
        dist (nq, 2) i32), best then second best; a missing neighbour is (-1, 257).
        Batched: q (P, q_stride, 32), t (P, t_stride, 32) with counts nq (P,), nt (P,)
        -> (P, q_stride, 2) arrays whose rows past nq[p] keep what idx / dist (given,
        int32, written in place) held, or (-1, 257) without them."""
        q = _c(q, np.uint8)
        t = _c(t, np.uint8)
        if nq is None and nt is None:
            q = q.reshape(-1, ORB_DESC_BYTES)
            t = t.reshape(-1, ORB_DESC_BYTES)
            P, qs, ts = 1, len(q), len(t)
            nq_a, nt_a = np.array([qs], np.int32), np.array([ts], np.int32)
            shape = (qs, 2)
        else:
            if q.ndim != 3 or t.ndim != 3 or q.shape[2] != ORB_DESC_BYTES or t.shape[2] != ORB_DESC_BYTES or \
                    len(q) != len(t) or nq is None or nt is None:
                raise SvoError("match_hamming: batched form takes q (P, q_stride, 32), t (P, t_stride, 32), nq, nt")
            P, qs, ts = len(q), q.shape[1], t.shape[1]
            nq_a, nt_a = _c(nq, np.int32).reshape(-1), _c(nt, np.int32).reshape(-1)
            if len(nq_a) != P or len(nt_a) != P:
                raise SvoError("match_hamming: one count per problem expected")
            shape = (P, qs, 2)
        if idx is None:
            idx = np.full(shape, -1, np.int32)
        if dist is None:
            dist = np.full(shape, 257, np.int32)
        if idx.dtype != np.int32 or dist.dtype != np.int32 or idx.shape != shape or dist.shape != shape or \
                not idx.flags.c_contiguous or not dist.flags.c_contiguous:
            raise SvoError(f"match_hamming: idx / dist must be C-contiguous int32 of shape {shape}")
        self._check(lib().svo_match_hamming(self.handle, P, _p(nq_a, _i32p), _p(nt_a, _i32p), qs, ts, _p(q, _u8p),
                                            _p(t, _u8p), _p(idx, _i32p), _p(dist, _i32p)))
        return idx, dist

    def match_filter_batch(self, idx_qt, dist_qt, nq, nt, idx_tq=None, ratio_pct: int = 80, pairs=None):
        """svo_match_filter_batch: match_filter on the device for P problems at once, on
        match_hamming's batched outputs: idx_qt / dist_qt (P, q_stride, 2), counts nq /
        nt (P,), the reverse match idx_tq (P, t_stride, 2) or None for no cross-check ->
        (pairs (P, q_stride, 2) int32, n (P,)): problem p's pairs (q, t) in ascending q
        in rows [0, n[p]); the rows behind keep what `pairs` (given, written in place)
        held, or -1 without it."""
        idx_qt = _c(idx_qt, np.int32)
        dist_qt = _c(dist_qt, np.int32)
        if idx_qt.ndim != 3 or idx_qt.shape[2] != 2 or dist_qt.shape != idx_qt.shape:
            raise SvoError("match_filter_batch: idx_qt / dist_qt of shape (P, q_stride, 2)")
        P, qs = idx_qt.shape[:2]
        nq_a, nt_a = _c(nq, np.int32).reshape(-1), _c(nt, np.int32).reshape(-1)
        if len(nq_a) != P or len(nt_a) != P:
            raise SvoError("match_filter_batch: one count per problem expected")
        tq, ts = None, int(nt_a.max()) if P else 0
        if idx_tq is not None:
            tq = _c(idx_tq, np.int32)
            if tq.ndim != 3 or tq.shape[0] != P or tq.shape[2] != 2:
                raise SvoError("match_filter_batch: idx_tq of shape (P, t_stride, 2)")
            ts = tq.shape[1]
        if pairs is None:
            pairs = np.full((P, qs, 2), -1, np.int32)
        if pairs.dtype != np.int32 or pairs.shape != (P, qs, 2) or not pairs.flags.c_contiguous:
            raise SvoError(f"match_filter_batch: pairs must be C-contiguous int32 of shape {(P, qs, 2)}")
        n = np.zeros(max(P, 1), np.int32)
        self._check(lib().svo_match_filter_batch(self.handle, P, _p(nq_a, _i32p), _p(nt_a, _i32p), qs, ts,
                                                 _p(idx_qt, _i32p), _p(dist_qt, _i32p),
                                                 None if tq is None else _p(tq, _i32p), int(ratio_pct),
                                                 _p(pairs, _i32p), _p(n, _i32p)))
        return pairs, n[:P]

    def orb_describe_time(self, img: Image, params: "OrbParams" = None, cap: int = 1 << 16, reps: int = 20):
        """Measurement only (svo_orb_describe_time): ms per launch of the blur, angle and
        BRIEF kernels on img's detected keypoints -> (ms (3,), keypoints)."""
        params = params or OrbParams(wta_k=2)
        ms = np.zeros(3, np.float64)
        n = C.c_int()
        self._check(lib().svo_orb_describe_time(self.handle, img.handle, C.byref(params), int(cap), int(reps),
                                                _p(ms, _f64p), C.byref(n)))
        return ms, n.value

    def match_hamming_time(self, q, t, nq, nt, reps: int = 10) -> float:
        """Measurement only (svo_match_hamming_time): ms per launch of the matcher on
        the batch q (P, q_stride, 32), t (P, t_stride, 32) with counts nq, nt."""
        q = _c(q, np.uint8)
        t = _c(t, np.uint8)
        nq_a, nt_a = _c(nq, np.int32).reshape(-1), _c(nt, np.int32).reshape(-1)
        assert q.ndim == 3 and t.ndim == 3 and len(q) == len(t) == len(nq_a) == len(nt_a)
        ms = C.c_double()
        self._check(lib().svo_match_hamming_time(self.handle, len(q), _p(nq_a, _i32p), _p(nt_a, _i32p), q.shape[1],
                                                 t.shape[1], _p(q, _u8p), _p(t, _u8p), int(reps), C.byref(ms)))
        return ms.value

    def relocalize(self, map_desc, map_xyz, desc, kp_xy, K, ratio_pct: int = 80, cross_check: bool = True,
                   iterations: int = 100, reproj_err: float = 8.0, confidence: float = 0.999):
        """Pose of a described frame against a described map: match_hamming of the
        frame's descriptors (queries) against the map's and, with cross_check, the
        reverse; match_filter; solve_pnp_ransac on the surviving pairs -> (rvec, tvec,
        inlier pairs (m, 2) of (frame index, map index)). SvoError when fewer than 4
        pairs survive or RANSAC finds no model."""
        map_desc = _c(map_desc, np.uint8).reshape(-1, ORB_DESC_BYTES)
        desc = _c(desc, np.uint8).reshape(-1, ORB_DESC_BYTES)
        map_xyz = _c(map_xyz, np.float64).reshape(-1, 3)
        kp_xy = np.asarray(kp_xy, np.float32)
        kp_xy = _c(kp_xy.reshape(len(desc), -1)[:, :2], np.float32)
        if len(map_xyz) != len(map_desc):
            raise SvoError("relocalize: one map point per map descriptor expected")
        idx_qt, dist_qt = self.match_hamming(desc, map_desc)
        idx_tq = self.match_hamming(map_desc, desc)[0] if cross_check else None
        pairs = match_filter(idx_qt, dist_qt, idx_tq, ratio_pct)
        if len(pairs) < 4:
            raise SvoError(f"relocalize: {len(pairs)} matches survive the filter, 4 needed")
        ok, rvec, tvec, inl = self.solve_pnp_ransac(map_xyz[pairs[:, 1]], kp_xy[pairs[:, 0]], K, iterations,
                                                    reproj_err, confidence)
        if not ok:
            raise SvoError("relocalize: RANSAC found no pose")
        return rvec, tvec, pairs[inl]

    def _proj_args(self, who, xyz, pdesc, kxy, kdesc, pose, K, size, n_pts, n_kp):
        xyz = _c(xyz, np.float64)
        pdesc = _c(pdesc, np.uint8)
        kxy = _c(kxy, np.float32)
        kdesc = _c(kdesc, np.uint8)
        pose = _c(pose, np.float64)
        K = _c(K, np.float64).reshape(-1)
        K4 = K if len(K) == 4 else _c(K.reshape(9)[[0, 4, 2, 5]], np.float64)
        w, h = int(size[0]), int(size[1])
        if n_pts is None and n_kp is None:
            xyz, pdesc = xyz.reshape(-1, 3), pdesc.reshape(-1, ORB_DESC_BYTES)
            kxy, kdesc = kxy.reshape(-1, 2), kdesc.reshape(-1, ORB_DESC_BYTES)
            P, ps, ks = 1, len(xyz), len(kxy)
            np_a, nk_a = np.array([ps], np.int32), np.array([ks], np.int32)
            lead = ()
        else:
            if xyz.ndim != 3 or pdesc.ndim != 3 or kxy.ndim != 3 or kdesc.ndim != 3 or n_pts is None or n_kp is None:
                raise SvoError(f"{who}: batched form takes xyz (P, p_stride, 3), pdesc (P, p_stride, 32), "
                               "kxy (P, k_stride, 2), kdesc (P, k_stride, 32), n_pts, n_kp")
            P, ps, ks = len(xyz), xyz.shape[1], kxy.shape[1]
            np_a, nk_a = _c(n_pts, np.int32).reshape(-1), _c(n_kp, np.int32).reshape(-1)
            if len(np_a) != P or len(nk_a) != P or len(kxy) != P:
                raise SvoError(f"{who}: one count per problem expected")
            lead = (P,)
        if xyz.shape != lead + (ps, 3) or pdesc.shape != lead + (ps, ORB_DESC_BYTES) or \
                kxy.shape != lead + (ks, 2) or kdesc.shape != lead + (ks, ORB_DESC_BYTES) or pose.size != 12 * P:
            raise SvoError(f"{who}: one descriptor per point and per keypoint, 12 pose doubles per problem expected")
        return xyz, pdesc, kxy, kdesc, pose, K4, w, h, P, ps, ks, np_a, nk_a, lead

    def match_projected(self, xyz, pdesc, kxy, kdesc, pose, K, size, params: "ProjMatchParams" = None, n_pts=None,
                        n_kp=None, idx=None, dist=None, proj=None, pairs=None):
        """svo_match_projected: the points xyz (f64, world) with
        descriptors pdesc projected under pose (12 doubles [R row-major | t], world ->
        camera: pose_from_rvec) and K (3x3, or (fx, fy, cx, cy)) into a frame of size =
        (w, h), each matched against the keypoints kxy / kdesc inside a window of
        +-params.radius. Single sets: xyz (n, 3), kxy (m, 2) -> (idx (n, 2), dist (n, 2),
        proj (n, 2) f32, pairs (m, 2), n_pairs): best then second-best keypoint of every
        point (a missing one -1 / 257), the projections, and the pairs (keypoint, point)
        in ascending keypoint, rows [0, n_pairs). Batched: (P, stride, ...) arrays with
        counts n_pts, n_kp (P,), pose (P, 12) -> (P, stride, 2) arrays and n_pairs (P,).
        Rows past the counts keep what idx / dist / proj / pairs (given, written in
        place) held, or -1 (257 for dist) without them."""
        who = "match_projected"
        params = params or ProjMatchParams()
        xyz, pdesc, kxy, kdesc, pose, K4, w, h, P, ps, ks, np_a, nk_a, lead = self._proj_args(
            who, xyz, pdesc, kxy, kdesc, pose, K, size, n_pts, n_kp)
        outs = []
        for name, a, rows, dt, fill in (("idx", idx, ps, np.int32, -1), ("dist", dist, ps, np.int32, 257),
                                        ("proj", proj, ps, np.float32, -1), ("pairs", pairs, ks, np.int32, -1)):
            shape = lead + (rows, 2)
            if a is None:
                a = np.full(shape, fill, dt)
            if a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
                raise SvoError(f"{who}: {name} must be C-contiguous {np.dtype(dt).name} of shape {shape}")
            outs.append(a)
        idx, dist, proj, pairs = outs
        n = np.zeros(max(P, 1), np.int32)
        self._check(lib().svo_match_projected(
            self.handle, P, _p(np_a, _i32p), _p(nk_a, _i32p), ps, ks, _p(xyz, _f64p), _p(pdesc, _u8p), _p(kxy, _f32p),
            _p(kdesc, _u8p), _p(pose, _f64p), _p(K4, _f64p), w, h, C.addressof(params), _p(idx, _i32p),
            _p(dist, _i32p), _p(proj, _f32p), _p(pairs, _i32p), _p(n, _i32p)))
        return idx, dist, proj, pairs, (n[:P] if lead else int(n[0]))

    def match_projected_time(self, xyz, pdesc, kxy, kdesc, pose, K, size, n_pts, n_kp,
                             params: "ProjMatchParams" = None, reps: int = 10) -> np.ndarray:
        """Measurement only (svo_match_projected_time): ms per launch of the bin, match
        and pairs kernels on the batch (match_projected's batched form) -> (3,)."""
        params = params or ProjMatchParams()
        xyz, pdesc, kxy, kdesc, pose, K4, w, h, P, ps, ks, np_a, nk_a, _ = self._proj_args(
            "match_projected_time", xyz, pdesc, kxy, kdesc, pose, K, size, n_pts, n_kp)
        ms = np.zeros(3, np.float64)
        self._check(lib().svo_match_projected_time(
            self.handle, P, _p(np_a, _i32p), _p(nk_a, _i32p), ps, ks, _p(xyz, _f64p), _p(pdesc, _u8p), _p(kxy, _f32p),
            _p(kdesc, _u8p), _p(pose, _f64p), _p(K4, _f64p), w, h, C.addressof(params), int(reps), _p(ms, _f64p)))
        return ms

    def relocalize_guided(self, map_desc, map_xyz, desc, kp_xy, K, size, params: "ProjMatchParams" = None,
                          **relocalize_kw):
        """relocalize, then the second look every ORB-style system takes before it
        accepts such a pose: match_projected of the whole map under the first pose
        into the frame of size = (w, h), and solve_pnp_ransac (relocalize's iterations,
        reproj_err, confidence) on the widened pairs in ascending frame index ->
        (rvec, tvec, inlier pairs (m, 2) of (frame index, map index), first), first =
        relocalize's own (rvec, tvec, inlier pairs). SvoError as relocalize's, and when
        fewer than 4 widened pairs remain or their RANSAC finds no model."""
        first = self.relocalize(map_desc, map_xyz, desc, kp_xy, K, **relocalize_kw)
        map_desc = _c(map_desc, np.uint8).reshape(-1, ORB_DESC_BYTES)
        desc = _c(desc, np.uint8).reshape(-1, ORB_DESC_BYTES)
        map_xyz = _c(map_xyz, np.float64).reshape(-1, 3)
        kp_xy = _c(np.asarray(kp_xy, np.float32).reshape(len(desc), -1)[:, :2], np.float32)
        _, _, _, pairs, n = self.match_projected(map_xyz, map_desc, kp_xy, desc, pose_from_rvec(first[0], first[1]), K,
                                                 size, params)
        pairs = pairs[:n]
        if n < 4:
            raise SvoError(f"relocalize_guided: {n} widened pairs, 4 needed")
        rkw = {k: relocalize_kw[k] for k in ("iterations", "reproj_err", "confidence") if k in relocalize_kw}
        ok, rvec, tvec, inl = self.solve_pnp_ransac(map_xyz[pairs[:, 1]], kp_xy[pairs[:, 0]], K, **rkw)
        if not ok:
            raise SvoError("relocalize_guided: RANSAC found no pose on the widened pairs")
        return rvec, tvec, pairs[inl], first

    def fast_score_map(self, img: Image, threshold: int = 20):
        score = np.empty((img.h, img.w), np.uint8)
        corner = np.empty((img.h, img.w), np.uint8)
        self._check(lib().svo_fast_score_map(self.handle, img.handle, int(threshold), _p(score, _u8p),
                                             _p(corner, _u8p)))
        return score, corner

    def mask_boxes(self, w: int, h: int, pts, half: float = 10.0) -> np.ndarray:
        pts = _c(pts, np.float32).reshape(-1, 2)
        mask = np.empty((h, w), np.uint8)
        self._check(lib().svo_mask_boxes(self.handle, w, h, _p(pts, _f32p), len(pts), float(half),
                                         _p(mask, _u8p)))
        return mask

    # ---------------------------------------------------------------- bucket
    def bucket_features(self, pts, img_w: int, img_h: int, bucket_size: int, per_bucket: int,
                        ages=None):
        pts = _c(pts, np.float32).reshape(-1, 2)
        n = len(pts)
        cap = (img_h // bucket_size + 1) * (img_w // bucket_size + 1) * per_bucket + 1
        xy_out = np.empty((cap, 2), np.float32)
        ages_out = np.empty(cap, np.int32)
        ap = None
        if ages is not None:
            ages = _c(ages, np.int32)
            ap = _p(ages, _i32p)
        nout = C.c_int()
        self._check(lib().svo_bucket_features(self.handle, _p(pts, _f32p), ap, n, img_w, img_h, bucket_size,
                                              per_bucket, _p(xy_out, _f32p), _p(ages_out, _i32p), cap,
                                              C.byref(nout)))
        k = min(nout.value, cap)
        return xy_out[:k].copy(), ages_out[:k].copy()

    # ---------------------------------------------------------------- LK
    def calc_optical_flow_pyr_lk(self, prev: Image, nxt: Image, prev_pts, next_pts=None,
                                 win_size=(21, 21), max_level: int = 3,
                                 criteria=(TERM_COUNT | TERM_EPS, 30, 0.01), flags: int = 0,
                                 min_eig_threshold: float = 1e-4, want_err: bool = True, split: int = None):
        """cv::calcOpticalFlowPyrLK -> (next_pts (n,2) f32, status (n,) u8, err (n,) f32).
        split: the call as two launches, points [0, split) and [split, n)
        (svo_calc_optical_flow_pyr_lk_split); the same outputs."""
        prev_pts = _c(prev_pts, np.float32).reshape(-1, 2)
        n = len(prev_pts)
        if next_pts is None:
            nxt_pts = np.zeros((n, 2), np.float32)
        else:
            nxt_pts = _c(next_pts, np.float32).reshape(-1, 2).copy()
        status = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32) if want_err else None
        ctype, count, eps = criteria
        tail = (_p(nxt_pts, _f32p), _p(status, _u8p), _p(err, _f32p) if err is not None else None, int(win_size[0]),
                int(win_size[1]), int(max_level), int(ctype), int(count), float(eps), int(flags),
                float(min_eig_threshold))
        if split is None:
            self._check(lib().svo_calc_optical_flow_pyr_lk(
                self.handle, prev.handle, nxt.handle, _p(prev_pts, _f32p), n, *tail))
        else:
            self._check(lib().svo_calc_optical_flow_pyr_lk_split(
                self.handle, prev.handle, nxt.handle, _p(prev_pts, _f32p), n, int(split), *tail))
        return nxt_pts, status, err

    def lk_last_iterations(self) -> int:
        return int(lib().svo_lk_last_iterations(self.handle))

    # ---------------------------------------------------------------- stereo rows
    def stereo_match_rows(self, left: Image, right: Image, pts, params: "StereoRowsParams" = None,
                          want_cost: bool = False):
        """svo_stereo_match_rows on a rectified pair -> (next_pts (n, 2) f32, status (n,)
        u8), and with want_cost also (disparity (n,) i32, cost (n,) i32)."""
        params = params or StereoRowsParams()
        pts = _c(pts, np.float32).reshape(-1, 2)
        n = len(pts)
        nxt = np.zeros((n, 2), np.float32)
        status = np.zeros(n, np.uint8)
        disp = np.zeros(n, np.int32) if want_cost else None
        cost = np.zeros(n, np.int32) if want_cost else None
        self._check(lib().svo_stereo_match_rows(
            self.handle, left.handle, right.handle, _p(pts, _f32p), n, C.byref(params), _p(nxt, _f32p),
            _p(status, _u8p), _p(disp, _i32p) if want_cost else None, _p(cost, _i32p) if want_cost else None))
        return (nxt, status, disp, cost) if want_cost else (nxt, status)

    def stereo_match_rows_guided(self, left: Image, right: Image, pts, d_prior=None, guide: int = 4,
                                 params: "StereoRowsParams" = None, want_cost: bool = False):
        """svo_stereo_match_rows_guided: stereo_match_rows where point i searches
        d_prior[i] +- guide (STEREO_NO_PRIOR: the full range); d_prior None or guide 0
        is stereo_match_rows itself. Returns what stereo_match_rows returns."""
        params = params or StereoRowsParams()
        pts = _c(pts, np.float32).reshape(-1, 2)
        n = len(pts)
        if d_prior is not None:
            d_prior = _c(d_prior, np.int32).reshape(-1)
            if len(d_prior) != n:
                raise ValueError("d_prior: one int per point")
        nxt = np.zeros((n, 2), np.float32)
        status = np.zeros(n, np.uint8)
        disp = np.zeros(n, np.int32) if want_cost else None
        cost = np.zeros(n, np.int32) if want_cost else None
        self._check(lib().svo_stereo_match_rows_guided(
            self.handle, left.handle, right.handle, _p(pts, _f32p), n, C.byref(params),
            _p(d_prior, _i32p) if d_prior is not None else None, int(guide), _p(nxt, _f32p), _p(status, _u8p),
            _p(disp, _i32p) if want_cost else None, _p(cost, _i32p) if want_cost else None))
        return (nxt, status, disp, cost) if want_cost else (nxt, status)

    def stereo_row_priors(self, mid, prev_mid, prev_xy, prev_ur):
        """svo_stereo_row_priors: per feature id in mid its disparity in the previous
        frame's lists (prev_mid strictly increasing, prev_xy (m, 2), prev_ur (m,)), or
        STEREO_NO_PRIOR -> (n,) i32."""
        mid = _c(mid, np.int32).reshape(-1)
        prev_mid = _c(prev_mid, np.int32).reshape(-1)
        prev_xy = _c(prev_xy, np.float32).reshape(-1, 2)
        prev_ur = _c(prev_ur, np.float32).reshape(-1)
        if not (len(prev_mid) == len(prev_xy) == len(prev_ur)):
            raise ValueError("prev_mid, prev_xy, prev_ur: one entry per previous feature")
        out = np.zeros(len(mid), np.int32)
        self._check(lib().svo_stereo_row_priors(
            self.handle, _p(mid, _i32p), len(mid), _p(prev_mid, _i32p), _p(prev_xy, _f32p), _p(prev_ur, _f32p),
            len(prev_mid), _p(out, _i32p)))
        return out

    # ---------------------------------------------------------------- PnP
    def pnp_residuals(self, obj, img_pts, hyps, K, thresh2: float = 64.0, want_err: bool = True):
        """hyps: (m, 12) = R row-major + t. -> (err (m,n) f32, mask (m,n) u8, counts (m,))."""
        obj = _c(obj, np.float32).reshape(-1, 3)
        img_pts = _c(img_pts, np.float32).reshape(-1, 2)
        hyps = _c(hyps, np.float64).reshape(-1, 12)
        K = _c(K, np.float64).reshape(9)
        n, m = len(obj), len(hyps)
        err = np.empty((m, n), np.float32) if want_err else None
        mask = np.empty((m, n), np.uint8)
        counts = np.empty(m, np.int32)
        self._check(lib().svo_pnp_residuals(self.handle, _p(obj, _f32p), _p(img_pts, _f32p), n,
                                            _p(hyps, _f64p), m, _p(K, _f64p), float(thresh2),
                                            _p(err, _f32p) if err is not None else None,
                                            _p(mask, _u8p), _p(counts, _i32p)))
        return err, mask, counts

    def epnp_subsets(self, subsets, K, device=True):
        """RANSAC's EPnP on (m, 25) float subsets (obj xyz x5, img xy x5) -> (Rt (m, 12), ok (m,)):
        device 0 / False: the host solver the RANSAC uses (bit-identical to the
        oracle's EPnP); 1 / True: the QL variant, one wave per subset on the GPU;
        2: that variant's host twin (bit-identical to 1); 3 / 4 / 5: device 0 forced
        to its scalar / AVX2 / AVX-512 form; 6: device 0's solver on the GPU, one
        lane per subset (bit-identical to 0)."""
        subsets = _c(subsets, np.float32).reshape(-1, 25)
        K = _c(K, np.float64).reshape(9)
        m = len(subsets)
        Rt = np.zeros((m, 12), np.float64)
        ok = np.zeros(m, np.int32)
        self._check(lib().svo_epnp_subsets(self.handle, _p(subsets, _f32p), m, _p(K, _f64p), int(device),
                                           _p(Rt, _f64p), _p(ok, _i32p)))
        return Rt, ok

    def pnp_score(self, obj, img_pts, counts, hyps, m, K, thresh2, bits, cnt):
        """svo_pnp_score (test view): the front end's scoring kernel on S sequences. obj (S, cap, 3)
        f32, img_pts (S, cap, 2) f32, counts (S,), hyps (S, m_stride, 12) f64 of which the first m
        rows are scored; bits (S, m_stride, words_cap) u32 and cnt (S, m_stride) i32 are read and
        written in place (what the kernel leaves alone keeps the caller's values) and returned."""
        obj = _c(obj, np.float32)
        img_pts = _c(img_pts, np.float32)
        counts = _c(counts, np.int32)
        hyps = _c(hyps, np.float64)
        K = _c(K, np.float64).reshape(9)
        S, cap = obj.shape[0], obj.shape[1]
        m_stride, words_cap = bits.shape[1], bits.shape[2]
        if (obj.shape != (S, cap, 3) or img_pts.shape != (S, cap, 2) or counts.shape != (S,)
                or hyps.shape != (S, m_stride, 12) or cnt.shape != (S, m_stride)
                or bits.dtype != np.uint32 or cnt.dtype != np.int32
                or not bits.flags.c_contiguous or not cnt.flags.c_contiguous):
            raise ValueError("pnp_score: shapes / dtypes")
        self._check(lib().svo_pnp_score(self.handle, _p(obj, _f32p), _p(img_pts, _f32p), _p(counts, _i32p), S, cap,
                                        _p(hyps, _f64p), int(m), m_stride, _p(K, _f64p), float(thresh2),
                                        _p(bits, _u32p), words_cap, _p(cnt, _i32p)))
        return bits, cnt

    def sqpnp_stats(self, obj, img_pts, counts, bits, K):
        """svo_sqpnp_stats (test view): SQPnP's 40 sufficient statistics of the points whose bit is
        set, per sequence (the front end's suffstats kernel). obj (S, cap, 3) f32, img_pts (S, cap, 2)
        f32, counts (S,), bits (S, words_cap) u32 -> (S, 40) f64."""
        obj = _c(obj, np.float32)
        img_pts = _c(img_pts, np.float32)
        counts = _c(counts, np.int32)
        bits = _c(bits, np.uint32)
        K = _c(K, np.float64).reshape(9)
        S, cap = obj.shape[0], obj.shape[1]
        if obj.shape != (S, cap, 3) or img_pts.shape != (S, cap, 2) or counts.shape != (S,) or bits.shape[:1] != (S,) \
                or bits.ndim != 2:
            raise ValueError("sqpnp_stats: shapes")
        stats = np.full((S, 40), np.nan)
        self._check(lib().svo_sqpnp_stats(self.handle, _p(obj, _f32p), _p(img_pts, _f32p), _p(counts, _i32p), S, cap,
                                          _p(bits, _u32p), bits.shape[1], _p(K, _f64p), _p(stats, _f64p)))
        return stats

    def sqpnp_fit(self, stats, mode, R, t, rv, obj, counts, bits, device=True):
        """svo_sqpnp_fit (test view): the final SQPnP fits from the statistics of sqpnp_stats and
        the poses the front end reports -> (pose6 (S, 6) = (rvec, tvec), pose12 (S, 12) camera ->
        world). mode (S,): 0 no model, 1 fit (R (S, 9), t (S, 3): the RANSAC model to fall back
        to), 2 given (rv (S, 3), t). device True: the device fit; False: the host pool's code."""
        stats = _c(stats, np.float64).reshape(-1, 40)
        S = len(stats)
        mode = _c(mode, np.int32).reshape(S)
        R = _c(R, np.float64).reshape(S, 9)
        t = _c(t, np.float64).reshape(S, 3)
        rv = _c(rv, np.float64).reshape(S, 3)
        obj = _c(obj, np.float32)
        counts = _c(counts, np.int32).reshape(S)
        bits = _c(bits, np.uint32)
        if obj.ndim != 3 or obj.shape[0] != S or obj.shape[2] != 3 or bits.ndim != 2 or bits.shape[0] != S:
            raise ValueError("sqpnp_fit: shapes")
        pose6 = np.full((S, 6), np.nan)
        pose12 = np.full((S, 12), np.nan)
        self._check(lib().svo_sqpnp_fit(self.handle, _p(stats, _f64p), _p(mode, _i32p), _p(R, _f64p), _p(t, _f64p),
                                        _p(rv, _f64p), _p(obj, _f32p), _p(counts, _i32p), S, obj.shape[1],
                                        _p(bits, _u32p), bits.shape[1], int(bool(device)), _p(pose6, _f64p),
                                        _p(pose12, _f64p)))
        return pose6, pose12

    def triangulate_points(self, P1, P2, pts1, pts2):
        """cv::triangulatePoints + convertPointsFromHomogeneous -> (xyzw (n,4), xyz (n,3)) float32."""
        P1 = _c(P1, np.float32).reshape(12)
        P2 = _c(P2, np.float32).reshape(12)
        pts1 = _c(pts1, np.float32).reshape(-1, 2)
        pts2 = _c(pts2, np.float32).reshape(-1, 2)
        n = len(pts1)
        if len(pts2) != n:
            raise ValueError("pts1 and pts2 differ in length")
        h = np.empty((n, 4), np.float32)
        x = np.empty((n, 3), np.float32)
        self._check(lib().svo_triangulate_points(self.handle, _p(P1, _f32p), _p(P2, _f32p), _p(pts1, _f32p),
                                                 _p(pts2, _f32p), n, _p(h, _f32p), _p(x, _f32p)))
        return h, x

    def reprojection_jacobians(self, obj, img_pts, poses, K, counts=None, huber_delta: float = 0.0):
        """obj (P, n, 3) f64, img (P, n, 2) f32, poses (P, 12) -> (res (P,n,2), jac (P,n,2,6), normal (P,28))."""
        obj = _c(obj, np.float64)
        if obj.ndim == 2:
            obj = obj[None]
        P, n = obj.shape[0], obj.shape[1]
        img_pts = _c(img_pts, np.float32).reshape(P, n, 2)
        poses = _c(poses, np.float64).reshape(P, 12)
        K = _c(K, np.float64).reshape(9)
        cnt = _c(counts, np.int32).reshape(P) if counts is not None else None
        res = np.empty((P, n, 2), np.float64)
        jac = np.empty((P, n, 2, 6), np.float64)
        ne = np.empty((P, 28), np.float64)
        self._check(lib().svo_reprojection_jacobians(self.handle, _p(obj, _f64p), _p(img_pts, _f32p),
                                                     _p(cnt, _i32p) if cnt is not None else None, P, n,
                                                     _p(poses, _f64p), _p(K, _f64p), float(huber_delta),
                                                     _p(res, _f64p), _p(jac, _f64p), _p(ne, _f64p)))
        return res, jac, ne

    def refine_poses(self, obj, img_pts, poses, K, counts=None, huber_delta: float = 0.0, max_iterations: int = 20):
        """Motion-only LM over SE(3) -> (poses (P,12), costs (P,), iterations)."""
        obj = _c(obj, np.float64)
        if obj.ndim == 2:
            obj = obj[None]
        P, n = obj.shape[0], obj.shape[1]
        img_pts = _c(img_pts, np.float32).reshape(P, n, 2)
        poses = np.array(poses, np.float64).reshape(P, 12)
        K = _c(K, np.float64).reshape(9)
        cnt = _c(counts, np.int32).reshape(P) if counts is not None else None
        costs = np.empty(P, np.float64)
        it = C.c_int()
        self._check(lib().svo_refine_poses(self.handle, _p(obj, _f64p), _p(img_pts, _f32p),
                                           _p(cnt, _i32p) if cnt is not None else None, P, n, _p(K, _f64p),
                                           float(huber_delta), int(max_iterations), _p(poses, _f64p),
                                           _p(costs, _f64p), C.byref(it)))
        return poses, costs, it.value

    @staticmethod
    def _refine_stereo_args(obj, img_pts, ur, poses, K, counts):
        obj = _c(obj, np.float64)
        if obj.ndim == 2:
            obj = obj[None]
        P, n = obj.shape[0], obj.shape[1]
        img_pts = _c(img_pts, np.float32).reshape(P, n, 2)
        ur = _c(ur, np.float32).reshape(P, n) if ur is not None else None
        poses = np.array(poses, np.float64).reshape(P, 12)
        K = _c(K, np.float64).reshape(9)
        cnt = _c(counts, np.int32).reshape(P) if counts is not None else None
        return P, n, obj, img_pts, ur, poses, K, cnt

    def refine_poses_stereo(self, obj, img_pts, ur, poses, K, baseline, counts=None, huber_delta: float = 0.0,
                            max_iterations: int = 20):
        """Motion-only LM over SE(3) from stereo observations, the whole run of every
        problem in one launch (svo_refine_poses_stereo): obj (P, n, 3) f64, img_pts
        (P, n, 2) f32, ur (P, n) f32 right columns (< 0: a monocular observation),
        poses (P, 12) -> (poses (P, 12), costs (P, 2): initial and final, iterations
        (P,), normal (P, 28): H, g, cost at the returned pose; H is the pose's
        information matrix). max_iterations = 0: the linearisation alone."""
        P, n, obj, img_pts, ur, poses, K, cnt = self._refine_stereo_args(obj, img_pts, ur, poses, K, counts)
        costs = np.zeros((P, 2), np.float64)
        its = np.zeros(P, np.int32)
        ne = np.zeros((P, 28), np.float64)
        self._check(lib().svo_refine_poses_stereo(
            self.handle, _p(obj, _f64p), _p(img_pts, _f32p), _p(ur, _f32p) if ur is not None else None,
            _p(cnt, _i32p) if cnt is not None else None, P, n, _p(K, _f64p), float(baseline), float(huber_delta),
            int(max_iterations), _p(poses, _f64p), _p(costs, _f64p), _p(its, _i32p), _p(ne, _f64p)))
        return poses, costs, its, ne

    def refine_poses_time(self, obj, img_pts, ur, poses, K, baseline, counts=None, huber_delta: float = 0.0,
                          max_iterations: int = 10, reps: int = 10) -> dict:
        """ms per whole LM launch of refine_poses_stereo (HIP events) and, wall time,
        per call of refine_poses on the same pixels from the same poses with the same
        iterations cap (svo_refine_poses_time)."""
        P, n, obj, img_pts, ur, poses, K, cnt = self._refine_stereo_args(obj, img_pts, ur, poses, K, counts)
        ms = np.zeros(2)
        self._check(lib().svo_refine_poses_time(
            self.handle, _p(obj, _f64p), _p(img_pts, _f32p), _p(ur, _f32p) if ur is not None else None,
            _p(cnt, _i32p) if cnt is not None else None, P, n, _p(K, _f64p), float(baseline), float(huber_delta),
            int(max_iterations), _p(poses, _f64p), int(reps), _p(ms[0:], _f64p), _p(ms[1:], _f64p)))
        return {"ms_device": float(ms[0]), "ms_host": float(ms[1])}

    # ---------------------------------------------------------------- pose graph
    @staticmethod
    def _pg_args(poses, fixed, edge_ij, edge_Z, edge_info, n_nodes, n_edges):
        """One problem (poses (N, 12), edges (E, ...)) or a batch (a leading axis P on
        every array) -> the C ABI's arguments; (single, P, N, E, ...)."""
        poses = np.array(poses, np.float64)
        single = poses.ndim == 2
        edge_ij = np.asarray(edge_ij)
        if single:
            poses, edge_ij = poses[None], edge_ij.reshape(1, -1, 2)
        P, N, E = poses.shape[0], poses.shape[1], edge_ij.shape[1]
        poses = np.ascontiguousarray(poses.reshape(P, N, 12))
        fixed = _c(np.asarray(fixed, np.uint8).reshape(P, N), np.uint8)
        edge_ij = _c(edge_ij.reshape(P, E, 2), np.int32)
        edge_Z = _c(np.asarray(edge_Z).reshape(P, E, 12), np.float64)
        edge_info = _c(np.asarray(edge_info).reshape(P, E, 21), np.float64)
        cnt = [None if c is None else _c(np.asarray(c).reshape(P), np.int32) for c in (n_nodes, n_edges)]
        return single, P, N, E, poses, fixed, edge_ij, edge_Z, edge_info, cnt

    def pose_graph_optimize(self, poses, fixed, edge_ij, edge_Z, edge_info, n_nodes=None, n_edges=None,
                            huber_delta: float = 0.0, max_iterations: int = 50, max_cg: int = 1024):
        """Pose-graph optimisation, the whole LM of every problem in one launch
        (svo_pose_graph_optimize): poses (P, N, 12) world -> camera, fixed (P, N)
        bool, edges edge_ij (P, E, 2) int pairs (i, j), edge_Z (P, E, 12) the measured
        T_j T_i^-1, edge_info (P, E, 21) the upper triangle of the 6x6 information
        matrix in the order (rho, phi) -- the first 21 of refine_poses_stereo's normal;
        n_nodes / n_edges: (P,) counts of a ragged batch. One problem may be given
        without the leading axis. -> (poses, costs (P, 2): initial and final,
        iterations (P,), cg_iterations (P,): matrix-vector products of the run).
        max_iterations = 0: the first cost twice, the poses' bits kept."""
        single, P, N, E, poses, fixed, ij, Z, info, cnt = self._pg_args(poses, fixed, edge_ij, edge_Z, edge_info,
                                                                        n_nodes, n_edges)
        costs = np.zeros((P, 2), np.float64)
        its, cgs = np.zeros(P, np.int32), np.zeros(P, np.int32)
        out = poses.copy()
        self._check(lib().svo_pose_graph_optimize(
            self.handle, P, N, E, *[None if c is None else _p(c, _i32p) for c in cnt], _p(poses, _f64p),
            _p(fixed, _u8p), _p(ij, _i32p), _p(Z, _f64p), _p(info, _f64p), float(huber_delta), int(max_iterations),
            int(max_cg), _p(out, _f64p), _p(costs, _f64p), _p(its, _i32p), _p(cgs, _i32p)))
        if single:
            return out[0], costs[0], int(its[0]), int(cgs[0])
        return out, costs, its, cgs

    def pose_graph_linearize(self, poses, fixed, edge_ij, edge_Z, edge_info, n_nodes=None, n_edges=None,
                             huber_delta: float = 0.0) -> dict:
        """The pose graph's first linearisation at the given poses
        (svo_pose_graph_linearize) -> dict of cost (P,), e (P, E, 6), w (P, E), Ji and
        Jj (P, E, 6, 6), node (P, N, 27): each node's 21 + 6 sums; without the leading
        axis for one problem. Entries beyond a problem's counts are zero."""
        single, P, N, E, poses, fixed, ij, Z, info, cnt = self._pg_args(poses, fixed, edge_ij, edge_Z, edge_info,
                                                                        n_nodes, n_edges)
        out = {"cost": np.zeros(P), "e": np.zeros((P, E, 6)), "w": np.zeros((P, E)), "Ji": np.zeros((P, E, 6, 6)),
               "Jj": np.zeros((P, E, 6, 6)), "node": np.zeros((P, N, 27))}
        self._check(lib().svo_pose_graph_linearize(
            self.handle, P, N, E, *[None if c is None else _p(c, _i32p) for c in cnt], _p(poses, _f64p),
            _p(fixed, _u8p), _p(ij, _i32p), _p(Z, _f64p), _p(info, _f64p), float(huber_delta),
            *[_p(out[k], _f64p) for k in ("cost", "e", "w", "Ji", "Jj", "node")]))
        return {k: v[0] for k, v in out.items()} if single else out

    def pose_graph_time(self, poses, fixed, edge_ij, edge_Z, edge_info, n_nodes=None, n_edges=None,
                        huber_delta: float = 0.0, max_iterations: int = 50, max_cg: int = 1024, reps: int = 5) -> dict:
        """ms per whole launch of pose_graph_optimize (HIP events, svo_pose_graph_time)
        with the last launch's iterations and cg_iterations (P,)."""
        single, P, N, E, poses, fixed, ij, Z, info, cnt = self._pg_args(poses, fixed, edge_ij, edge_Z, edge_info,
                                                                        n_nodes, n_edges)
        ms = np.zeros(1)
        its, cgs = np.zeros(P, np.int32), np.zeros(P, np.int32)
        self._check(lib().svo_pose_graph_time(
            self.handle, P, N, E, *[None if c is None else _p(c, _i32p) for c in cnt], _p(poses, _f64p),
            _p(fixed, _u8p), _p(ij, _i32p), _p(Z, _f64p), _p(info, _f64p), float(huber_delta), int(max_iterations),
            int(max_cg), int(reps), _p(ms, _f64p), _p(its, _i32p), _p(cgs, _i32p)))
        return {"ms": float(ms[0]), "iterations": its, "cg_iterations": cgs}

    @staticmethod
    def pose_graph_edge(Ti, Tj) -> np.ndarray:
        """Z = T_j T_i^-1 (12,), the measurement of an edge (i, j) that the two poses
        agree with (svo_pose_graph_edge): the solver's own arithmetic, on the host."""
        Ti, Tj = _c(np.asarray(Ti, np.float64).reshape(12), np.float64), _c(np.asarray(Tj, np.float64).reshape(12), np.float64)
        Z = np.zeros(12)
        if lib().svo_pose_graph_edge(_p(Ti, _f64p), _p(Tj, _f64p), _p(Z, _f64p)) != 0:
            raise SvoError("svo_pose_graph_edge: bad arguments")
        return Z

    # ---------------------------------------------------------------- bundle adjustment
    @staticmethod
    def _ba_args(poses, fixed, points, obs_cam, obs_point, obs_xy, K, n_cams, n_points, n_obs):
        """One problem (poses (C, 12), points (M, 3), obs (O,)) or a batch (a leading
        axis P on every array) -> the C ABI's arguments; (single, P, C, M, O, ...)."""
        poses = np.array(poses, np.float64)
        single = poses.ndim == 2
        if single:
            poses = poses[None]
        P, Cn = poses.shape[0], poses.shape[1]
        poses = np.ascontiguousarray(poses.reshape(P, Cn, 12))
        points = np.array(points, np.float64)
        obs_cam = np.asarray(obs_cam)
        if single:
            points, obs_cam = points[None], obs_cam[None]
        Mn, On = points.shape[1], obs_cam.shape[1]
        points = np.ascontiguousarray(points.reshape(P, Mn, 3))
        fixed = _c(np.asarray(fixed, np.uint8).reshape(P, Cn), np.uint8)
        obs_cam = _c(obs_cam.reshape(P, On), np.int32)
        obs_point = _c(np.asarray(obs_point).reshape(P, On), np.int32)
        obs_xy = _c(np.asarray(obs_xy).reshape(P, On, 2), np.float32)
        K = _c(K, np.float64).reshape(9)
        cnt = [None if c is None else _c(np.asarray(c).reshape(P), np.int32) for c in (n_cams, n_points, n_obs)]
        return single, P, Cn, Mn, On, poses, fixed, points, obs_cam, obs_point, obs_xy, K, cnt

    @staticmethod
    def _ba_stereo(obs_ur, baseline, P, On):
        """The stereo entries' two extra arguments, or None when neither is given."""
        if obs_ur is None and baseline is None:
            return None
        if obs_ur is None or baseline is None:
            raise ValueError("obs_ur and baseline go together")
        return [_p(_c(np.asarray(obs_ur).reshape(P, On), np.float32), _f32p), float(baseline)]

    def bundle_adjust(self, poses, fixed, points, obs_cam, obs_point, obs_xy, K, n_cams=None, n_points=None,
                      n_obs=None, huber_delta: float = 0.0, max_iterations: int = 50, obs_ur=None, baseline=None):
        """Windowed bundle adjustment (svo_bundle_adjust): poses (P, C, 12) world ->
        camera, fixed (P, C) bool, points (P, M, 3), observations obs_cam / obs_point
        (P, O) and obs_xy (P, O, 2) in any order; n_cams / n_points / n_obs: (P,)
        counts of a ragged batch. One problem may be given without the leading axis.
        obs_ur (P, O) with baseline: the right image's column per observation (< 0:
        a monocular observation) of a rectified pair (svo_bundle_adjust_stereo).
        -> (poses, points, costs (P, 2): initial and final, iterations (P,))."""
        single, P, Cn, Mn, On, poses, fixed, points, oc, op, oxy, K, cnt = self._ba_args(
            poses, fixed, points, obs_cam, obs_point, obs_xy, K, n_cams, n_points, n_obs)
        costs = np.zeros((P, 2), np.float64)
        its = np.zeros(P, np.int32)
        stereo = self._ba_stereo(obs_ur, baseline, P, On)
        entry = lib().svo_bundle_adjust if stereo is None else lib().svo_bundle_adjust_stereo
        self._check(entry(
            self.handle, P, Cn, Mn, On, *[None if c is None else _p(c, _i32p) for c in cnt], _p(poses, _f64p),
            _p(fixed, _u8p), _p(points, _f64p), _p(oc, _i32p), _p(op, _i32p), _p(oxy, _f32p), *(stereo or []),
            _p(K, _f64p), float(huber_delta), int(max_iterations), _p(costs, _f64p), _p(its, _i32p)))
        if single:
            return poses[0], points[0], costs[0], int(its[0])
        return poses, points, costs, its

    def ba_linearize(self, poses, fixed, points, obs_cam, obs_point, obs_xy, K, lam: float = 1e-4, n_cams=None,
                     n_points=None, n_obs=None, huber_delta: float = 0.0, obs_ur=None, baseline=None) -> dict:
        """One linearisation and one solve of the bundle adjustment at damping lam
        (svo_ba_linearize) -> dict of U (P, C, 21), gc (P, C, 6), V (P, M, 6), gp
        (P, M, 3), cost (P,), S (P, 6C, 6C), b (P, 6C), dc (P, C, 6), dp (P, M, 3),
        n_free (P,), status (P,); without the leading axis for one problem. obs_ur
        with baseline: svo_ba_linearize_stereo."""
        single, P, Cn, Mn, On, poses, fixed, points, oc, op, oxy, K, cnt = self._ba_args(
            poses, fixed, points, obs_cam, obs_point, obs_xy, K, n_cams, n_points, n_obs)
        out = {"U": np.zeros((P, Cn, 21)), "gc": np.zeros((P, Cn, 6)), "V": np.zeros((P, Mn, 6)),
               "gp": np.zeros((P, Mn, 3)), "cost": np.zeros(P), "S": np.zeros((P, 6 * Cn, 6 * Cn)),
               "b": np.zeros((P, 6 * Cn)), "dc": np.zeros((P, Cn, 6)), "dp": np.zeros((P, Mn, 3))}
        nfree = np.zeros(P, np.int32)
        status = np.zeros(P, np.int32)
        stereo = self._ba_stereo(obs_ur, baseline, P, On)
        entry = lib().svo_ba_linearize if stereo is None else lib().svo_ba_linearize_stereo
        self._check(entry(
            self.handle, P, Cn, Mn, On, *[None if c is None else _p(c, _i32p) for c in cnt], _p(poses, _f64p),
            _p(fixed, _u8p), _p(points, _f64p), _p(oc, _i32p), _p(op, _i32p), _p(oxy, _f32p), *(stereo or []),
            _p(K, _f64p), float(huber_delta), float(lam),
            *[_p(out[k], _f64p) for k in ("U", "gc", "V", "gp", "cost", "S", "b", "dc", "dp")],
            _p(nfree, _i32p), _p(status, _i32p)))
        out["n_free"], out["status"] = nfree, status
        return {k: v[0] for k, v in out.items()} if single else out

    def ba_stage_lists(self, counts, ids, xy, ur=None) -> dict:
        """The bundle adjustment's staging on the device (svo_ba_stage_lists) of
        observations given as sorted lists per camera: counts (P, W), ids (P, W, cap)
        strictly increasing per list, xy (P, W, cap, 2) -> dict of ocam (P, O), oxy
        (P, O, 2), pt_off (P, O + 1), cam_off (P, W + 1), cam_idx, cam_pt, pt_id
        (P, O), n_points, n_obs (P,), O = W * cap. ur (P, W, cap): the right columns
        beside xy, staged as "our" (P, O) (svo_ba_stage_lists_stereo)."""
        counts = _c(counts, np.int32)
        P, W = counts.shape
        ids = _c(ids, np.int32).reshape(P, W, -1)
        cap = ids.shape[2]
        xy = _c(xy, np.float32).reshape(P, W, cap, 2)
        O = W * cap
        out = {"ocam": np.zeros((P, O), np.int32), "oxy": np.zeros((P, O, 2), np.float32),
               "pt_off": np.zeros((P, O + 1), np.int32), "cam_off": np.zeros((P, W + 1), np.int32),
               "cam_idx": np.zeros((P, O), np.int32), "cam_pt": np.zeros((P, O), np.int32),
               "pt_id": np.zeros((P, O), np.int32), "n_points": np.zeros(P, np.int32), "n_obs": np.zeros(P, np.int32)}
        if ur is not None:
            ur = _c(ur, np.float32).reshape(P, W, cap)
            out["our"] = np.zeros((P, O), np.float32)
            self._check(lib().svo_ba_stage_lists_stereo(
                self.handle, P, W, cap, _p(counts, _i32p), _p(ids, _i32p), _p(xy, _f32p), _p(ur, _f32p),
                _p(out["ocam"], _i32p), _p(out["oxy"], _f32p), _p(out["our"], _f32p),
                *[_p(out[k], _i32p) for k in ("pt_off", "cam_off", "cam_idx", "cam_pt", "pt_id", "n_points", "n_obs")]))
            return out
        self._check(lib().svo_ba_stage_lists(
            self.handle, P, W, cap, _p(counts, _i32p), _p(ids, _i32p), _p(xy, _f32p), _p(out["ocam"], _i32p),
            _p(out["oxy"], _f32p), *[_p(out[k], _i32p) for k in ("pt_off", "cam_off", "cam_idx", "cam_pt", "pt_id",
                                                                  "n_points", "n_obs")]))
        return out

    def ba_time_staging(self, counts, ids, xy, reps: int = 20) -> dict:
        """ms of the device staging chain (HIP events) and, wall time, of the host's
        way for the same lists: their download and svo_bundle_adjust's sort + uploads
        (svo_ba_time_staging)."""
        counts = _c(counts, np.int32)
        P, W = counts.shape
        ids = _c(ids, np.int32).reshape(P, W, -1)
        cap = ids.shape[2]
        xy = _c(xy, np.float32).reshape(P, W, cap, 2)
        ms = np.zeros(3)
        self._check(lib().svo_ba_time_staging(self.handle, P, W, cap, _p(counts, _i32p), _p(ids, _i32p),
                                              _p(xy, _f32p), int(reps), _p(ms[0:], _f64p), _p(ms[1:], _f64p),
                                              _p(ms[2:], _f64p)))
        return {"ms_device": float(ms[0]), "ms_host_readback": float(ms[1]), "ms_host_stage": float(ms[2])}

    def ba_time_iteration(self, poses, fixed, points, obs_cam, obs_point, obs_xy, K, lam: float = 1e-4,
                          n_cams=None, n_points=None, n_obs=None, huber_delta: float = 0.0, reps: int = 10) -> float:
        """ms per LM iteration of the bundle adjustment's launch chain (HIP events)."""
        _, P, Cn, Mn, On, poses, fixed, points, oc, op, oxy, K, cnt = self._ba_args(
            poses, fixed, points, obs_cam, obs_point, obs_xy, K, n_cams, n_points, n_obs)
        ms = C.c_double()
        self._check(lib().svo_ba_time_iteration(
            self.handle, P, Cn, Mn, On, *[None if c is None else _p(c, _i32p) for c in cnt], _p(poses, _f64p), _p(fixed, _u8p), _p(points, _f64p),
            _p(oc, _i32p), _p(op, _i32p), _p(oxy, _f32p), _p(K, _f64p), float(huber_delta), float(lam), int(reps),
            C.byref(ms)))
        return ms.value

    def solve_pnp_ransac(self, obj, img_pts, K, iterations: int = 100, reproj_err: float = 8.0,
                         confidence: float = 0.999):
        """cv::solvePnPRansac(..., SOLVEPNP_SQPNP) -> (ok, rvec, tvec, inliers)."""
        obj = _c(obj, np.float64).reshape(-1, 3)
        img_pts = _c(img_pts, np.float32).reshape(-1, 2)
        K = _c(K, np.float64).reshape(9)
        n = len(obj)
        rvec = np.zeros(3, np.float64)
        tvec = np.zeros(3, np.float64)
        inl = np.zeros(max(n, 1), np.int32)
        ninl = C.c_int()
        rc = self._check(lib().svo_solve_pnp_ransac(self.handle, _p(obj, _f64p), _p(img_pts, _f32p), n,
                                                    _p(K, _f64p), int(iterations), float(reproj_err),
                                                    float(confidence), _p(rvec, _f64p), _p(tvec, _f64p),
                                                    _p(inl, _i32p), C.byref(ninl)))
        return rc == 1, rvec, tvec, inl[: ninl.value].copy()


KF_EVERY, KF_REFERENCE = 0, 1  # SVO_KF_EVERY / SVO_KF_REFERENCE


class FrontendConfig(C.Structure):
    """svo_frontend_config (include/svo_gpu.h); defaults = the reference's
    temporal-tracking call (R:src/tracking.cpp:157-165), FAST params
    (R:configs/config.yaml:29-32), solvePnPRansac args (:191-196) and
    features_to_track (R:configs/config.yaml:15). keyframe_rule: KF_EVERY (every
    frame a keyframe topping the set up to n_features; the benchmark) or
    KF_REFERENCE (Tracking::nextFrame's rule, R:src/tracking.cpp:68-69).
    use_orb=1 + orb=OrbParams(...): the keyframe detector is ORB (the shipped
    config, R:configs/config.yaml:19-27) instead of FAST."""
    _fields_ = [
        ("width", C.c_int), ("height", C.c_int), ("n_seq", C.c_int), ("n_frames", C.c_int),
        ("n_features", C.c_int), ("max_level", C.c_int), ("win", C.c_int), ("lk_max_count", C.c_int),
        ("lk_epsilon", C.c_double), ("min_eig", C.c_double), ("lk_flags", C.c_int),
        ("fast_threshold", C.c_int), ("fast_nonmax", C.c_int), ("mask_half", C.c_float),
        ("bucket_size", C.c_int), ("per_bucket", C.c_int), ("pnp_iterations", C.c_int),
        ("pnp_reproj", C.c_float), ("pnp_confidence", C.c_double), ("K", C.c_double * 9),
        ("host_threads", C.c_int), ("timing", C.c_int), ("keyframe_rule", C.c_int), ("features_to_track", C.c_int),
        ("P_left", C.c_float * 12), ("P_right", C.c_float * 12), ("y_threshold", C.c_float),
        ("stereo_win", C.c_int), ("stereo_max_level", C.c_int), ("stereo_max_count", C.c_int),
        ("stereo_epsilon", C.c_double), ("use_orb", C.c_int), ("orb", OrbParams),
    ]

    def __init__(self, width, height, K, n_seq=1, n_frames=2, n_features=2000, P_left=None, P_right=None, **kw):
        """P_left / P_right: the stereo rig's 3x4 projection matrices (KITTI calib P2 /
        P3, R:src/main.cpp:25-32); default K[I|0] and K[I|(-bf, 0, 0)] with the
        synthetic scene's fx * baseline (svo_amd.scene.STEREO_BF)."""
        super().__init__()
        d = dict(max_level=3, win=21, lk_max_count=50, lk_epsilon=1e-3, min_eig=1e-4,
                 lk_flags=LK_GET_MIN_EIGENVALS, fast_threshold=20, fast_nonmax=1, mask_half=10.0,
                 bucket_size=0, per_bucket=0, pnp_iterations=100, pnp_reproj=8.0, pnp_confidence=0.999,
                 host_threads=0, timing=0, keyframe_rule=KF_EVERY, features_to_track=70, y_threshold=40.0,
                 stereo_win=11, stereo_max_level=3,
                 stereo_max_count=30, stereo_epsilon=1e-3, use_orb=0)
        orb = kw.pop("orb", None)
        d.update(kw)
        self.width, self.height, self.n_seq, self.n_frames, self.n_features = width, height, n_seq, n_frames, n_features
        for k, v in d.items():
            setattr(self, k, v)
        self.orb = orb if orb is not None else OrbParams()
        self.K[:] = [float(x) for x in np.asarray(K, np.float64).ravel()]
        if P_left is None or P_right is None:
            from .scene import stereo_projections
            P_left, P_right = stereo_projections(K)
        self.P_left[:] = [float(x) for x in np.asarray(P_left, np.float32).ravel()]
        self.P_right[:] = [float(x) for x in np.asarray(P_right, np.float32).ravel()]


class FrontendStats(C.Structure):
    _fields_ = [("lk_iterations", C.c_int64), ("tracked", C.c_int64), ("inliers", C.c_int64),
                ("added", C.c_int64), ("features", C.c_int64), ("hypotheses", C.c_int64),
                ("host_ms_hyp", C.c_double), ("host_ms_fit", C.c_double), ("host_ms_wait", C.c_double),
                ("keyframes", C.c_int64),
                ("host_ms_wait_post", C.c_double), ("host_ms_wait_score", C.c_double),
                ("host_ms_wait_kf", C.c_double), ("host_ms_enqueue", C.c_double), ("host_ms_step", C.c_double),
                ("ransac_rounds", C.c_int64), ("max_hypotheses", C.c_int64), ("serial_keyframe", C.c_int64),
                ("full_copy", C.c_int64), ("kf_overflow", C.c_int64), ("host_ms_orb", C.c_double),
                ("spec_margin", C.c_int64)]

    def as_dict(self):
        return {k: (float(getattr(self, k)) if k.startswith("host_") else int(getattr(self, k)))
                for k, _ in self._fields_}


PHASES = ["pyramid", "lk", "post_lk", "stereo_lk", "pnp_score", "tail", "fast", "bucket", "append", "pyramid_right"]


class Frontend:
    """Batched tracking loop of Tracking::startStereo (R:src/tracking.cpp:232-276) over
    n_seq independent sequences (svo_frontend_*)."""

    def __init__(self, ctx: Context, cfg: FrontendConfig):
        self.ctx, self.cfg = ctx, cfg
        h = _vp()
        ctx._check(lib().svo_frontend_create(ctx.handle, C.byref(cfg), C.byref(h)))
        self.handle = h
        ctx._deps[h.value] = "frontend"
        self._queued = {}  # ring slot -> (t, lefts, rights) of queue_frames, until upload_wait(t)
        self._rect = None  # (left, right) RectMaps once set_rectification was called: kept alive, the raw size
        _LIVE["frontend"].add(self)

    def _frame_hw(self):
        """(rows, columns) of the frames set_frame / queue_frames take: the raw size once
        rectification is set, else the config's."""
        if self._rect is not None:
            return (self._rect[0].raw_h, self._rect[0].raw_w)
        return (self.cfg.height, self.cfg.width)

    def set_rectification(self, left: RectMaps, right: RectMaps):
        """svo_frontend_set_rectification: from here on set_frame and queue_frames take
        the cameras' raw frames and rectify them on the device with each eye's maps.
        Once, before the first set_frame, queue_frames or init."""
        self.ctx._check(lib().svo_frontend_set_rectification(self.handle, left.handle, right.handle))
        self._rect = (left, right)

    def set_stereo_matcher(self, params: "StereoRowsParams" = None):
        """svo_frontend_set_stereo_matcher: every stereo match of the front end is row
        SAD (Context.stereo_match_rows' rule) with `params` instead of the stereo LK;
        the frames must be rectified. Once, before the first set_frame, queue_frames
        or init."""
        params = params or StereoRowsParams()
        self.ctx._check(lib().svo_frontend_set_stereo_matcher(self.handle, C.byref(params)))
        self._rows = params

    def set_stereo_tracking(self, params: "StereoRowsParams" = None, guide: int = 4):
        """svo_frontend_set_stereo_tracking: every recorded frame matches its tracked
        features in its own right image (Context.stereo_match_rows_guided around the
        feature's disparity one frame ago), so the stereo window holds a right column
        for them too; the frames must be rectified. Once, after
        window_enable(stereo=True) and before init."""
        params = params or StereoRowsParams()
        self.ctx._check(lib().svo_frontend_set_stereo_tracking(self.handle, C.byref(params), int(guide)))
        self._trk = (params, guide)

    def set_frame(self, seq, t, left, right):
        """Stereo pair t of sequence seq: (h, w) grey, or (h, w, 3) BGR converted on the
        device; raw frames of the maps' raw size once rectification is set."""
        left = _c(left, np.uint8)
        right = _c(right, np.uint8)
        if left.shape != right.shape:
            raise SvoError("set_frame: left / right shapes differ")
        if self._rect is not None and left.shape[:2] != self._frame_hw():
            raise SvoError(f"set_frame: raw frames of {self._frame_hw()} expected, got {left.shape}")
        if left.ndim == 3:
            self.ctx._check(lib().svo_frontend_set_frame_bgr(self.handle, seq, t, _p(left, _u8p), _p(right, _u8p),
                                                             3 * left.shape[1]))
            return
        self.ctx._check(lib().svo_frontend_set_frame(self.handle, seq, t, _p(left, _u8p), _p(right, _u8p),
                                                     left.shape[1]))

    def prebuild_pyramids(self):
        self.ctx._check(lib().svo_frontend_prebuild_pyramids(self.handle))

    def queue_frames(self, t, lefts, rights):
        """svo_frontend_queue_frames: frame t of every sequence from host arrays
        (lefts[s], rights[s]: (height, width) grey or (height, width, 3) BGR of the
        config's size, all of one shape), queued as asynchronous H2D copies (see
        include/svo_gpu.h for the ring discipline). The copies read the arrays after
        this call returns: the wrapper keeps them referenced until upload_wait(t) (or
        until ring slot t % n_frames is queued again); their contents must stay
        unchanged until then."""
        S = self.cfg.n_seq
        if len(lefts) != S or len(rights) != S:
            raise SvoError("queue_frames: one left and one right image per sequence")
        a0 = lefts[0]
        hw = self._frame_hw()  # (the raw size once rectification is set)
        if a0.shape not in (hw, hw + (3,)):
            raise SvoError(f"queue_frames: images must be {hw} grey or {hw + (3,)} BGR, got {a0.shape}")
        bgr = a0.ndim == 3
        for a in list(lefts) + list(rights):
            if a.shape != a0.shape or a.dtype != np.uint8 or not a.flags["C_CONTIGUOUS"]:
                raise SvoError("queue_frames: C-contiguous uint8 images of one shape")
        L = (_u8p * S)(*[a.ctypes.data_as(_u8p) for a in lefts])
        R = (_u8p * S)(*[a.ctypes.data_as(_u8p) for a in rights])
        stride = a0.shape[1] * (3 if bgr else 1)
        self.ctx._check(lib().svo_frontend_queue_frames(self.handle, int(t), L, R, stride, int(bgr)))
        # the asynchronous copies read these buffers: hold them until upload_wait(t)
        self._queued[int(t) % max(self.cfg.n_frames, 1)] = (int(t), list(lefts), list(rights))

    def upload_wait(self, t):
        self.ctx._check(lib().svo_frontend_upload_wait(self.handle, int(t)))
        slot = int(t) % max(self.cfg.n_frames, 1)
        held = self._queued.get(slot)
        if held is not None and held[0] == int(t):
            del self._queued[slot]

    def init(self, t0=0):
        self.ctx._check(lib().svo_frontend_init(self.handle, t0))

    def step(self, t) -> FrontendStats:
        st = FrontendStats()
        self.ctx._check(lib().svo_frontend_step(self.handle, t, C.byref(st)))
        return st

    def synchronize(self):
        """Wait for all of the front end's streams and finish the pose fits."""
        self.ctx._check(lib().svo_frontend_synchronize(self.handle))

    def pose(self, seq):
        r = np.zeros(3)
        t = np.zeros(3)
        self.ctx._check(lib().svo_frontend_pose(self.handle, seq, _p(r, _f64p), _p(t, _f64p)))
        return r, t

    def features(self, seq, cap=1 << 16):
        xy = np.empty((cap, 2), np.float32)
        n = C.c_int()
        self.ctx._check(lib().svo_frontend_features(self.handle, seq, _p(xy, _f32p), cap, C.byref(n)))
        return xy[: min(n.value, cap)].copy()

    def map_points(self, seq, cap=1 << 16):
        """World positions of the current features' map points (float64, (n, 3))."""
        xyz = np.empty((cap, 3), np.float64)
        n = C.c_int()
        self.ctx._check(lib().svo_frontend_map_points(self.handle, seq, _p(xyz, _f64p), cap, C.byref(n)))
        return xyz[: min(n.value, cap)].copy()

    def window_enable(self, window, stereo=False):
        """Keep the last `window` (1 .. BA_MAX_CAMS) frames' observations per sequence
        on the device (svo_frontend_window_enable); once, before init. stereo: also
        the right column of the match that created each feature
        (svo_frontend_window_enable_stereo)."""
        enable = lib().svo_frontend_window_enable_stereo if stereo else lib().svo_frontend_window_enable
        self.ctx._check(enable(self.handle, int(window)))
        self._window = int(window)
        self._window_stereo = bool(stereo)

    def window(self, seq):
        """The valid frames of sequence seq's window, oldest first (svo_frontend_window)
        -> dict of frame_t (n,), poses (n, 12) world -> camera, ids and xy: lists of n
        arrays (k,) int32 map ids / (k, 2) float32 pixels; with a stereo window also
        ur: n arrays (k,) float32, the right column in the frame that created the
        feature and -1 in the frames that tracked it (svo_frontend_window_right)."""
        W = getattr(self, "_window", 0) or 1
        cap = (self.cfg.n_features + 63) // 64 * 64
        n = C.c_int()
        ft, cnt = np.zeros(W, np.int32), np.zeros(W, np.int32)
        poses = np.zeros((W, 12), np.float64)
        ids = np.zeros((W, cap), np.int32)
        xy = np.zeros((W, cap, 2), np.float32)
        self.ctx._check(lib().svo_frontend_window(self.handle, int(seq), cap, C.byref(n), _p(ft, _i32p),
                                                  _p(poses, _f64p), _p(cnt, _i32p), _p(ids, _i32p), _p(xy, _f32p)))
        k = n.value
        out = {"frame_t": ft[:k].copy(), "poses": poses[:k].copy(),
               "ids": [ids[j, :cnt[j]].copy() for j in range(k)], "xy": [xy[j, :cnt[j]].copy() for j in range(k)]}
        if getattr(self, "_window_stereo", False):
            out["ur"] = [u[:c].copy() for u, c in zip(self.window_right(seq), cnt[:k])]
        return out

    def window_right(self, seq):
        """(W, cap) float32: the right columns of sequence seq's window in window()'s
        order (svo_frontend_window_right); an error without a stereo window."""
        W = getattr(self, "_window", 0) or 1
        cap = (self.cfg.n_features + 63) // 64 * 64
        ur = np.zeros((W, cap), np.float32)
        self.ctx._check(lib().svo_frontend_window_right(self.handle, int(seq), cap, _p(ur, _f32p)))
        return ur

    def bundle_adjust(self, n_fixed=2, huber_delta=0.0, max_iterations=10, stereo=False):
        """Windowed bundle adjustment of every sequence from its own window, on the
        device (svo_frontend_bundle_adjust): refined points into the map, refined
        poses into the window -> (costs (S, 2): initial and final, iterations (S,),
        sizes (S, 3): frames, points, observations). stereo: with the right columns
        of a stereo window and the rig's baseline (svo_frontend_bundle_adjust_stereo)."""
        S = self.cfg.n_seq
        costs = np.zeros((S, 2), np.float64)
        its = np.zeros(S, np.int32)
        sizes = np.zeros((S, 3), np.int32)
        adjust = lib().svo_frontend_bundle_adjust_stereo if stereo else lib().svo_frontend_bundle_adjust
        self.ctx._check(adjust(self.handle, int(n_fixed), float(huber_delta), int(max_iterations), _p(costs, _f64p),
                               _p(its, _i32p), _p(sizes, _i32p)))
        return costs, its, sizes

    def refine_poses(self, huber_delta=0.0, max_iterations=10):
        """Motion-only refinement of every sequence's newest window frame from its
        stereo observations, on the device (svo_frontend_refine_poses): the refined
        pose goes into the window's newest slot and nowhere else -> (costs (S, 2):
        initial and final, iterations (S,), counts (S,): observations used). A plain
        window gives the monocular run."""
        S = self.cfg.n_seq
        costs = np.zeros((S, 2), np.float64)
        its = np.zeros(S, np.int32)
        cnt = np.zeros(S, np.int32)
        self.ctx._check(lib().svo_frontend_refine_poses(self.handle, float(huber_delta), int(max_iterations),
                                                        _p(costs, _f64p), _p(its, _i32p), _p(cnt, _i32p)))
        return costs, its, cnt

    def places_enable(self, slots, every=1, patch_size=31, pattern=None):
        """svo_frontend_places_enable: keep a ring of `slots` (1 .. PLACES_MAX_SLOTS)
        described records per sequence, one of init's frame and of every `every`-th
        frame after it; once, before init. pattern: (512, 2) int8 or None (the default)."""
        keep, pp = Context._pattern_arg(pattern)  # (keep: the converted array, alive over the call)
        self.ctx._check(lib().svo_frontend_places_enable(self.handle, int(slots), int(every), int(patch_size), pp))
        self._places = int(slots)

    def place(self, seq, slot):
        """One record (svo_frontend_place, a test view; synchronises) -> dict of frame_t
        (-1: none), desc (n, 32) u8, xy (n, 2) f32, xyz (n, 3) f64."""
        cap = (self.cfg.n_features + 63) // 64 * 64
        ft, n = C.c_int(), C.c_int()
        desc = np.zeros((cap, ORB_DESC_BYTES), np.uint8)
        xy = np.zeros((cap, 2), np.float32)
        xyz = np.zeros((cap, 3), np.float64)
        self.ctx._check(lib().svo_frontend_place(self.handle, int(seq), int(slot), C.byref(ft), C.byref(n),
                                                 _p(desc, _u8p), _p(xy, _f32p), _p(xyz, _f64p), cap))
        k = min(n.value, cap)
        return {"frame_t": ft.value, "desc": desc[:k].copy(), "xy": xy[:k].copy(), "xyz": xyz[:k].copy()}

    def places_query(self, t_lo=0, t_hi=(1 << 31) - 1, which=None, ratio_pct=80, cross_check=True, min_pairs=4,
                     out=None):
        """svo_frontend_places_query: the last step's frame against the records of the
        frames in [t_lo, t_hi], for the sequences flagged in `which` (None: all) ->
        dict of per-sequence arrays frame_t (-1: no result), n_pairs, n_inliers, ok,
        rvec (S, 3), tvec (S, 3), slot_pairs (S, slots; -1: not searched), and lists
        pairs / inliers: per sequence the best record's (query index, record index)
        pairs and the RANSAC inliers' indices into them (empty without a result).
        out: such a dict of a former call, whose arrays are written in place (the rows
        of sequences outside `which` keep what they held)."""
        S, slots = self.cfg.n_seq, getattr(self, "_places", 0) or 1
        cap = (self.cfg.n_features + 63) // 64 * 64
        w = None if which is None else _c(np.asarray(which).astype(np.uint8), np.uint8)
        if w is not None and len(w) != S:
            raise SvoError("places_query: one flag per sequence")
        o = out if out is not None else {
            "frame_t": np.full(S, -1, np.int32), "n_pairs": np.zeros(S, np.int32), "n_inliers": np.zeros(S, np.int32),
            "ok": np.zeros(S, np.int32), "rvec": np.zeros((S, 3)), "tvec": np.zeros((S, 3)),
            "slot_pairs": np.full((S, slots), -1, np.int32)}
        pairs = np.zeros((S, cap, 2), np.int32)
        inl = np.zeros((S, cap), np.int32)
        self.ctx._check(lib().svo_frontend_places_query(
            self.handle, None if w is None else _p(w, _u8p), int(t_lo), int(t_hi), int(ratio_pct), int(bool(cross_check)),
            int(min_pairs), _p(o["frame_t"], _i32p), _p(o["n_pairs"], _i32p), _p(o["n_inliers"], _i32p),
            _p(o["ok"], _i32p), _p(o["rvec"], _f64p), _p(o["tvec"], _f64p), _p(o["slot_pairs"], _i32p),
            _p(pairs, _i32p), _p(inl, _i32p), cap))
        hit = [o["frame_t"][s] >= 0 and (w is None or w[s]) for s in range(S)]
        o["pairs"] = [pairs[s, : o["n_pairs"][s]].copy() if hit[s] else np.zeros((0, 2), np.int32) for s in range(S)]
        o["inliers"] = [inl[s, : o["n_inliers"][s]].copy() if hit[s] else np.zeros(0, np.int32) for s in range(S)]
        return o

    def places_widen(self, result, params: "ProjMatchParams" = None, which=None):
        """svo_frontend_places_widen: the second look at places_query's poses. result:
        places_query's return value; every sequence flagged in `which` (None: all) with
        result["frame_t"][s] >= 0 has that frame's record projected under the query's
        pose and matched by match_projected's rules against the last step's frame,
        then solve_pnp_ransac on the widened pairs -> dict of per-sequence arrays
        n_pairs, n_inliers, ok, rvec (S, 3), tvec (S, 3) (zero rows for the sequences
        left out) and lists pairs (query index, record index) / inliers."""
        S = self.cfg.n_seq
        cap = (self.cfg.n_features + 63) // 64 * 64
        params = params or ProjMatchParams()
        w = None if which is None else _c(np.asarray(which).astype(np.uint8), np.uint8)
        if w is not None and len(w) != S:
            raise SvoError("places_widen: one flag per sequence")
        ft = _c(result["frame_t"], np.int32).reshape(-1)
        rv, tv = _c(result["rvec"], np.float64), _c(result["tvec"], np.float64)
        if len(ft) != S or rv.shape != (S, 3) or tv.shape != (S, 3):
            raise SvoError("places_widen: result must be places_query's return value")
        o = {"n_pairs": np.zeros(S, np.int32), "n_inliers": np.zeros(S, np.int32), "ok": np.zeros(S, np.int32),
             "rvec": np.zeros((S, 3)), "tvec": np.zeros((S, 3))}
        pairs = np.zeros((S, cap, 2), np.int32)
        inl = np.zeros((S, cap), np.int32)
        self.ctx._check(lib().svo_frontend_places_widen(
            self.handle, None if w is None else _p(w, _u8p), _p(ft, _i32p), _p(rv, _f64p), _p(tv, _f64p),
            C.addressof(params), _p(o["n_pairs"], _i32p), _p(o["n_inliers"], _i32p), _p(o["ok"], _i32p),
            _p(o["rvec"], _f64p), _p(o["tvec"], _f64p), _p(pairs, _i32p), _p(inl, _i32p), cap))
        o["pairs"] = [pairs[s, : o["n_pairs"][s]].copy() for s in range(S)]
        o["inliers"] = [inl[s, : o["n_inliers"][s]].copy() for s in range(S)]
        return o

    def places_time(self, t_lo=0, t_hi=(1 << 31) - 1, ratio_pct=80, cross_check=True):
        """Measurement only (svo_frontend_places_time) -> (ms of one record, ms of a
        query's device half, the (sequence, record) problems matched)."""
        ms = np.zeros(2, np.float64)
        n = C.c_int()
        self.ctx._check(lib().svo_frontend_places_time(self.handle, int(t_lo), int(t_hi), int(ratio_pct),
                                                       int(bool(cross_check)), _p(ms, _f64p), C.byref(n)))
        return float(ms[0]), float(ms[1]), n.value

    def time_pyramid(self, t, reps=20):
        """ms per pyramid + Scharr launch chain of frame t, timed alone."""
        ms = np.zeros(1)
        self.ctx._check(lib().svo_frontend_time_pyramid(self.handle, int(t), int(reps), _p(ms, _f64p)))
        return float(ms[0])

    def time_ingest(self, t, rectify, reps=20):
        """ms per level-0 write of the left eye (every sequence) from the staging block of
        the last queue_frames, timed alone: the rectifying kernel (rectify=True) or the
        plain copy / conversion kernel (svo_frontend_time_ingest)."""
        ms = np.zeros(1)
        self.ctx._check(lib().svo_frontend_time_ingest(self.handle, int(t), int(bool(rectify)), int(reps),
                                                       _p(ms, _f64p)))
        return float(ms[0])

    def time_fast(self, t, reps=20):
        """ms per FAST detection launch (unmasked, every sequence) of frame t, timed alone."""
        ms = np.zeros(1)
        self.ctx._check(lib().svo_frontend_time_fast(self.handle, int(t), int(reps), _p(ms, _f64p)))
        return float(ms[0])

    def phase_times(self):
        ms = np.zeros(16)
        n = np.zeros(16, np.int64)
        k = lib().svo_frontend_phase_times(self.handle, _p(ms, _f64p), n.ctypes.data_as(C.POINTER(C.c_int64)), 16)
        return {PHASES[i]: (float(ms[i]), int(n[i])) for i in range(k)}

    def reset_times(self):
        lib().svo_frontend_reset_times(self.handle)

    def scharr(self, seq, t, level, w, h):
        """(ix, iy) of frame t's level (w x h) as the fused pyrDown + Scharr pass built
        them (svo_frontend_scharr_level)."""
        ix = np.empty((h, w), np.int16)
        iy = np.empty_like(ix)
        self.ctx._check(lib().svo_frontend_scharr_level(self.handle, int(seq), int(t), int(level),
                                                        ix.ctypes.data_as(C.POINTER(C.c_int16)),
                                                        iy.ctypes.data_as(C.POINTER(C.c_int16)), w))
        return ix, iy

    def pyramid_level(self, seq, t, level, w, h, right=False):
        """Level `level` (w x h) of frame t's left / right pyramid with its stored
        REFLECT_101 border of PYR_PAD pixels (svo_frontend_pyramid_level)."""
        out = np.empty((h + 2 * PYR_PAD, w + 2 * PYR_PAD), np.uint8)
        self.ctx._check(lib().svo_frontend_pyramid_level(self.handle, int(seq), int(t), int(bool(right)), int(level),
                                                         out.ctypes.data_as(C.POINTER(C.c_uint8)), out.shape[1]))
        return out

    def host_cpus(self):
        """CPUs the host pool is pinned to (svo_host_cpu_plan's share of this rank)."""
        cpus = np.zeros(4096, np.int32)
        n = C.c_int(0)
        self.ctx._check(lib().svo_frontend_host_cpus(self.handle, _p(cpus, _i32p), 4096, C.byref(n)))
        return cpus[:n.value].tolist()

    def streams(self):
        """The HIP stream handles (LK, FAST, copies) this front end runs on."""
        arr = (_vp * 3)()
        n = C.c_int(0)
        self.ctx._check(lib().svo_frontend_streams(self.handle, arr, 3, C.byref(n)))
        return [arr[i] for i in range(n.value)]

    def close(self):
        if getattr(self, "handle", None):
            if self.ctx._deps.pop(self.handle.value, None):  # (else the context went first and took it along)
                lib().svo_frontend_destroy(self.handle)  # waits for the front end's streams
            self.handle = None
            self._queued = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FastFeatureDetector:
    """cv::FastFeatureDetector::create(threshold, nonmaxSuppression) (TYPE_9_16),
    as the reference creates it at R:src/tracking.cpp:54-57."""

    def __init__(self, ctx: Context, threshold: int = 20, nonmax_suppression: bool = True):
        self.ctx, self.threshold, self.nonmax = ctx, threshold, nonmax_suppression

    @classmethod
    def create(cls, ctx: Context, threshold: int = 20, nonmax_suppression: bool = True):
        return cls(ctx, threshold, nonmax_suppression)

    def detect(self, img: Image, mask=None) -> np.ndarray:
        return self.ctx.fast_detect(img, self.threshold, self.nonmax, mask)


