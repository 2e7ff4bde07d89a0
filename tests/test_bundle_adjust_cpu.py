"""Windowed bundle adjustment, the parts that need no GPU: the numpy yardstick
the GPU tests rest on (tests/ba_reference.py) against a dense solve of the full
damped system, the observation staging of the library (host code) on a
hand-written case, and the refusal to run without a device."""
import ctypes

import numpy as np
import pytest

import ba_reference as B
import svo_amd as S


@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_schur_step_equals_dense_solve_of_the_full_system(delta):
    prob = B.perturbed(B.window_scene(C=5, M=65, seed=3, noise=0.5, outliers=0.2 if delta else 0.0), seed=4)
    # a point with one observation and a point with none stay out of both systems
    keep = ~((prob["obs_point"] == 7) | ((prob["obs_point"] == 9) & (prob["obs_cam"] != 2)))
    for k in ("obs_cam", "obs_point", "obs_xy"):
        prob[k] = prob[k][keep]
    L = B.linearize(prob, 1e-4, delta)
    dc, dp = B.dense_step(prob, 1e-4, delta)
    assert L["status"] == 0 and L["n_free"] == 3
    assert not L["pt_free"][7] and not L["pt_free"][9] and L["pt_free"].sum() >= 60
    assert np.abs(L["dc"] - dc).max() <= 1e-9 * np.abs(dc).max()
    assert np.abs(L["dp"] - dp).max() <= 1e-9 * np.abs(dp).max()
    assert np.all(L["dp"][[7, 9]] == 0)


def test_numpy_lm_converges_on_the_window_scene():
    """6 cameras, 300 points, two fixed cameras. Every point keeps two
    observations: one seen once is held constant at its perturbed depth and, seen
    from another place than the first camera, leaves a residual no pose can remove
    (a cost floor of 0.35 here without min_obs)."""
    truth = B.window_scene(C=6, M=300, seed=0, min_obs=2)
    poses, points, (c0, c1), it = B.lm(B.perturbed(truth, seed=1), max_iterations=50)
    n_obs = len(truth["obs_cam"])
    assert it <= 50 and c0 > 1e3 and c1 <= 1e-6 * n_obs
    assert np.abs(poses - truth["poses"]).max() < 1e-5
    assert np.median(np.linalg.norm(points - truth["points"], axis=1)) < 1e-3


def sort_native(cam, pt, C, M):
    cam, pt = np.ascontiguousarray(cam, np.int32), np.ascontiguousarray(pt, np.int32)
    n = len(cam)
    order, cam_idx = np.zeros(n, np.int32), np.zeros(n, np.int32)
    pt_off, cam_off = np.zeros(M + 1, np.int32), np.zeros(C + 1, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    rc = S.lib().svo_ba_sort_observations(*[a.ctypes.data_as(ip) for a in (cam, pt)], n, C, M,
                                          *[a.ctypes.data_as(ip) for a in (order, pt_off, cam_off, cam_idx)])
    return rc, order, pt_off, cam_off, cam_idx


def test_observation_staging_on_a_hand_written_case():
    """3 cameras, 4 points (point 2 unseen, point 1 seen twice by camera 0): sorted
    by (point, camera), ties in the caller's order."""
    #      k:  0  1  2  3  4  5  6
    cam = [2, 0, 1, 0, 0, 2, 1]
    pt = [3, 1, 0, 3, 1, 0, 3]
    rc, order, pt_off, cam_off, cam_idx = sort_native(cam, pt, 3, 4)
    assert rc == 0
    # staged: (p0,c1)=k2 (p0,c2)=k5 (p1,c0)=k1 (p1,c0)=k4 (p3,c0)=k3 (p3,c1)=k6 (p3,c2)=k0
    assert order.tolist() == [2, 5, 1, 4, 3, 6, 0]
    assert pt_off.tolist() == [0, 2, 4, 4, 7]
    assert cam_off.tolist() == [0, 3, 5, 7]
    assert cam_idx.tolist() == [2, 3, 4, 0, 5, 1, 6]
    ro, rp, rc_, ri = B.sort_observations(cam, pt, 3, 4)
    assert ro.tolist() == order.tolist() and rp.tolist() == pt_off.tolist()
    assert rc_.tolist() == cam_off.tolist() and ri.tolist() == cam_idx.tolist()
    # a random case against the numpy restatement, and an index out of range
    rng = np.random.default_rng(0)
    cam, pt = rng.integers(0, 7, 500), rng.integers(0, 40, 500)
    rc, order, pt_off, cam_off, cam_idx = sort_native(cam, pt, 7, 40)
    ref = B.sort_observations(cam, pt, 7, 40)
    assert rc == 0 and all(np.array_equal(a, b) for a, b in zip((order, pt_off, cam_off, cam_idx), ref))
    assert sort_native([0, 3], [0, 0], 3, 1)[0] == -1  # SVO_ERR_ARG


def test_bundle_adjust_fails_loudly_without_device():
    if S.lib().svo_ctx_create(0, ctypes.byref(ctypes.c_void_p())) == 0:
        pytest.skip("a HIP device is present")
    prob = B.window_scene(C=2, M=4, seed=0, drop=0.0)
    with pytest.raises(S.SvoError):
        S.Context(0).bundle_adjust(prob["poses"], prob["fixed"], prob["points"], prob["obs_cam"],
                                   prob["obs_point"], prob["obs_xy"], B.K)
    assert "svo_bundle_adjust" in S.SYMBOLS and "svo_ba_linearize" in S.SYMBOLS
    assert hasattr(S.Context, "bundle_adjust") and hasattr(S.Context, "ba_linearize")
