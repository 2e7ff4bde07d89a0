"""Motion-only stereo refinement, the parts that need no GPU: the new C symbols
(declared, exported, bound, refusing null handles); the numpy restatement of
tests/pose_refine_reference.py against central differences and, where every
observation is monocular, against test_reproj_gpu's restatement; and the condition
that keeps the GPU trajectory test from comparing nothing: every one of its
scenes has a prefix of clear LM decisions in float64 and longdouble alike."""
import ctypes
import os

import numpy as np
import pytest

import ba_stereo_reference as R
import pose_refine_reference as Q
import svo_amd as S
from test_capi import ROOT, declared_symbols
from test_reproj_gpu import ref_normal

NEW = ["svo_refine_poses_stereo", "svo_refine_poses_time", "svo_frontend_refine_poses"]


def test_header_library_and_binding_carry_the_new_symbols():
    assert set(NEW) <= set(declared_symbols())
    lib = ctypes.CDLL(S.lib_path())
    for name in NEW:
        assert hasattr(lib, name), name
    assert set(NEW) <= set(S.SYMBOLS)
    assert callable(S.Context.refine_poses_stereo) and callable(S.Context.refine_poses_time)
    assert callable(S.Frontend.refine_poses)
    assert "#define SVO_REFINE_MAX_ITERATIONS 1000" in open(os.path.join(ROOT, "include", "svo_gpu.h")).read()


def test_calls_refuse_null_handles():
    """Argument checks that need no device; the checks behind a live context are in
    the GPU tests."""
    lib = S.lib()
    n = [None] * 8
    assert lib.svo_refine_poses_stereo(None, None, None, None, None, 1, 1, None, 0.5, 0.0, 5, *n[:4]) == -1
    assert lib.svo_refine_poses_time(None, None, None, None, None, 1, 1, None, 0.5, 0.0, 5, None, 3, None, None) == -1
    assert lib.svo_frontend_refine_poses(None, 0.0, 5, None, None, None) == -1


def test_jacobian_rows_match_central_differences():
    """All three rows of the restatement's pose Jacobian (left perturbation) against
    central differences of ba_stereo_reference.predict, h = 1e-6, at
    test_reproj_gpu's finite-difference bars (rtol 1e-5, atol 1e-4)."""
    X, xy, ur, T = Q.stereo_scene(200, 2)
    front, stereo, r, w, c, Jc = Q.terms(T, X, xy, ur, Q.BASELINE, 0.0)
    assert np.all(front) and stereo.sum() > 50 and (~stereo).sum() > 50
    h = 1e-6
    for n in range(len(X)):
        fd = np.zeros((3, 6))
        for k in range(6):
            e = np.zeros(6)
            e[k] = h
            fd[:, k] = (R.predict(Q.left_update(T, e), X[n], Q.BASELINE) -
                        R.predict(Q.left_update(T, -e), X[n], Q.BASELINE)) / (2 * h)
        rows = 3 if stereo[n] else 2
        assert np.allclose(Jc[n, :rows], fd[:rows], rtol=1e-5, atol=1e-4), n
        assert stereo[n] or (np.all(Jc[n, 2] == 0) and r[n, 2] == 0)
        want = R.predict(T, X[n], Q.BASELINE) - np.r_[xy[n], ur[n]].astype(np.float64)
        assert np.allclose(r[n, :rows], want[:rows], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_all_monocular_equals_the_reprojection_restatement(delta):
    """ur all negative: the 28 sums are test_reproj_gpu.ref_normal's, at the bar the
    two restatements' different summation orders allow (rtol 1e-12)."""
    X, xy, _, T = Q.stereo_scene(300, 5, noise=0.5, outliers=0.2)
    T0 = Q.left_update(T, np.r_[0.05, -0.02, 0.1, 0.003, -0.002, 0.001])
    for fill in (-1.0, -7.5):
        got = Q.linearize(T0, X, xy, np.full(len(X), fill, np.float32), delta=delta)
        _, _, want = ref_normal(T0, X, xy, delta)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-9), fill


def test_points_behind_the_camera_add_nothing():
    X, xy, ur, T = Q.stereo_scene(64, 6, noise=0.5)
    Xb = X.copy()
    Xb[5] = T[:9].reshape(3, 3).T @ (np.array([0.3, -0.2, -3.0]) - T[9:])
    keep = np.arange(64) != 5
    # (numpy sums the two lists in different blocks: equal up to rounding)
    assert np.allclose(Q.linearize(T, Xb, xy, ur, delta=2.0), Q.linearize(T, X[keep], xy[keep], ur[keep], delta=2.0),
                       rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", list(Q.TRAJECTORY))
def test_trajectory_scenes_have_a_prefix_of_clear_decisions(name):
    """K >= 3 iterations whose verdicts float64 and longdouble share and rounding
    cannot change; the rough starts reject at least three steps inside it; and the
    two precisions' costs agree to 1e-12 throughout, a hundredth of the GPU test's
    bar of 1e-10, so that bar is one a correct float64 kernel can meet."""
    X, xy, ur, T, T0, delta = Q.trajectory_case(name)
    assert np.sum(ur >= 0) >= 0.3 * len(ur) and np.sum(ur < 0) >= 0.3 * len(ur)
    K, h64, hld, r64, rld = Q.lm_prefix(T0, X, xy, ur, delta=delta, max_iterations=Q.TRAJECTORY_ITERATIONS)
    pattern = "".join(h["event"][0] for h in h64[:K])
    print(name, "K", K, pattern, "iterations", r64[2], "cost", r64[1])
    assert K >= 3
    if name.endswith("rough"):
        assert pattern.count("r") >= 3 and pattern.count("a") >= 4
    for a, b in zip(h64[:K], hld[:K]):
        assert abs(a["cost"] - float(b["cost"])) <= 1e-12 * abs(a["cost"])


def test_restatement_reaches_the_truth_on_exact_data():
    X, xy, ur, T = Q.stereo_scene(40, 1)
    pose, (c0, c1), it, ne = Q.lm(Q.start_pose(T, 1, 0.5, 0.05), X, xy, ur, max_iterations=50)
    assert np.abs(pose - T).max() < 1e-5 and c1 < 1e-6 * len(X) and 1 < it < 50
    # the information matrix at the solution: stereo adds sum J2^T J2 to it
    mono = Q.linearize(pose, X, xy, np.full(len(X), -1, np.float32))
    _, stereo, _, w, _, Jc = Q.terms(pose, X, xy, ur, Q.BASELINE, 0.0)
    add = np.einsum("n,ni,nj->ij", w * stereo, Jc[:, 2], Jc[:, 2])[Q.TRIU6]
    assert np.allclose(ne[:21] - mono[:21], add, rtol=1e-10, atol=1e-6) and np.all(add[[0, 6, 11, 15, 18, 20]] >= 0)
