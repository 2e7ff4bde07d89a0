"""Stereo observations in the bundle adjustment, the parts that need no GPU: the
numpy restatement of tests/ba_stereo_reference.py against central differences,
against ba_reference where every observation is monocular and against a dense
solve; the rule that counts a stereo observation as two views; the scenes the
GPU tests build on, judged by numpy alone; and the new C symbols (declared,
exported, bound, refusing null handles)."""
import ctypes

import numpy as np

import ba_reference as B
import ba_stereo_reference as R
import svo_amd as S
from test_capi import declared_symbols

LAM = 1e-4
NEW = ["svo_bundle_adjust_stereo", "svo_ba_linearize_stereo", "svo_ba_stage_lists_stereo",
       "svo_frontend_window_enable_stereo", "svo_frontend_window_right", "svo_frontend_bundle_adjust_stereo"]


def test_stereo_rows_match_central_differences():
    """Jc (3 x 6, left perturbation) and Jp (3 x 3) of every stereo observation of
    a parity case against central differences of (u, v, ur), h = 1e-6, at
    test_reproj_gpu's finite-difference tolerances (rtol 1e-5, atol 1e-4)."""
    q = R.parity_case(4, 64, 3)
    front, stereo, r, w, c, Jc, Jp = R.obs_terms(q["poses"], q["points"], q["obs_cam"], q["obs_point"], q["obs_xy"],
                                                 q["obs_ur"], q["baseline"], 0.0)
    h, b = 1e-6, q["baseline"]
    rows = np.flatnonzero(stereo & front)
    assert len(rows) > 50
    for n in rows:
        T, X = q["poses"][q["obs_cam"][n]], q["points"][q["obs_point"][n]]
        assert np.allclose(r[n], R.predict(T, X, b) - np.r_[q["obs_xy"][n], q["obs_ur"][n]].astype(np.float64),
                           rtol=1e-12, atol=1e-9)
        for k in range(6):
            e = np.zeros(6)
            e[k] = h
            fd = (R.predict(B.left_update(T, e), X, b) - R.predict(B.left_update(T, -e), X, b)) / (2 * h)
            assert np.allclose(Jc[n, :, k], fd, rtol=1e-5, atol=1e-4), (n, k)
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            fd = (R.predict(T, X + e, b) - R.predict(T, X - e, b)) / (2 * h)
            assert np.allclose(Jp[n, :, k], fd, rtol=1e-5, atol=1e-4), (n, k)
    # a monocular observation has no third row
    mono = np.flatnonzero(~stereo)
    assert len(mono) > 50 and np.all(Jc[mono, 2] == 0) and np.all(Jp[mono, 2] == 0) and np.all(r[mono, 2] == 0)


def test_all_monocular_equals_the_monocular_restatement():
    for k, (Cn, M) in enumerate(B.PARITY_SHAPES):
        for delta, outl in ((0.0, 0.0), (2.0, 0.2)):
            q = R.parity_case(Cn, M, 10 + k, outl)
            q["obs_ur"] = np.full(len(q["obs_cam"]), -1.0, np.float32)
            a, b = R.linearize(q, LAM, delta), B.linearize(R.mono(q), LAM, delta)
            for key in ("U", "gc", "V", "gp", "cost", "S", "b", "dc", "dp", "pt_cnt", "pt_free"):
                assert np.array_equal(a[key], b[key]), (Cn, M, delta, key)


def test_elimination_equals_the_dense_solve():
    for delta, outl in ((0.0, 0.0), (2.0, 0.2)):
        q = R.parity_case(5, 65, 14, outl)
        L = R.linearize(q, LAM, delta)
        dc, dp = R.dense_step(q, LAM, delta)
        assert np.abs(dc - L["dc"]).max() <= 1e-9 * np.abs(dc).max()
        assert np.abs(dp - L["dp"]).max() <= 1e-9 * np.abs(dp).max()


def test_counting_rule():
    """A stereo observation in front of its camera counts as two views; within a
    (point, camera) run of duplicates: one, plus one if any of them is stereo."""
    want = {"one stereo observation": (2, True), "one monocular observation": (1, False),
            "monocular + stereo duplicates by one camera": (2, True),
            "stereo + monocular duplicates by one camera": (2, True),
            "stereo observation behind the camera": (0, False)}
    cases = R.counting_cases()
    assert set(cases) == set(want)
    for name, (q, free) in cases.items():
        L = R.linearize(q, LAM)
        assert (L["pt_cnt"][0], bool(L["pt_free"][0])) == want[name] and free == want[name][1], name
        assert np.all(L["pt_free"][1:]) and bool(np.any(L["dp"][0] != 0)) == free, name
    L = R.linearize(R.single_stereo(), LAM)
    assert L["n_free"] == 0 and L["pt_free"][0] and np.any(L["dp"][0] != 0)
    L = R.linearize(R.boundary_duplicates(), LAM)
    assert list(L["pt_cnt"][[3, 4, 7, 8]]) == [2, 2, 2, 2] and np.all(L["pt_free"])


def test_single_view_points_need_the_stereo_term():
    """The scene of test_bundle_adjust_stereo_gpu's purpose test, by numpy alone: the
    monocular LM leaves the points created at the last camera where they start
    (median 0.54 m off) and ends at cost 58.3; the stereo LM ends at cost 3.5e-8
    with those points 1.4e-5 m (median; largest 1.5e-4 m) and the poses 2.2e-7
    from the truth."""
    truth, start, new = R.newest_keyframe_scene(seed=0)
    assert len(new) >= 30
    Pm, Xm, cm, _ = B.lm(R.mono(start), 0.0, 50)
    assert np.array_equal(Xm[new], start["points"][new]) and cm[1] > 10
    P, X, c, it = R.lm(start, 0.0, 50)
    err = np.linalg.norm(X - truth["points"], axis=1)[new]
    err0 = np.linalg.norm(start["points"] - truth["points"], axis=1)[new]
    print(f"stereo: cost {c[0]:.3e} -> {c[1]:.3e} in {it}, new points median {np.median(err):.2e} max {err.max():.2e}"
          f" (start {np.median(err0):.2e}), poses {np.abs(P - truth['poses']).max():.2e}; monocular cost {cm[1]:.3e}")
    assert np.median(err0) > 0.1 and np.median(err) < 1e-4 and np.abs(P - truth["poses"]).max() < 1e-6
    assert c[1] <= 1e-6 * len(truth["obs_cam"])


def noisy_scene():
    """6 cameras stepping 0.8 m along z, 120 points, 0.5 px noise on all three
    coordinates, every observation stereo; two fixed cameras, the usual start."""
    truth = R.stereo_window_scene(C=6, M=120, seed=2, mono_fraction=0.0, noise=0.5, min_obs=2)
    return truth, B.perturbed(truth, 3)


def test_stereo_halves_the_point_error_under_noise():
    """numpy alone: median point error 0.110 m after the stereo LM, 0.311 m after
    the monocular one (factor 2.8) on noisy_scene()."""
    truth, start = noisy_scene()
    _, X, c, _ = R.lm(start, 0.0, 30)
    _, Xm, cm, _ = B.lm(R.mono(start), 0.0, 30)
    es = np.median(np.linalg.norm(X - truth["points"], axis=1))
    em = np.median(np.linalg.norm(Xm - truth["points"], axis=1))
    print(f"median point error: stereo {es:.3f} m, monocular {em:.3f} m")
    assert em >= 2 * es


def test_header_library_and_binding_carry_the_new_symbols():
    assert set(NEW) <= set(declared_symbols())
    lib = ctypes.CDLL(S.lib_path())
    for name in NEW:
        assert hasattr(lib, name), name
    assert set(NEW) <= set(S.SYMBOLS)
    assert callable(S.Frontend.window_right)


def test_calls_refuse_null_handles():
    """Argument checks that need no device (test_window_capi_cpu's way); the checks
    behind a live context are in the GPU tests."""
    lib = S.lib()
    n = [None] * 16
    assert lib.svo_bundle_adjust_stereo(None, 1, 1, 1, 1, *n[:9], None, 0.5, None, 0.0, 5, None, None) == -1
    assert lib.svo_ba_linearize_stereo(None, 1, 1, 1, 1, *n[:9], None, 0.5, None, 0.0, 1e-4, *n[:11]) == -1
    assert lib.svo_ba_stage_lists_stereo(None, 1, 1, 1, *n[:14]) == -1
    assert lib.svo_frontend_window_enable_stereo(None, 4) == -1
    assert lib.svo_frontend_window_right(None, 0, 0, None) == -1
    assert lib.svo_frontend_bundle_adjust_stereo(None, 2, 0.0, 5, None, None, None) == -1
