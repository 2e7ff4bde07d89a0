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


# ---------------------------------------------------------------- the scenes of test_bundle_adjust_paths_gpu
# Each has the property its GPU test relies on. The device's constants: 256
# threads per camera block, 512 per elimination block, 4 points staged per pass,
# 256 points per block of the point kernels, kMaxNS = 4656 packed entries.

@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_unreached_shapes_are_what_they_claim(delta):
    outl = 0.2 if delta else 0.0
    robust = lambda q: np.linalg.norm(B.obs_terms(q["poses"], q["points"], q["obs_cam"], q["obs_point"],  # noqa: E731
                                                  q["obs_xy"], delta)[1], axis=1) > delta
    # dense duplicates: both strided second passes, runs of 70
    q = B.dense_duplicates(0, outl)
    L = B.linearize(q, 1e-4, delta)
    assert q["fixed"].tolist() == [1, 0] and np.bincount(q["obs_cam"]).tolist() == [350, 350]  # > 256 per camera
    assert (q["obs_point"] < 4).sum() == 560  # > 512 among the four points of the first staging pass
    pairs = q["obs_point"].astype(int) * 2 + q["obs_cam"]
    assert np.bincount(pairs).tolist() == [70] * 10
    assert L["status"] == 0 and L["n_free"] == 1 and L["pt_free"].all() and np.all(L["pt_cnt"] == 2)
    assert np.all(np.abs(L["dp"]).max(1) > 0)
    # the duplicates are not sorted as they come: the staging has something to do
    assert np.any(np.diff(pairs) < 0)
    # sparse duplicates: point 0 seen twice by camera 1 alone, point 1 twice by camera 1 and once by camera 2
    q = B.sparse_duplicates(0, outl)
    oc, op = q["obs_cam"], q["obs_point"]
    assert q["fixed"].tolist() == [1, 0, 0]
    assert sorted(oc[op == 0].tolist()) == [1, 1] and sorted(oc[op == 1].tolist()) == [1, 1, 2]
    a, b = q["obs_xy"][op == 0]
    assert np.abs(a - b).max() == 0.5
    assert all(np.bincount(oc[op == i], minlength=3).tolist() == [1, 1, 1] for i in range(2, 20))
    L = B.linearize(q, 1e-4, delta)
    old = B.linearize(q, 1e-4, delta, count_observations=True)
    assert L["status"] == 0 and L["pt_cnt"][0] == 1 and not L["pt_free"][0] and np.all(L["dp"][0] == 0)
    assert L["pt_cnt"][1] == 2 and L["pt_free"][1] and np.abs(L["dp"][1]).max() > 1e-3
    # the rule this replaced calls point 0 free and moves it by centimetres: the case tells the rules apart
    assert old["pt_cnt"][0] == 2 and old["pt_free"][0] and np.linalg.norm(old["dp"][0]) > 1e-2
    # wide camera: a second strided pass without duplicates, two blocks of points
    q = B.wide_camera(0, outl)
    assert np.bincount(q["obs_cam"]).tolist() == [300, 300] and len(q["points"]) > 256
    assert len(set(zip(q["obs_cam"].tolist(), q["obs_point"].tolist()))) == 600
    assert B.linearize(q, 1e-4, delta)["status"] == 0
    # full system: 16 free cameras, the last packed entry
    q = B.full_system(0, outl)
    L = B.linearize(q, 1e-4, delta)
    assert L["n_free"] == 16 == S.BA_MAX_CAMS and L["status"] == 0
    assert L["S"].shape == (96, 96) and 96 * 97 // 2 == 4656
    if delta:  # Huber has both branches to take in every shape
        for q in (B.dense_duplicates(0, outl), B.sparse_duplicates(0, outl), B.wide_camera(0, outl), q):
            assert 0.05 < robust(q).mean() < 0.95


def test_on_axis_system_is_exactly_singular():
    q = B.on_axis()
    for dt in (np.float64, np.longdouble):
        for lam in (0.0, 1e-4, 1.0, 1e15):
            L = B.linearize(q, lam, 0.0, dt)
            assert L["status"] == 1 and L["n_free"] == 1 and not L["pt_free"][0]
            assert np.all(L["S"][[2, 5]] == 0) and np.all(L["S"][:, [2, 5]] == 0) and L["S"][0, 0] > 0 < L["S"][1, 1]
            assert np.all(L["dc"] == 0) and np.all(L["dp"] == 0)
    hist = []
    poses, points, (c0, c1), it = B.lm(q, history=hist)
    assert it == 1 and c0 == c1 > 0 and np.array_equal(poses, q["poses"]) and np.array_equal(points, q["points"])
    assert [h["event"] for h in hist] == ["give up"] and hist[0]["retries"] == 20  # 1e-4 -> 1e16
    # Huber changes the weight, not the zeros
    assert B.linearize(q, 1e-4, 1.5)["status"] == 1


@pytest.mark.parametrize("scene", B.REJECT_SCENES)
def test_reject_scenes_reject_clearly(scene):
    """The trajectory test's conditions on its scenes: a prefix of K >= 8
    iterations in which float64 and longdouble decide alike with a margin of 1e-6,
    at least 3 rejections in it, no lambda retries (the device would take them in
    the same iteration, but the scenes do not rely on it)."""
    Cn, M, seed, dpos, delta = scene
    q = B.reject_scene(Cn, M, seed, dpos)
    assert q["fixed"].tolist() == [1, 1] + [0] * (Cn - 2)
    K, h64, hld = B.lm_prefix(q, delta, B.REJECT_ITERATIONS)
    events = [h["event"] for h in h64[:K]]
    assert K >= 8 and events.count("reject") >= 3 and events == [h["event"] for h in hld[:K]]
    assert all(h["retries"] == 0 for h in h64[:K])
    assert all(abs(h["c_trial"] - h["c_cur"]) > 1e-6 * h["c_cur"] for h in h64[:K] + hld[:K])
    # a rejected step leaves the cost where it was, an accepted one lowers it
    for h in h64[:K]:
        assert h["cost"] == h["c_cur"] if h["event"] == "reject" else h["cost"] == h["c_trial"] < h["c_cur"]
    # the two precisions stay close over the prefix: the bars of the GPU test are small
    assert max(abs(a["cost"] - b["cost"]) / abs(b["cost"]) for a, b in zip(h64[:K], hld[:K])) < 1e-6
    # lm's float64 path is the one it always was: max_iterations = k gives the history's k-th cost
    _, _, (c0, ck), it = B.lm(q, delta, max_iterations=5)
    assert it == 5 and ck == h64[4]["cost"] and c0 == h64[0]["c_cur"]


@pytest.mark.parametrize("kind", list(B.POISONED))
def test_poisoned_problems_hold_one_bad_value(kind):
    good, bad = B.healthy(2), B.poisoned(kind)
    n_bad = sum(int((~np.isfinite(np.asarray(bad[k], np.float64))).sum()) for k in ("poses", "points", "obs_xy"))
    assert n_bad == 1 and all(np.all(np.isfinite(good[k])) for k in ("poses", "points", "obs_xy"))
    assert good["fixed"].tolist() == [1, 1, 0, 0, 0]
    with np.errstate(all="ignore"):
        cost = B.total_cost(bad["poses"], bad["points"], bad["obs_cam"], bad["obs_point"], bad["obs_xy"],
                            B.POISONED[kind])
    # the Pz <= 0 rule hides a NaN depth: these costs are finite, and only a look at the inputs finds them
    assert np.isfinite(cost) == (kind in ("nan pose depth", "nan point"))
    if kind == "inf observation":
        assert np.isposinf(cost)


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
