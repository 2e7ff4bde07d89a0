"""Windowed bundle adjustment on the device (svo_bundle_adjust, svo_ba_linearize,
Tracking.bundle_adjust) against the independent numpy restatement of
tests/ba_reference.py. The reference project has no back end to compare with
(Map::run is an empty loop), so the yardsticks are numpy, central differences
and the truth of synthetic scenes."""
import ctypes as C

import numpy as np
import pytest

import ba_reference as B
import svo_amd as S

pytestmark = pytest.mark.gpu

LAM = 1e-4


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def call(ctx, fn, q, **kw):
    return fn(q["poses"], q["fixed"], q["points"], q["obs_cam"], q["obs_point"], q["obs_xy"], B.K,
              n_cams=q.get("n_cams"), n_points=q.get("n_points"), n_obs=q.get("n_obs"), **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def parity_refs():
    """Per Huber setting: the problems, their numpy linearisation and the measured
    float64-vs-longdouble rounding of S, b, dc, dp (computed once)."""
    out = {}
    for delta, outl in ((0.0, 0.0), (2.0, 0.2)):
        probs = [B.parity_case(Cn, M, 10 + k, outl) for k, (Cn, M) in enumerate(B.PARITY_SHAPES)]
        out[delta] = (probs, [B.linearize(q, LAM, delta) for q in probs],
                      [B.rounding_error(q, LAM, delta) for q in probs])
    return out


@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_linearisation_matches_numpy(ctx, parity_refs, delta):
    """U, gc, V, gp, cost at the bar of test_reproj_gpu's normal equations (rtol
    1e-10, atol 1e-6). S, b, dc, dp pass through V*^-1: their bar is 100 x the
    distance of the float64 numpy restatement from the same computation in
    np.longdouble on these inputs, relative to the largest entry. Measured on the
    CPU (Huber off / delta = 2), largest over the five shapes: S 1.0e-12 / 2.0e-13,
    b 9.5e-13 / 1.6e-13, dc 6.0e-9 / 4.3e-10 (all at (2, 1): one free camera seen
    through one point), dp 6.2e-11 / 9.2e-12; at (16, 300): S 2.4e-15, b 7.6e-15,
    dc 1.6e-13, dp 1.3e-13. Bars: 100 x each, per shape. The MI355X lies at
    (16, 300): S 2.4e-15, dc 2.2e-13; at (2, 1), delta = 2: dc 1.1e-9."""
    probs, refs, errs = parity_refs[delta]
    q = B.batch(probs)
    got = call(ctx, ctx.ba_linearize, q, lam=LAM, huber_delta=delta)
    for p, (prob, ref, err) in enumerate(zip(probs, refs, errs)):
        Cn, M, n = len(prob["poses"]), len(prob["points"]), 6 * ref["n_free"]
        assert got["n_free"][p] == ref["n_free"] and got["status"][p] == ref["status"] == 0
        for k, cnt in (("U", Cn), ("gc", Cn), ("V", M), ("gp", M)):
            d = np.abs(got[k][p, :cnt] - ref[k]).max()
            print(f"delta={delta} shape={B.PARITY_SHAPES[p]} {k}: max abs diff {d:.3e}")
            assert np.allclose(got[k][p, :cnt], ref[k], rtol=1e-10, atol=1e-6), (p, k)
            assert np.all(got[k][p, cnt:] == 0)
        assert np.isclose(got["cost"][p], ref["cost"], rtol=1e-10, atol=1e-6)
        view = {"S": got["S"][p, :n, :n], "b": got["b"][p, :n], "dc": got["dc"][p, :Cn], "dp": got["dp"][p, :M]}
        for k, g in view.items():
            bar = 100 * err[k]
            d = np.abs(g - ref[k]).max() / np.abs(ref[k]).max()
            print(f"delta={delta} shape={B.PARITY_SHAPES[p]} {k}: rel diff {d:.3e} bar {bar:.3e}")
            assert d <= bar, (p, k, d, bar)
        assert np.all(got["S"][p, n:] == 0) and np.all(got["S"][p, :, n:] == 0)
        # constant points do not move: none, one, or one usable observation
        if M >= 63:
            assert np.all(got["dp"][p, [10, 11]] == 0) and ref["pt_cnt"][10] == 0 and ref["pt_cnt"][11] <= 1
    # the same bits on a repeat and with the observations in another order
    again = call(ctx, ctx.ba_linearize, q, lam=LAM, huber_delta=delta)
    rng = np.random.default_rng(5)
    sh = dict(q)
    sh["obs_cam"], sh["obs_point"], sh["obs_xy"] = q["obs_cam"].copy(), q["obs_point"].copy(), q["obs_xy"].copy()
    for p, prob in enumerate(probs):
        perm = rng.permutation(len(prob["obs_cam"]))
        for k in ("obs_cam", "obs_point", "obs_xy"):
            sh[k][p, :len(perm)] = q[k][p, :len(perm)][perm]
    shuffled = call(ctx, ctx.ba_linearize, sh, lam=LAM, huber_delta=delta)
    for k in ("U", "gc", "V", "gp", "cost", "S", "b", "dc", "dp"):
        assert np.array_equal(bits(got[k]), bits(again[k])), k
        assert np.array_equal(bits(got[k]), bits(shuffled[k])), k


def test_point_jacobian_matches_central_differences(ctx):
    """One camera, one point, one observation per problem: gp = Jp^T r. Two
    problems per (pose, point) with different observations give two residuals, so
    Jp^T = [gp1 gp2] [r1 r2]^-1; against central differences of the projection in
    the point, h = 1e-6, at test_reproj_gpu's finite-difference tolerances."""
    rng = np.random.default_rng(2)
    n, h = 40, 1e-6
    probs, meta = [], []
    for i in range(n):
        R, _ = B.se3_exp(np.r_[0, 0, 0, rng.normal(0, 0.2, 3)])
        T = np.r_[R.ravel(), rng.normal(0, 0.3, 3)]
        Xc = np.array([rng.uniform(-8, 8), rng.uniform(-3, 3), rng.uniform(5, 40)])
        X = R.T @ (Xc - T[9:])
        uv = B.project(T, X[None])[0][0]
        for off in ((1.0, 0.25), (-0.5, 1.5)):
            probs.append({"poses": T[None], "fixed": np.ones(1, np.uint8), "points": X[None],
                          "obs_cam": np.zeros(1, np.int32), "obs_point": np.zeros(1, np.int32),
                          "obs_xy": (uv - off)[None].astype(np.float32)})
        meta.append((T, X, uv))
    q = B.batch(probs)
    gp = call(ctx, ctx.ba_linearize, q, lam=LAM)["gp"][:, 0]
    for i, (T, X, uv) in enumerate(meta):
        r = np.stack([uv - q["obs_xy"][2 * i, 0].astype(np.float64), uv - q["obs_xy"][2 * i + 1, 0].astype(np.float64)], 1)
        JpT = np.stack([gp[2 * i], gp[2 * i + 1]], 1) @ np.linalg.inv(r)  # 3 x 2
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            fd = (B.project(T, (X + e)[None])[0][0] - B.project(T, (X - e)[None])[0][0]) / (2 * h)
            assert np.allclose(JpT[k], fd, rtol=1e-5, atol=1e-4), (i, k)


def test_converges_to_the_truth(ctx):
    """6 cameras stepping 0.8 m along z, 300 points at 6 - 40 m, 30 % of the
    observations dropped (every point keeps two: see test_bundle_adjust_cpu),
    float32 observations without noise, two fixed cameras, free poses off by
    N(0, 0.05 m) / N(0, 0.005 rad), depths by 1 +- 3 %."""
    truth = B.window_scene(C=6, M=300, seed=0, min_obs=2)
    poses, points, costs, it = call(ctx, ctx.bundle_adjust, B.perturbed(truth, seed=1), max_iterations=50)
    n_obs = len(truth["obs_cam"])
    perr = np.abs(poses - truth["poses"]).max()
    xerr = np.median(np.linalg.norm(points - truth["points"], axis=1))
    print(f"cost {costs[0]:.3e} -> {costs[1]:.3e} in {it} iterations, pose {perr:.2e}, median point {xerr:.2e}")
    assert 0 < it <= 50
    assert costs[0] > 1e3 and costs[1] <= 1e-6 * n_obs
    assert perr < 1e-5
    assert xerr < 1e-3
    assert np.array_equal(bits(poses[:2]), bits(truth["poses"][:2]))


def test_huber_is_robust_and_weak_points_stay(ctx):
    truth = B.window_scene(C=6, M=300, seed=0, noise=0.5, outliers=0.1)
    start = B.perturbed(truth, seed=1)
    weak = np.flatnonzero(np.bincount(start["obs_point"], minlength=300) < 2)
    assert len(weak) > 0  # the scene has points seen once or never
    err = {}
    for delta in (1.0, 0.0):
        poses, points, costs, it = call(ctx, ctx.bundle_adjust, start, huber_delta=delta, max_iterations=50)
        err[delta] = np.abs(poses[2:, 9:] - truth["poses"][2:, 9:]).max()
        assert costs[1] < costs[0]
        assert np.array_equal(bits(points[weak]), bits(start["points"][weak]))
    print(f"translation error: Huber {err[1.0]:.2e}, least squares {err[0.0]:.2e}")
    assert err[1.0] < err[0.0] and err[1.0] < 0.05


def test_degenerate_structure(ctx):
    truth = B.window_scene(C=4, M=65, seed=3, min_obs=2)
    start = B.perturbed(truth, seed=4)
    # all cameras fixed: structure only
    q = dict(start)
    q["fixed"] = np.ones(4, np.uint8)
    poses, points, costs, it = call(ctx, ctx.bundle_adjust, q)
    assert np.array_equal(bits(poses), bits(start["poses"])) and costs[1] < costs[0] and it > 0
    lin = call(ctx, ctx.ba_linearize, q, lam=LAM)
    assert lin["n_free"] == 0 and lin["status"] == 0 and np.all(lin["dc"] == 0) and np.any(lin["dp"] != 0)
    # all points constant (each seen once) and one free camera: svo_refine_poses
    n = 200
    rng = np.random.default_rng(8)
    X = np.c_[rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(5, 40, n)]
    T = B.left_update(np.r_[np.eye(3).ravel(), 0, 0, 0], np.r_[0.3, -0.2, 0.1, 0.02, -0.03, 0.01])
    u = (B.project(T, X)[0] + rng.normal(0, 0.5, (n, 2))).astype(np.float32)
    T0 = B.left_update(T, np.r_[0.2, -0.1, 0.3, 0.02, -0.01, 0.015])
    for delta in (0.0, 1.0):
        ref, ref_cost, _ = ctx.refine_poses(X, u, T0[None], B.K, huber_delta=delta, max_iterations=50)
        poses, points, costs, it = ctx.bundle_adjust(T0[None], [0], X, np.zeros(n, np.int32), np.arange(n), u, B.K,
                                                     huber_delta=delta, max_iterations=50)
        assert np.abs(poses[0] - ref[0]).max() < 1e-9 and np.array_equal(bits(points), bits(X))
        assert np.isclose(costs[1], ref_cost[0], rtol=1e-9)
    # a free camera nobody observes through comes back unchanged
    q = dict(start)
    q["poses"] = np.vstack([start["poses"], B.left_update(start["poses"][3], np.r_[0, 0, 0.8, 0, 0, 0])[None]])
    q["fixed"] = np.r_[start["fixed"], 0].astype(np.uint8)
    poses, points, costs, it = call(ctx, ctx.bundle_adjust, q)
    assert np.array_equal(bits(poses[4]), bits(q["poses"][4])) and costs[1] < 1e-3 * costs[0]
    # no problem at all
    p0, x0, c0, i0 = ctx.bundle_adjust(np.zeros((0, 2, 12)), np.zeros((0, 2)), np.zeros((0, 3, 3)),
                                       np.zeros((0, 4)), np.zeros((0, 4)), np.zeros((0, 4, 2)), B.K)
    assert p0.shape == (0, 2, 12) and c0.shape == (0, 2) and len(i0) == 0


def test_batch_equals_one_by_one(ctx):
    probs = [B.perturbed(B.window_scene(C=3 + k % 3, M=40 + 9 * k, seed=20 + k, noise=0.3, outliers=0.05), seed=k)
             for k in range(8)]
    q = B.batch(probs)
    poses, points, costs, its = call(ctx, ctx.bundle_adjust, q, huber_delta=1.5, max_iterations=15)
    for p, prob in enumerate(probs):
        a, x, c, i = call(ctx, ctx.bundle_adjust, prob, huber_delta=1.5, max_iterations=15)
        Cn, M = len(prob["poses"]), len(prob["points"])
        assert np.array_equal(bits(poses[p, :Cn]), bits(a)) and np.array_equal(bits(points[p, :M]), bits(x)), p
        assert np.array_equal(bits(costs[p]), bits(c)) and its[p] == i, p


def raw_bundle_adjust(ctx, q, max_cams=None, null=None):
    """svo_bundle_adjust on caller-held arrays -> (rc, poses, points, costs, iterations)."""
    P, Cn = q["poses"].shape[:2]
    a = {k: np.ascontiguousarray(q[k], t) for k, t in (("poses", np.float64), ("fixed", np.uint8),
                                                        ("points", np.float64), ("obs_cam", np.int32),
                                                        ("obs_point", np.int32), ("obs_xy", np.float32))}
    a["poses"], a["points"] = a["poses"].copy(), a["points"].copy()
    cnt = {k: np.ascontiguousarray(q[k], np.int32) for k in ("n_cams", "n_points", "n_obs")}
    costs, its = np.full((P, 2), -7.0), np.full(P, -7, np.int32)
    Kf = np.ascontiguousarray(B.K.ravel())
    ptr = lambda k, v, t: None if k == null else v.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = S.lib().svo_bundle_adjust(
        ctx.handle, P, Cn if max_cams is None else max_cams, q["points"].shape[1], q["obs_cam"].shape[1],
        *[ptr(k, cnt[k], C.c_int) for k in ("n_cams", "n_points", "n_obs")], ptr("poses", a["poses"], C.c_double),
        ptr("fixed", a["fixed"], C.c_uint8), ptr("points", a["points"], C.c_double),
        ptr("obs_cam", a["obs_cam"], C.c_int), ptr("obs_point", a["obs_point"], C.c_int),
        ptr("obs_xy", a["obs_xy"], C.c_float), ptr("K", Kf, C.c_double), 0.0, 10,
        costs.ctypes.data_as(C.POINTER(C.c_double)), its.ctypes.data_as(C.POINTER(C.c_int)))
    return rc, a["poses"], a["points"], costs, its


def test_bad_arguments_leave_the_outputs_alone(ctx):
    good = B.batch([B.perturbed(B.window_scene(C=3, M=20, seed=k), seed=k) for k in range(2)])

    def broken(**changes):
        q = {k: v.copy() for k, v in good.items()}
        for k, (idx, val) in changes.items():
            q[k][idx] = val
        return q

    cases = {
        "camera index": (broken(obs_cam=((1, 3), 3)), {}),
        "negative camera index": (broken(obs_cam=((0, 0), -1)), {}),
        "point index": (broken(obs_point=((0, 5), 20)), {}),
        "camera count": (broken(n_cams=(1, 4)), {}),
        "point count": (broken(n_points=(0, 21)), {}),
        "observation count": (broken(n_obs=(1, good["obs_cam"].shape[1] + 1)), {}),
        "negative count": (broken(n_obs=(0, -1)), {}),
        "too many cameras": (good, {"max_cams": S.BA_MAX_CAMS + 1}),
        "null poses": (good, {"null": "poses"}),
        "null fixed": (good, {"null": "fixed"}),
        "null points": (good, {"null": "points"}),
        "null observations": (good, {"null": "obs_xy"}),
        "null K": (good, {"null": "K"}),
    }
    for name, (q, kw) in cases.items():
        rc, poses, points, costs, its = raw_bundle_adjust(ctx, q, **kw)
        assert rc == -1, name  # SVO_ERR_ARG
        assert np.array_equal(bits(poses), bits(q["poses"])) and np.array_equal(bits(points), bits(q["points"])), name
        assert np.all(costs == -7.0) and np.all(its == -7), name
        assert S.lib().svo_last_error(ctx.handle).decode().startswith("svo_bundle_adjust"), name
    rc, poses, points, costs, its = raw_bundle_adjust(ctx, good)
    assert rc == 0 and np.all(costs[:, 1] < costs[:, 0]) and np.all(its > 0)
    # the binding raises, for both entry points
    q = broken(obs_point=((1, 2), 99))
    with pytest.raises(S.SvoError):
        call(ctx, ctx.bundle_adjust, q)
    with pytest.raises(S.SvoError):
        call(ctx, ctx.ba_linearize, q)
    with pytest.raises(S.SvoError):
        ctx.bundle_adjust(np.zeros((17, 12)), np.zeros(17), np.zeros((1, 3)), [0], [0], [[0, 0]], B.K)


def test_host_mirror_bundle_adjust_is_opt_in():
    """Tracking over 6 frames of test_tracking_gpu's scene, then Map::localBundleAdjust
    over the five frames the map holds (the sixth is still the tracker's). The
    cost is recomputed from frame_info / features of those frames: their left
    features are exactly the observations not flagged as outliers."""
    from svo_amd.scene import Scene
    from svo_amd.tracking import Tracking

    sc = Scene(1241, 376, seed=33)
    P0, P1 = sc.projections()
    frames = [(sc.frame(t), sc.right(t)) for t in range(6)]

    def run(tr):
        log = []
        for L, R in frames:
            tr.push(L, R)
            assert tr.step()
            info, (xy, world, ids) = tr.frame_info(), tr.features()
            log.append((info["R"], info["t"], xy, world, ids, tr.trace("pnp_pose") if info["id"] else np.zeros(7)))
        return log

    # the tracker's K is float (Matx33f in the reference): the same rounded entries here
    Kf = np.asarray(P0, np.float32).reshape(3, 4)[:, :3].astype(np.float64)

    def cost(tr, delta):
        total, n = 0.0, 0
        for k in range(-5, 0):
            info, (xy, world, _) = tr.frame_info(map_index=k), tr.features(map_index=k)
            T = np.r_[info["R"].T.ravel(), -info["R"].T @ info["t"]]  # world -> camera
            Pc = world @ T[:9].reshape(3, 3).T + T[9:]
            r = np.c_[Kf[0, 0] * Pc[:, 0] / Pc[:, 2] + Kf[0, 2], Kf[1, 1] * Pc[:, 1] / Pc[:, 2] + Kf[1, 2]] - xy
            nr = np.linalg.norm(r, axis=1)[Pc[:, 2] > 0]
            total += np.where(nr > delta, delta * (nr - 0.5 * delta), 0.5 * nr ** 2).sum()
            n += len(xy)
        return total, n

    tr = Tracking(np.r_[P0.ravel(), P1.ravel()], features_to_track=1 << 30)
    log = run(tr)
    assert tr.frame_info(map_index=-1)["map_frames"] == 5 and tr.frame_info(map_index=-1)["id"] == 4
    before = [tr.frame_info(map_index=k) for k in range(-5, 0)]
    c_before, n_obs = cost(tr, 2.0)
    res = tr.bundle_adjust(window=5, n_fixed=2, huber_delta=2.0)
    after = [tr.frame_info(map_index=k) for k in range(-5, 0)]
    c_after, _ = cost(tr, 2.0)
    print(f"host mirror BA: {res}, numpy cost {c_before:.6e} -> {c_after:.6e}")
    assert res["frames"] == 5 and res["observations"] == n_obs and res["iterations"] > 0
    assert res["final_cost"] < res["initial_cost"]
    assert abs(c_before - res["initial_cost"]) <= 1e-9 * res["initial_cost"]
    assert abs(c_after - res["final_cost"]) <= 1e-9 * res["final_cost"]
    for k in range(2):  # the two oldest frames of the window are held
        assert np.array_equal(bits(before[k]["R"]), bits(after[k]["R"]))
        assert np.array_equal(bits(before[k]["t"]), bits(after[k]["t"]))
    assert any(not np.array_equal(before[k]["t"], after[k]["t"]) for k in range(2, 5))
    # a tracker that never calls it: the same trace, bit for bit
    tr2 = Tracking(np.r_[P0.ravel(), P1.ravel()], features_to_track=1 << 30)
    for a, b in zip(log, run(tr2)):
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8))
    with pytest.raises(S.SvoError):
        tr2.bundle_adjust(window=S.BA_MAX_CAMS + 1)
    tr.close()
    tr2.close()
