"""Stereo observations in the windowed bundle adjustment on the device
(svo_bundle_adjust_stereo, svo_ba_linearize_stereo, svo_ba_stage_lists_stereo)
against the numpy restatement of tests/ba_stereo_reference.py: the linearisation,
the bit identities (all-monocular = the monocular entries, repeat, shuffle, batch),
the counting rule and the other degenerate cases, what the stereo term is for,
and the staging of the right columns."""
import ctypes as C

import numpy as np
import pytest

import ba_reference as B
import ba_stereo_reference as R
import svo_amd as S
from test_ba_stage_gpu import host_stage, pack
from test_bundle_adjust_stereo_cpu import noisy_scene

pytestmark = pytest.mark.gpu

LAM = 1e-4
LIN_KEYS = ("U", "gc", "V", "gp", "cost", "S", "b", "dc", "dp")


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def call(ctx, fn, q, stereo=True, **kw):
    if stereo:
        kw.update(obs_ur=q["obs_ur"], baseline=q["baseline"])
    return fn(q["poses"], q["fixed"], q["points"], q["obs_cam"], q["obs_point"], q["obs_xy"], B.K,
              n_cams=q.get("n_cams"), n_points=q.get("n_points"), n_obs=q.get("n_obs"), **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def shuffled(q, probs, seed):
    """The batch with every problem's observations (ur along) in another order."""
    rng = np.random.default_rng(seed)
    sh = dict(q)
    for k in ("obs_cam", "obs_point", "obs_xy", "obs_ur"):
        sh[k] = q[k].copy()
    for p, prob in enumerate(probs):
        perm = rng.permutation(len(prob["obs_cam"]))
        for k in ("obs_cam", "obs_point", "obs_xy", "obs_ur"):
            sh[k][p, :len(perm)] = q[k][p, :len(perm)][perm]
    return sh


def assert_linearisation(got, p, prob, ref, err, tag):
    """Problem p of a batched svo_ba_linearize_stereo against numpy: U, gc, V, gp,
    cost at rtol 1e-10 / atol 1e-6; S, b, dc, dp within 100 x err (the restatement's
    float64-vs-longdouble distance on the same inputs), relative to the largest entry."""
    Cn, M, n = len(prob["poses"]), len(prob["points"]), 6 * ref["n_free"]
    assert got["n_free"][p] == ref["n_free"] and got["status"][p] == ref["status"] == 0, tag
    for k, cnt in (("U", Cn), ("gc", Cn), ("V", M), ("gp", M)):
        print(f"{tag} {k}: max abs diff {np.abs(got[k][p, :cnt] - ref[k]).max():.3e}")
        assert np.allclose(got[k][p, :cnt], ref[k], rtol=1e-10, atol=1e-6), (tag, k)
        assert np.all(got[k][p, cnt:] == 0), (tag, k)
    assert np.isclose(got["cost"][p], ref["cost"], rtol=1e-10, atol=1e-6), tag
    view = {"S": got["S"][p, :n, :n], "b": got["b"][p, :n], "dc": got["dc"][p, :Cn], "dp": got["dp"][p, :M]}
    for k, g in view.items():
        if ref[k].size == 0 or np.abs(ref[k]).max() == 0:  # no free camera: nothing to compare with
            assert np.all(g == 0), (tag, k)
            continue
        bar = 100 * err[k]
        d = np.abs(g - ref[k]).max() / np.abs(ref[k]).max()
        print(f"{tag} {k}: rel diff {d:.3e} bar {bar:.3e}")
        assert d <= bar, (tag, k, d, bar)
    assert np.all(got["S"][p, n:] == 0) and np.all(got["S"][p, :, n:] == 0), tag
    assert np.array_equal(got["dp"][p, :M].any(axis=1), ref["pt_free"] & ref["dp"].any(axis=1)), tag


# ---------------------------------------------------------------- 1. linearisation
@pytest.fixture(scope="module")
def parity_refs():
    """Per Huber setting: (1 camera, 1 point, 1 stereo observation) and
    ba_reference.PARITY_SHAPES with about half of the observations stereo, their
    numpy linearisation and its measured rounding (computed once)."""
    out = {}
    for delta, outl in ((0.0, 0.0), (2.0, 0.2)):
        probs = [R.single_stereo()] + [R.parity_case(Cn, M, 10 + k, outl) for k, (Cn, M) in enumerate(B.PARITY_SHAPES)]
        out[delta] = (probs, [R.linearize(q, LAM, delta) for q in probs],
                      [R.rounding_error(q, LAM, delta) for q in probs])
    return out


@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_linearisation_matches_numpy(ctx, parity_refs, delta):
    """Shapes (1, 1) structure only, (2, 1), (3, 63), (4, 64), (5, 65), (16, 300);
    Huber off, and delta = 2 with 20 % outliers. The float64-vs-longdouble distance
    of the stereo restatement, measured on the CPU (Huber off / delta = 2), largest
    over the shapes: S 1.4e-13 / 1.5e-13, b 4.6e-14 / 1.4e-13, dc 1.1e-11 (at (2, 1))
    / 1.6e-12, dp 2.5e-13 / 9.5e-13; at (16, 300): S 9.2e-16 / 2.6e-15, b 5.5e-15 /
    4.8e-15, dc 8.2e-14 / 1.1e-14, dp 1.5e-13 / 4.3e-14; at (1, 1): dp 8.5e-15.
    Bars: 100 x each, per shape. The MI355X lies at (16, 300): S 5.5e-15 / 4.3e-15,
    dc 2.9e-13 / 2.7e-14, dp 2.8e-13 / 1.1e-14; at (2, 1): dc 1.8e-11 / 2.1e-12; at
    (1, 1): dp 4.4e-15. Then the same bits on a repeat and with the observations, ur
    along, in another order."""
    probs, refs, errs = parity_refs[delta]
    shapes = [(1, 1)] + B.PARITY_SHAPES
    q = R.batch(probs)
    got = call(ctx, ctx.ba_linearize, q, lam=LAM, huber_delta=delta)
    for p, (prob, ref, err) in enumerate(zip(probs, refs, errs)):
        frac = (prob["obs_ur"] >= 0).mean()
        assert p < 2 or 0.3 < frac < 0.6, (p, frac)
        assert_linearisation(got, p, prob, ref, err, f"delta={delta} shape={shapes[p]}")
    assert refs[0]["n_free"] == 0 and np.any(got["dp"][0, 0] != 0)  # one stereo observation frees its point
    again = call(ctx, ctx.ba_linearize, q, lam=LAM, huber_delta=delta)
    other = call(ctx, ctx.ba_linearize, shuffled(q, probs, 5), lam=LAM, huber_delta=delta)
    for k in LIN_KEYS:
        assert np.array_equal(bits(got[k]), bits(again[k])), k
        assert np.array_equal(bits(got[k]), bits(other[k])), k


# ---------------------------------------------------------------- 2. bit identities
def stereo_healthy(k):
    """B.healthy(k) with right columns for half of its observations (0.3 px noise, 5 % outliers)."""
    truth = B.window_scene(C=3 + k % 3, M=40 + 9 * k, seed=20 + k, noise=0.3, outliers=0.05)
    truth = R.with_right(truth, truth["poses"], truth["points"], 20 + k, 0.5, 0.3, 0.05)
    return B.perturbed(truth, seed=k)


def test_all_monocular_gives_the_monocular_bits(ctx, parity_refs):
    """Every ur = -1: svo_ba_linearize_stereo returns svo_ba_linearize's bits and
    svo_bundle_adjust_stereo svo_bundle_adjust's, Huber on and off."""
    for delta in (0.0, 2.0):
        probs = parity_refs[delta][0]
        q = R.batch(probs)
        q["obs_ur"] = np.full_like(q["obs_ur"], -1.0)
        a = call(ctx, ctx.ba_linearize, q, lam=LAM, huber_delta=delta)
        b = call(ctx, ctx.ba_linearize, q, stereo=False, lam=LAM, huber_delta=delta)
        for k in LIN_KEYS + ("n_free", "status"):
            assert np.array_equal(bits(a[k]), bits(b[k])), (delta, k)
        # a point on the optical axis: x = y = 0 exactly, the terms that are -0
        q = R.batch([dict(B.on_axis(), obs_ur=np.full(1, -1.0, np.float32), baseline=R.BASELINE)])
        a = call(ctx, ctx.ba_linearize, q, lam=LAM, huber_delta=delta)
        b = call(ctx, ctx.ba_linearize, q, stereo=False, lam=LAM, huber_delta=delta)
        for k in LIN_KEYS + ("n_free", "status"):
            assert np.array_equal(bits(a[k]), bits(b[k])), (delta, k, "on the axis")
    probs = [stereo_healthy(k) for k in range(4)]
    q = R.batch(probs)
    q["obs_ur"] = np.full_like(q["obs_ur"], -1.0)
    for delta in (0.0, 1.5):
        a = call(ctx, ctx.bundle_adjust, q, huber_delta=delta, max_iterations=12)
        b = call(ctx, ctx.bundle_adjust, q, stereo=False, huber_delta=delta, max_iterations=12)
        assert np.all(a[3] > 0)
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(bits(x), bits(y)), delta
        assert np.array_equal(a[3], b[3])


def test_batch_equals_one_by_one_and_repeats(ctx):
    probs = [stereo_healthy(k) for k in range(8)]
    q = R.batch(probs)
    poses, points, costs, its = call(ctx, ctx.bundle_adjust, q, huber_delta=1.5, max_iterations=15)
    again = call(ctx, ctx.bundle_adjust, q, huber_delta=1.5, max_iterations=15)
    other = call(ctx, ctx.bundle_adjust, shuffled(q, probs, 6), huber_delta=1.5, max_iterations=15)
    for r in (again, other):
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((poses, points, costs), r[:3]))
        assert np.array_equal(its, r[3])
    mono = call(ctx, ctx.bundle_adjust, q, stereo=False, huber_delta=1.5, max_iterations=15)
    assert not np.array_equal(bits(points), bits(mono[1]))  # the stereo term is in the sums
    for p, prob in enumerate(probs):
        a, x, c, i = call(ctx, ctx.bundle_adjust, prob, huber_delta=1.5, max_iterations=15)
        Cn, M = len(prob["poses"]), len(prob["points"])
        assert np.array_equal(bits(poses[p, :Cn]), bits(a)) and np.array_equal(bits(points[p, :M]), bits(x)), p
        assert np.array_equal(bits(costs[p]), bits(c)) and its[p] == i, p


# ---------------------------------------------------------------- 3. degenerate cases
def test_counting_rule_on_the_device(ctx):
    """One stereo observation frees its point, one monocular one does not, a
    duplicate run of monocular + stereo by one camera does (in either order), a
    stereo observation behind the camera counts nothing: dp against numpy, and
    through the LM the constant point keeps its bits."""
    cases = R.counting_cases()
    names = list(cases)
    probs = [cases[n][0] for n in names]
    q = R.batch(probs)
    got = call(ctx, ctx.ba_linearize, q, lam=LAM)
    poses, points, costs, its = call(ctx, ctx.bundle_adjust, q, max_iterations=10)
    for p, name in enumerate(names):
        prob, free = cases[name]
        ref = R.linearize(prob, LAM)
        assert bool(ref["pt_free"][0]) == free, name
        assert_linearisation(got, p, prob, ref, R.rounding_error(prob, LAM, 0.0), name)
        assert bool(np.any(got["dp"][p, 0] != 0)) == free, name
        assert (not np.array_equal(bits(points[p, 0]), bits(prob["points"][0]))) == free, name
        assert costs[p, 1] < costs[p, 0] and its[p] > 0, name


def test_mixed_duplicate_runs_at_the_staging_boundary(ctx):
    """Points 3 | 4 and 7 | 8 lie either side of the elimination's 4-point passes;
    camera 1 sees each three times (monocular, stereo, monocular), camera 0 never:
    one W_ij per run, and the run's stereo observation alone frees the point."""
    prob = R.boundary_duplicates()
    ref = R.linearize(prob, LAM)
    assert list(ref["pt_cnt"][[3, 4, 7, 8]]) == [2, 2, 2, 2] and np.all(ref["pt_free"])
    q = R.batch([prob])
    got = call(ctx, ctx.ba_linearize, q, lam=LAM)
    assert_linearisation(got, 0, prob, ref, R.rounding_error(prob, LAM, 0.0), "boundary")
    assert np.all(got["dp"][0].any(axis=1))
    m = dict(prob)
    m["obs_ur"] = np.full_like(prob["obs_ur"], -1.0)
    held = call(ctx, ctx.ba_linearize, R.batch([m]), lam=LAM)
    assert not held["dp"][0, [3, 4, 7, 8]].any() and np.all(held["dp"][0, [0, 1, 2, 5, 6]].any(axis=1))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_problem_poisoned_through_ur_alone_is_left_alone(ctx, bad):
    probs = [stereo_healthy(k) for k in range(3)]
    probs[1] = dict(probs[1])
    probs[1]["obs_ur"] = probs[1]["obs_ur"].copy()
    probs[1]["obs_ur"][int(np.flatnonzero(probs[1]["obs_cam"] == 3)[0])] = bad
    q = R.batch(probs)
    poses, points, costs, its = call(ctx, ctx.bundle_adjust, q, huber_delta=1.5, max_iterations=10)
    assert np.array_equal(bits(poses[1]), bits(q["poses"][1])) and np.array_equal(bits(points[1]), bits(q["points"][1]))
    assert np.all(np.isnan(costs[1])) and its[1] == 0
    for p in (0, 2):
        a, x, c, i = call(ctx, ctx.bundle_adjust, probs[p], huber_delta=1.5, max_iterations=10)
        Cn, M = len(probs[p]["poses"]), len(probs[p]["points"])
        assert np.array_equal(bits(poses[p, :Cn]), bits(a)) and np.array_equal(bits(points[p, :M]), bits(x)), p
        assert np.array_equal(bits(costs[p]), bits(c)) and its[p] == i and i > 0, p


def raw_stereo(ctx, q, obs_ur, baseline):
    """svo_bundle_adjust_stereo on caller-held arrays -> (rc, poses, points, costs, iterations)."""
    P, Cn = q["poses"].shape[:2]
    a = {k: np.ascontiguousarray(q[k], t).copy() for k, t in (("poses", np.float64), ("fixed", np.uint8),
                                                               ("points", np.float64), ("obs_cam", np.int32),
                                                               ("obs_point", np.int32), ("obs_xy", np.float32))}
    cnt = [np.ascontiguousarray(q[k], np.int32) for k in ("n_cams", "n_points", "n_obs")]
    costs, its = np.full((P, 2), -7.0), np.full(P, -7, np.int32)
    Kf = np.ascontiguousarray(B.K.ravel())
    ptr = lambda v, t: v.ctypes.data_as(C.POINTER(t))  # noqa: E731
    ur_held = None if obs_ur is None else np.ascontiguousarray(obs_ur, np.float32)
    ur = None if obs_ur is None else ptr(ur_held, C.c_float)
    rc = S.lib().svo_bundle_adjust_stereo(
        ctx.handle, P, Cn, q["points"].shape[1], q["obs_cam"].shape[1], *[ptr(c, C.c_int) for c in cnt],
        ptr(a["poses"], C.c_double), ptr(a["fixed"], C.c_uint8), ptr(a["points"], C.c_double),
        ptr(a["obs_cam"], C.c_int), ptr(a["obs_point"], C.c_int), ptr(a["obs_xy"], C.c_float), ur, baseline,
        ptr(Kf, C.c_double), 0.0, 10, ptr(costs, C.c_double), ptr(its, C.c_int))
    return rc, a["poses"], a["points"], costs, its


def test_bad_stereo_arguments_leave_the_outputs_alone(ctx):
    q = R.batch([stereo_healthy(k) for k in range(2)])
    cases = {"null obs_ur": (None, 0.54), "zero baseline": (q["obs_ur"], 0.0),
             "negative baseline": (q["obs_ur"], -0.54), "nan baseline": (q["obs_ur"], np.nan),
             "infinite baseline": (q["obs_ur"], np.inf)}
    for name, (ur, b) in cases.items():
        rc, poses, points, costs, its = raw_stereo(ctx, q, ur, b)
        assert rc == -1, name  # SVO_ERR_ARG
        assert np.array_equal(bits(poses), bits(q["poses"])) and np.array_equal(bits(points), bits(q["points"])), name
        assert np.all(costs == -7.0) and np.all(its == -7), name
        assert S.lib().svo_last_error(ctx.handle).decode().startswith("svo_bundle_adjust_stereo"), name
    rc, poses, points, costs, its = raw_stereo(ctx, q, q["obs_ur"], 0.54)
    assert rc == 0 and np.all(costs[:, 1] < costs[:, 0]) and np.all(its > 0)
    for b in (0.0, -1.0, np.nan):
        with pytest.raises(S.SvoError):
            call(ctx, ctx.ba_linearize, dict(q, baseline=b), lam=LAM)
    with pytest.raises(ValueError):
        ctx.bundle_adjust(q["poses"], q["fixed"], q["points"], q["obs_cam"], q["obs_point"], q["obs_xy"], B.K,
                          obs_ur=q["obs_ur"])


# ---------------------------------------------------------------- 4. what it is for
def test_points_of_the_newest_keyframe_move_to_the_truth(ctx):
    """5 cameras stepping 0.8 m along z (two fixed), 60 points seen by all of them
    (stereo in the camera that created them), 38 points created at the last camera:
    one stereo observation each and nothing else; float32 observations without
    noise, free poses off by N(0, 0.05 m) / N(0, 0.005 rad), depths by 1 +- 5 %.
    The monocular call leaves the new points' bits alone. The stereo call moves
    them to the truth; numpy's LM on the same inputs (test_bundle_adjust_stereo_cpu)
    ends at cost 3.5e-8 with the new points 1.4e-5 m (median; largest 1.5e-4 m) and
    the poses 2.2e-7 from it. Bars: test_converges_to_the_truth's (cost 1e-6 per
    observation, poses 1e-5, median point 1e-3)."""
    truth, start, new = R.newest_keyframe_scene(seed=0)
    n_obs = len(truth["obs_cam"])
    _, pm, cm, _ = call(ctx, ctx.bundle_adjust, start, stereo=False, max_iterations=50)
    assert np.array_equal(bits(pm[new]), bits(start["points"][new]))
    poses, points, costs, it = call(ctx, ctx.bundle_adjust, start, max_iterations=50)
    err = np.linalg.norm(points - truth["points"], axis=1)[new]
    err0 = np.linalg.norm(start["points"] - truth["points"], axis=1)[new]
    perr = np.abs(poses - truth["poses"]).max()
    print(f"cost {costs[0]:.3e} -> {costs[1]:.3e} in {it} iterations (monocular: {cm[1]:.3e}), poses {perr:.2e}, "
          f"new points median {np.median(err):.2e} max {err.max():.2e} (start {np.median(err0):.2e})")
    assert 0 < it <= 50 and np.median(err0) > 0.1
    assert costs[0] > 1e3 and costs[1] <= 1e-6 * n_obs
    assert perr < 1e-5
    assert np.median(err) < 1e-3
    assert np.array_equal(bits(poses[:2]), bits(truth["poses"][:2]))


def test_stereo_beats_monocular_under_noise(ctx):
    """noisy_scene() (0.5 px noise, every observation stereo): the median point error
    after the stereo adjustment lies below the monocular one's (numpy alone: 0.110 m
    against 0.311 m), and both final costs agree with numpy's LM."""
    truth, start = noisy_scene()
    _, X, c, _ = call(ctx, ctx.bundle_adjust, start, max_iterations=30)
    _, Xm, cm, _ = call(ctx, ctx.bundle_adjust, start, stereo=False, max_iterations=30)
    es = np.median(np.linalg.norm(X - truth["points"], axis=1))
    em = np.median(np.linalg.norm(Xm - truth["points"], axis=1))
    ref, ref_m = R.lm(start, 0.0, 30)[2], B.lm(R.mono(start), 0.0, 30)[2]
    print(f"median point error: stereo {es:.4f} m, monocular {em:.4f} m; final cost {c[1]:.9e} (numpy {ref[1]:.9e}), "
          f"monocular {cm[1]:.9e} (numpy {ref_m[1]:.9e})")
    assert es < em
    assert np.isclose(c[0], ref[0], rtol=1e-10) and np.isclose(c[1], ref[1], rtol=1e-9)
    assert np.isclose(cm[1], ref_m[1], rtol=1e-9)


# ---------------------------------------------------------------- 5. staging
def test_staging_carries_the_right_columns(ctx):
    """svo_ba_stage_lists_stereo's `our` = ur gathered by svo_ba_sort_observations'
    order, everything else as svo_ba_stage_lists: empty lists, a list of one, ids
    shared by all lists, lengths around a wave and a block."""
    rng = np.random.default_rng(11)
    W, cap = 4, 320

    def lst(a):
        a = np.asarray(a, np.int32)
        return a, rng.uniform(0, 1000, (len(a), 2)).astype(np.float32)

    empty = lst([])
    shared = np.arange(5, 70, dtype=np.int32)
    ragged = [np.sort(rng.choice(480, size=n, replace=False)) for n in (63, 65, 257, cap)]
    problems = [[empty, lst([9]), empty, lst([3, 9, 11])], [lst(shared) for _ in range(W)], [lst(a) for a in ragged],
                [empty] * W]
    counts, ids, xy = pack(problems, W, cap)
    ur = np.full((len(problems), W, cap), np.nan, np.float32)  # (behind a list's end: never read)
    for p, lists in enumerate(problems):
        for j, (a, _) in enumerate(lists):
            u = rng.uniform(0, 1000, len(a)).astype(np.float32)
            u[rng.random(len(a)) < 0.4] = -1.0
            ur[p, j, :len(a)] = u
    got = ctx.ba_stage_lists(counts, ids, xy, ur=ur)
    plain = ctx.ba_stage_lists(counts, ids, xy)
    assert "our" not in plain
    ip = C.POINTER(C.c_int)
    for p, lists in enumerate(problems):
        want = host_stage(lists, W, cap)
        for k, v in want.items():
            assert np.array_equal(np.asarray(got[k][p]).view(np.uint32), np.asarray(v).view(np.uint32)), (p, k)
            assert np.array_equal(got[k][p], plain[k][p], equal_nan=True), (p, k)
        # the host's order of the observations listed camera by camera
        cam = np.concatenate([np.full(len(a), j, np.int32) for j, (a, _) in enumerate(lists)]).astype(np.int32)
        mid = np.concatenate([a for a, _ in lists]).astype(np.int32)
        flat = np.concatenate([ur[p, j, :len(a)] for j, (a, _) in enumerate(lists)])
        pid = np.unique(mid)
        pt = np.ascontiguousarray(np.searchsorted(pid, mid), np.int32)
        n, M = len(cam), len(pid)
        order, cam_idx = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        pt_off, cam_off = np.zeros(M + 1, np.int32), np.zeros(W + 1, np.int32)
        assert S.lib().svo_ba_sort_observations(cam.ctypes.data_as(ip), pt.ctypes.data_as(ip), n, W, M,
                                                order.ctypes.data_as(ip), pt_off.ctypes.data_as(ip),
                                                cam_off.ctypes.data_as(ip), cam_idx.ctypes.data_as(ip)) == 0
        assert np.array_equal(got["our"][p, :n].view(np.uint32), flat[order[:n]].view(np.uint32)), p
        assert np.all(got["our"][p, n:] == 0), p
    assert list(got["n_obs"]) == [4, W * len(shared), 63 + 65 + 257 + cap, 0]
    with pytest.raises(S.SvoError):
        ctx._check(S.lib().svo_ba_stage_lists_stereo(ctx.handle, 1, 1, 1, *[None] * 14))
