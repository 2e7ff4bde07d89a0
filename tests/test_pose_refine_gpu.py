"""svo_refine_poses_stereo: the whole Levenberg-Marquardt of a stereo pose
refinement in one launch. The linearisation against the numpy restatement
(tests/pose_refine_reference.py); the summation order against
svo_reprojection_jacobians, bit for bit; determinism and independence of the
batch; the LM trajectory against the restatement over the prefix in which float64
and longdouble decide alike; the paths (empty, behind the camera, values that are
not finite, refused arguments); and what the stereo term adds to the information
matrix."""
import ctypes as C

import numpy as np
import pytest

import pose_refine_reference as Q
import svo_amd as S

pytestmark = pytest.mark.gpu

K = Q.K
NEAR = np.r_[0.05, -0.02, 0.1, 0.003, -0.002, 0.001]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def batch(probs, max_n=None):
    """[(X, xy, ur, T0)] -> padded arrays and counts."""
    counts = np.array([len(p[0]) for p in probs], np.int32)
    n = max(int(max_n or counts.max()), 1)
    X, xy = np.zeros((len(probs), n, 3)), np.zeros((len(probs), n, 2), np.float32)
    ur = np.full((len(probs), n), -1.0, np.float32)
    for p, (x, u, r, _) in enumerate(probs):
        X[p, :len(x)], xy[p, :len(x)], ur[p, :len(x)] = x, u, r
    return X, xy, ur, np.stack([p[3] for p in probs]), counts


def run(ctx, probs, delta=0.0, iters=20, max_n=None, baseline=Q.BASELINE):
    X, xy, ur, T, counts = batch(probs, max_n)
    return ctx.refine_poses_stereo(X, xy, ur, T, K, baseline, counts=counts, huber_delta=delta, max_iterations=iters)


def same(a, b):
    """two (poses, costs, iterations, normal) results, bit for bit"""
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def behind(T, X, i):
    """X with point i 3 m behind the camera of pose T"""
    X = X.copy()
    X[i] = T[:9].reshape(3, 3).T @ (np.array([0.3, -0.2, -3.0]) - T[9:])
    return X


def problem(n, seed, noise=0.5, outliers=0.2, xi=NEAR, of=None):
    """the first n points of a noisy scene of `of` points, started xi off the truth"""
    X, xy, ur, T = Q.stereo_scene(of or n, seed, noise, outliers)
    return X[:n], xy[:n], ur[:n], Q.left_update(T, xi)


# ---------------------------------------------------------------- 1. linearisation
SIZES = [1, 63, 64, 65, 255, 256, 257, 513, 700]


def test_linearisation_matches_the_restatement(ctx):
    """max_iterations = 0 over one ragged batch of the nine sizes around the block
    and wave boundaries, half the observations stereo,
    20 % outliers, Huber 2, a point behind the camera in the problems of 64 and 700:
    normal against numpy at test_reproj_gpu's bar; poses keep their bits, the costs
    are equal and no iteration is counted."""
    probs = [problem(n, 30 + k, of=700) for k, n in enumerate(SIZES)]
    for k in (2, 8):
        X, xy, ur, T0 = probs[k]
        probs[k] = (behind(T0, X, 5), xy, ur, T0)
    poses, costs, its, ne = run(ctx, probs, delta=2.0, iters=0)
    for p, (X, xy, ur, T0) in enumerate(probs):
        assert np.array_equal(bits(poses[p]), bits(T0))
        ref = Q.linearize(T0, X, xy, ur, delta=2.0)
        assert np.allclose(ne[p], ref, rtol=1e-10, atol=1e-6), (SIZES[p], np.abs(ne[p] - ref).max())
        assert bits(costs[p, 0]) == bits(costs[p, 1]) == bits(ne[p, 27]) and its[p] == 0
    front = Q.terms(probs[8][3], *probs[8][:3], Q.BASELINE, 2.0)[0]
    assert not front[5] and front.sum() == 699


# ---------------------------------------------------------------- 2. the summation order
@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_monocular_sums_are_the_reprojection_kernels_bits(ctx, delta):
    """n <= 256, ur all negative: the stated order is reproj_kernel's, so normal
    equals svo_reprojection_jacobians' to the bit. The last problem sees 64 points
    from the identity rotation, 8 of them on the optical axis (x = y = 0 exactly),
    8 on x = 0 and 8 on y = 0: the terms that are -0."""
    probs = [problem(n, 50 + k) for k, n in enumerate([1, 64, 200, 256])]
    X, xy, _, _ = problem(64, 54)
    X[:8, :2], X[8:16, 0], X[16:24, 1] = 0.0, 0.0, 0.0
    probs.append((X, xy, None, np.r_[np.eye(3).ravel(), 0.0, 0.0, 0.5]))
    probs = [(X, xy, np.full(len(X), -1.0, np.float32), T0) for X, xy, _, T0 in probs]
    X, xy, ur, T, counts = batch(probs)
    _, _, _, ne = run(ctx, probs, delta=delta, iters=0)
    _, _, want = ctx.reprojection_jacobians(X, xy, T, K, counts=counts, huber_delta=delta)
    assert np.array_equal(bits(ne), bits(want)), np.abs(ne - want).max()


# ---------------------------------------------------------------- 3. determinism, independence
def test_results_do_not_depend_on_the_batch(ctx):
    solo = problem(300, 60)
    others = [problem(n, 61 + k) for k, n in enumerate([40, 257, 513, 100])]
    a = run(ctx, [solo], delta=2.0, iters=8)
    assert a[2][0] > 1 and a[1][0, 1] < a[1][0, 0]
    assert same(a, run(ctx, [solo], delta=2.0, iters=8))  # two runs
    b = run(ctx, others[:3] + [solo] + others[3:], delta=2.0, iters=8)  # problem 3 of 5
    assert same(a, [x[3:4] for x in b])
    assert same(a, run(ctx, [solo], delta=2.0, iters=8, max_n=1000))  # max_n padded from 300 to 1000
    X, xy, _, T0 = solo
    m1 = run(ctx, [(X, xy, np.full(300, -1.0, np.float32), T0)], delta=2.0, iters=8)
    m2 = run(ctx, [(X, xy, np.full(300, -7.5, np.float32), T0)], delta=2.0, iters=8)
    assert same(m1, m2) and not same(m1, a)


# ---------------------------------------------------------------- 4. trajectory
@pytest.mark.parametrize("name", list(Q.TRAJECTORY))
def test_trajectory_follows_the_restatement(ctx, name):
    """The device keeps lambda and its verdicts to itself, so the trajectory is read
    by running from the same start with max_iterations = 1 .. K, K from
    Q.lm_prefix (>= 3 for every scene: test_pose_refine_cpu). After k iterations the
    cost equals the float64 restatement's at rtol 1e-10 and a step was rejected
    exactly when the restatement rejected it; the run to convergence ends at the
    restatement's cost (rtol 1e-9) and within 100 x the float64-to-longdouble
    distance of its pose (floor 1e-12)."""
    X, xy, ur, T, T0, delta = Q.trajectory_case(name)
    Kp, h64, hld, r64, rld = Q.lm_prefix(T0, X, xy, ur, delta=delta, max_iterations=Q.TRAJECTORY_ITERATIONS)
    assert Kp >= 3
    prev, pattern = None, ""
    for k in range(1, Kp + 1):
        poses, costs, its, ne = run(ctx, [(X, xy, ur, T0)], delta=delta, iters=k)
        if prev is None:
            prev = costs[0, 0]
            assert np.isclose(costs[0, 0], h64[0]["c_cur"], rtol=1e-10)
        rejected = bits(costs[0, 1]) == bits(prev)
        prev = costs[0, 1]
        pattern += "r" if rejected else "a"
        ref = float(h64[k - 1]["cost"])
        print(f"{name} k={k} {h64[k - 1]['event']}: cost {costs[0, 1]:.12e} ref {ref:.12e} "
              f"rel diff {abs(costs[0, 1] - ref) / ref:.3e}")
        assert rejected == (h64[k - 1]["event"] == "reject"), (k, pattern)
        assert np.isclose(costs[0, 1], ref, rtol=1e-10, atol=0), (k, costs[0, 1], ref)
        assert its[0] == k and bits(ne[0, 27]) == bits(costs[0, 1])
    if Kp == len(h64):  # the prefix covers the whole capped run
        _, _, its, _ = run(ctx, [(X, xy, ur, T0)], delta=delta, iters=Q.TRAJECTORY_ITERATIONS)
        assert its[0] == r64[2]
    p64, c64, _, _ = Q.lm(T0, X, xy, ur, delta=delta, max_iterations=50)
    pld = Q.lm(T0, X, xy, ur, delta=delta, max_iterations=50, dt=np.longdouble)[0]
    poses, costs, its, ne = run(ctx, [(X, xy, ur, T0)], delta=delta, iters=50)
    bar = max(100 * float(np.abs(p64 - pld).max()), 1e-12)
    d = np.abs(poses[0] - p64).max()
    print(f"{name} K={Kp} {pattern}: converged in {its[0]}, cost {costs[0, 1]:.12e} ref {c64[1]:.12e}, "
          f"pose distance {d:.3e} bar {bar:.3e}")
    assert np.isclose(costs[0, 1], c64[1], rtol=1e-9, atol=0)
    assert d <= bar, (d, bar)
    assert its[0] < 50


def test_exact_data_reaches_the_truth(ctx):
    probs, truth = [], []
    for seed, n in ((70, 40), (71, 300), (72, 1500)):
        X, xy, ur, T = Q.stereo_scene(n, seed)
        probs.append((X, xy, ur, Q.start_pose(T, seed, 0.5, 0.05)))
        truth.append(T)
    poses, costs, its, ne = run(ctx, probs, iters=50)
    for p, T in enumerate(truth):
        assert np.abs(poses[p] - T).max() < 1e-5, p  # float observations -> ~1e-6 pose noise
        assert costs[p, 1] < 1e-6 * len(probs[p][0]) and 1 < its[p] < 50


@pytest.mark.parametrize("delta", [0.0, 1.0])
def test_all_monocular_run_reaches_the_host_solvers_cost(ctx, delta):
    X, xy, _, T0 = problem(500, 75, outliers=0.1)
    ur = np.full(500, -1.0, np.float32)
    _, costs, its, _ = run(ctx, [(X, xy, ur, T0)], delta=delta, iters=50)
    _, want, _ = ctx.refine_poses(X, xy, T0[None], K, huber_delta=delta, max_iterations=50)
    assert np.isclose(costs[0, 1], want[0], rtol=1e-9, atol=0) and its[0] > 1


# ---------------------------------------------------------------- 5. paths
def test_nothing_to_see_stops_on_the_step_rule(ctx):
    X, xy, ur, T0 = problem(70, 80)
    Xb = np.tile(behind(T0, X, 0)[0], (70, 1))
    empty = (X[:0], xy[:0], ur[:0], T0)
    poses, costs, its, ne = run(ctx, [empty, (Xb, xy, ur, T0), (X, xy, ur, T0)], delta=2.0, iters=10)
    for p in (0, 1):
        assert np.array_equal(bits(poses[p]), bits(T0)) and np.all(costs[p] == 0) and its[p] == 1
        assert np.all(ne[p] == 0)
    assert its[2] > 1 and costs[2, 1] < costs[2, 0]
    # max_n == 0: every problem is the empty one
    p0, c0, i0, _ = ctx.refine_poses_stereo(np.zeros((2, 0, 3)), np.zeros((2, 0, 2), np.float32), None,
                                            np.stack([T0, T0]), K, Q.BASELINE, max_iterations=5)
    assert np.array_equal(bits(p0), bits(np.stack([T0, T0]))) and np.all(c0 == 0) and list(i0) == [1, 1]


@pytest.mark.parametrize("where", ["pose", "point", "xy", "ur", "inf ur"])
def test_values_that_are_not_finite_stay_in_their_problem(ctx, where):
    good = [problem(100, 81), problem(300, 82)]
    X, xy, ur, T0 = [a.copy() for a in problem(257, 83)]
    if where == "pose":
        T0[10] = np.nan
    elif where == "point":
        X[256, 1] = np.nan
    elif where == "xy":
        xy[3, 0] = np.nan
    elif where == "ur":
        ur[200] = np.nan
    else:
        ur[200] = -np.inf
    poses, costs, its, ne = run(ctx, [good[0], (X, xy, ur, T0), good[1]], delta=2.0, iters=10)
    assert np.array_equal(bits(poses[1]), bits(T0)) and np.all(np.isnan(costs[1])) and its[1] == 0
    for p, g in ((0, good[0]), (2, good[1])):
        solo = run(ctx, [g], delta=2.0, iters=10)
        assert same(solo, [x[p:p + 1] for x in (poses, costs, its, ne)]), p
        assert its[p] > 1 and np.all(np.isfinite(costs[p]))


def test_a_nan_beyond_the_count_is_ignored(ctx):
    X, xy, ur, T0 = problem(100, 84)
    a = run(ctx, [(X, xy, ur, T0)], delta=2.0, iters=6, max_n=104)
    Xp, xyp, urp, T, counts = batch([(X, xy, ur, T0)], 104)
    Xp[0, 100:], xyp[0, 101], urp[0, 102:] = np.nan, np.nan, np.nan
    b = ctx.refine_poses_stereo(Xp, xyp, urp, T, K, Q.BASELINE, counts=counts, huber_delta=2.0, max_iterations=6)
    assert same(a, b) and np.all(np.isfinite(b[1]))


def test_refused_arguments_write_nothing(ctx):
    X, xy, ur, T0 = problem(20, 85)
    with pytest.raises(S.SvoError):
        run(ctx, [(X, xy, ur, T0)], iters=1001)
    with pytest.raises(S.SvoError):
        run(ctx, [(X, xy, ur, T0)], baseline=0.0)
    with pytest.raises(S.SvoError):
        run(ctx, [(X, xy, ur, T0)], baseline=np.inf)
    with pytest.raises(S.SvoError):
        ctx.refine_poses_stereo(X, xy, None, T0, K, Q.BASELINE)
    with pytest.raises(S.SvoError):
        run(ctx, [(X, xy, ur, T0)], iters=-1)
    # straight at the C ABI: the outputs keep what they held
    f64p, f32p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
    Xc, xyc, urc = np.ascontiguousarray(X), np.ascontiguousarray(xy), np.ascontiguousarray(ur)
    Kc = np.ascontiguousarray(K, np.float64).reshape(9)
    for kw in ({"iters": 1001}, {"baseline": 0.0}, {"ur": None}):
        pose, costs, ne = T0.copy(), np.full(2, 7.0), np.full(28, 7.0)
        its = np.full(1, 7, np.int32)
        u = kw.get("ur", urc)
        rc = S.lib().svo_refine_poses_stereo(
            ctx.handle, Xc.ctypes.data_as(f64p), xyc.ctypes.data_as(f32p), u.ctypes.data_as(f32p) if u is not None else None,
            None, 1, 20, Kc.ctypes.data_as(f64p), kw.get("baseline", Q.BASELINE), 0.0, kw.get("iters", 5),
            pose.ctypes.data_as(f64p), costs.ctypes.data_as(f64p), its.ctypes.data_as(i32p), ne.ctypes.data_as(f64p))
        assert rc == -1 and S.lib().svo_last_error(ctx.handle).decode().startswith("svo_refine_poses_stereo"), kw
        assert np.array_equal(bits(pose), bits(T0)) and np.all(costs == 7) and its[0] == 7 and np.all(ne == 7), kw


def test_no_problem_at_all(ctx):
    p, c, i, ne = ctx.refine_poses_stereo(np.zeros((0, 4, 3)), np.zeros((0, 4, 2), np.float32),
                                          np.zeros((0, 4), np.float32), np.zeros((0, 12)), K, Q.BASELINE)
    assert p.shape == (0, 12) and c.shape == (0, 2) and len(i) == 0 and ne.shape == (0, 28)


# ---------------------------------------------------------------- 6. what stereo adds
def test_stereo_adds_its_rows_to_the_information_matrix(ctx):
    """Exact data at the truth: H_stereo - H_mono is sum J2^T J2 over the stereo
    observations (the restatement's), at test 1's bar. Its diagonal is positive
    except for the y translation: the right column does not depend on it (the
    row's second entry is 0), so H[1][1] gains exactly nothing."""
    X, xy, ur, T = Q.stereo_scene(300, 90)
    mono = np.full(300, -1.0, np.float32)
    _, _, _, ne = run(ctx, [(X, xy, ur, T), (X, xy, mono, T)], iters=0)
    _, stereo, _, w, _, Jc = Q.terms(T, X, xy, ur, Q.BASELINE, 0.0)
    assert stereo.sum() > 100 and np.all(w == 1)
    add = np.einsum("n,ni,nj->ij", stereo.astype(np.float64), Jc[:, 2], Jc[:, 2])[Q.TRIU6]
    got = ne[0, :21] - ne[1, :21]
    assert np.allclose(got, add, rtol=1e-10, atol=1e-6), np.abs(got - add).max()
    diag = [0, 11, 15, 18, 20]
    assert np.all(got[diag] > 0) and got[6] == 0
