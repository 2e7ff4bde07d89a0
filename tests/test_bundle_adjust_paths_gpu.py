"""The windowed bundle adjustment where test_bundle_adjust_gpu's scenes never
take it: runs of duplicate (camera, point) observations, the strided second
passes of the camera kernel and of the elimination's staging, the full reduced
system of order 96, a reduced system that is exactly singular (status 1, the
retry loop, giving up), rejected steps, and values that are not finite. The
yardstick is tests/ba_reference.py; test_bundle_adjust_cpu.py asserts that each
scene has the property its test here relies on."""
import functools

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


def order_keeping_shuffle(rng, oc, op):
    """A random order of the observations that keeps the caller's order within
    every (camera, point) pair: the results do not depend on the order beyond the
    stable sort by (point, camera), which sums a pair's duplicates as they came.
    Without duplicates this is any permutation."""
    perm = rng.permutation(len(oc))
    key = (np.asarray(op, np.int64) * (S.BA_MAX_CAMS + 1) + oc)[perm]
    for v in np.unique(key):
        at = np.flatnonzero(key == v)
        perm[at] = np.sort(perm[at])
    return perm


SHAPES = {
    "dense duplicates": lambda outl: [B.dense_duplicates(0, outl)],
    "sparse duplicates": lambda outl: [B.sparse_duplicates(0, outl)],
    "wide camera": lambda outl: [B.wide_camera(0, outl)],
    # a small problem behind the full one: whatever the full system writes past its own block lands there
    "full system": lambda outl: [B.full_system(0, outl), B.parity_case(2, 1, 10, outl)],
}


@functools.lru_cache(maxsize=None)
def shape_refs(shape, delta):
    """The problems of a shape, their numpy linearisation and the measured
    float64-vs-longdouble rounding of S, b, dc, dp (computed once, never written to)."""
    probs = SHAPES[shape](0.2 if delta else 0.0)
    return probs, [B.linearize(q, LAM, delta) for q in probs], [B.rounding_error(q, LAM, delta) for q in probs]


@pytest.mark.parametrize("delta", [0.0, 2.0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_linearisation_on_the_unreached_shapes(ctx, shape, delta):
    """test_linearisation_matches_numpy's bars on the shapes its scenes leave out.
    U, gc, V, gp, cost: rtol 1e-10, atol 1e-6. S, b, dc, dp: 100 x the distance of
    the float64 restatement from np.longdouble on the case's own inputs, relative
    to the largest entry. Then the same bits on a repeat and on shuffled
    observations.
    - dense duplicates: 2 cameras x 5 points x 70 observations of every pair; 350
      observations per camera (ba_camera_kernel's second a += 256 pass), 560 among
      the first four points (the staging loop's second a += 512 pass), runs of 70
      for the first observation of a run to sum.
    - sparse duplicates: point 0 seen twice by camera 1 and by nobody else is
      constant (one camera: dp == 0 exactly); point 1, seen twice by camera 1 and
      once by camera 2, moves.
    - wide camera: 2 cameras x 300 points, nothing dropped.
    - full system: 16 free cameras, n = 96, all 4656 packed entries; S symmetric,
      and the small problem behind it in the batch has nothing outside its block.
    Measured (CPU rounding, Huber off / delta = 2) -> bars are 100 x these:
      dense   S 5.6e-12 / 5.5e-13, b 3.7e-12 / 5.3e-13, dc 1.7e-11 / 1.9e-12, dp 5.9e-11 / 2.8e-12
      sparse  S 7.6e-14 / 8.6e-14, b 8.9e-14 / 6.9e-14, dc 8.0e-13 / 2.8e-13, dp 2.2e-12 / 9.8e-13
      wide    S 1.2e-13 / 2.8e-14, b 2.4e-14 / 2.7e-14, dc 3.2e-13 / 2.4e-13, dp 6.2e-13 / 8.3e-13
      full    S 3.6e-15 / 9.7e-15, b 4.0e-15 / 2.2e-14, dc 5.8e-12 / 1.2e-11, dp 6.4e-13 / 6.1e-13
    Measured on the MI355X (device against float64 numpy, same order):
      dense   S 1.1e-12 / 2.0e-12, b 8.9e-13 / 1.2e-12, dc 2.6e-11 / 8.7e-13, dp 7.5e-11 / 4.6e-12
      sparse  S 1.0e-13 / 1.1e-13, b 9.9e-14 / 1.1e-13, dc 7.0e-13 / 9.8e-13, dp 1.7e-12 / 9.9e-13
      wide    S 9.8e-14 / 2.6e-14, b 1.8e-14 / 3.8e-14, dc 2.9e-13 / 4.0e-13, dp 6.6e-13 / 1.0e-12
      full    S 4.3e-15 / 1.3e-14, b 1.3e-14 / 1.8e-14, dc 1.0e-11 / 1.4e-11, dp 1.1e-12 / 4.2e-13
    (the nearest to its bar: dense, delta = 2, S at 3.7 % of it); U, gc, V, gp: at most 6.6e-7
    absolute (an entry of U of the dense case)."""
    probs, refs, errs = shape_refs(shape, delta)
    q = B.batch(probs)
    got = call(ctx, ctx.ba_linearize, q, lam=LAM, huber_delta=delta)
    for p, (prob, ref, err) in enumerate(zip(probs, refs, errs)):
        Cn, M, n = len(prob["poses"]), len(prob["points"]), 6 * ref["n_free"]
        assert got["n_free"][p] == ref["n_free"] and got["status"][p] == ref["status"] == 0
        for k, cnt in (("U", Cn), ("gc", Cn), ("V", M), ("gp", M)):
            d = np.abs(got[k][p, :cnt] - ref[k]).max()
            print(f"{shape} delta={delta} problem {p} {k}: max abs diff {d:.3e}")
            assert np.allclose(got[k][p, :cnt], ref[k], rtol=1e-10, atol=1e-6), (p, k)
            assert np.all(got[k][p, cnt:] == 0)
        assert np.isclose(got["cost"][p], ref["cost"], rtol=1e-10, atol=1e-6)
        view = {"S": got["S"][p, :n, :n], "b": got["b"][p, :n], "dc": got["dc"][p, :Cn], "dp": got["dp"][p, :M]}
        for k, g in view.items():
            bar = 100 * err[k]
            d = np.abs(g - ref[k]).max() / np.abs(ref[k]).max()
            print(f"{shape} delta={delta} problem {p} {k}: rel diff {d:.3e} bar {bar:.3e}")
            assert d <= bar, (p, k, d, bar)
        # nothing beyond n, beyond the problem's cameras and points
        assert np.all(got["S"][p, n:] == 0) and np.all(got["S"][p, :, n:] == 0) and np.all(got["b"][p, n:] == 0)
        assert np.all(got["dc"][p, Cn:] == 0) and np.all(got["dp"][p, M:] == 0)
        assert np.array_equal(bits(got["S"][p]), bits(got["S"][p].T))
    dp = got["dp"][0]
    if shape == "dense duplicates":
        assert refs[0]["pt_free"].all() and np.all(np.abs(dp[:5]).max(1) > 0)
    if shape == "sparse duplicates":
        assert refs[0]["pt_cnt"][0] == 1 and np.all(dp[0] == 0)
        assert refs[0]["pt_cnt"][1] == 2 and np.abs(dp[1]).max() > 1e-3
    if shape == "full system":
        assert got["n_free"][0] == 16 and got["n_free"][1] == 1
    # the same bits on a repeat and with the observations in another order
    again = call(ctx, ctx.ba_linearize, q, lam=LAM, huber_delta=delta)
    rng = np.random.default_rng(5)
    sh = dict(q)
    sh["obs_cam"], sh["obs_point"], sh["obs_xy"] = q["obs_cam"].copy(), q["obs_point"].copy(), q["obs_xy"].copy()
    for p, prob in enumerate(probs):
        perm = order_keeping_shuffle(rng, prob["obs_cam"], prob["obs_point"])
        assert not np.array_equal(perm, np.arange(len(perm))) or len(perm) < 2
        for k in ("obs_cam", "obs_point", "obs_xy"):
            sh[k][p, :len(perm)] = q[k][p, :len(perm)][perm]
    shuffled = call(ctx, ctx.ba_linearize, sh, lam=LAM, huber_delta=delta)
    for k in ("U", "gc", "V", "gp", "cost", "S", "b", "dc", "dp"):
        assert np.array_equal(bits(got[k]), bits(again[k])), k
        assert np.array_equal(bits(got[k]), bits(shuffled[k])), k


def test_singular_reduced_system_is_status_1_exactly(ctx):
    """B.on_axis(): x = y = 0, so rows and columns 2 and 5 of U are exactly zero at
    every lambda, the point is constant (seen once) and S = U*: the third pivot is
    exactly 0 on any correct implementation. svo_ba_linearize reports status 1
    with a zero step and still returns S and b; svo_bundle_adjust raises lambda to
    1e16, gives up and returns the input, having begun one iteration. Between two
    healthy problems of a batch the retries run with a subset active while the
    neighbours wait for their verdict; they come out as they do alone."""
    q = B.on_axis()
    for lam in (0.0, LAM, 1.0, 1e15):
        ref = B.linearize(q, lam)
        got = call(ctx, ctx.ba_linearize, q, lam=lam)
        assert ref["status"] == 1 and got["status"] == 1 and got["n_free"] == 1 == ref["n_free"]
        assert np.all(got["dc"] == 0) and np.all(got["dp"] == 0)
        assert np.all(got["S"][[2, 5]] == 0) and np.all(got["S"][:, [2, 5]] == 0)
        assert np.allclose(got["S"], ref["S"], rtol=1e-13, atol=0) and np.allclose(got["b"], ref["b"], rtol=1e-13, atol=0)
        assert np.isclose(got["cost"], ref["cost"], rtol=1e-13)
    _, _, ref_costs, ref_it = B.lm(q)
    poses, points, costs, it = call(ctx, ctx.bundle_adjust, q)
    assert np.array_equal(bits(poses), bits(q["poses"])) and np.array_equal(bits(points), bits(q["points"]))
    assert bits(costs[0]) == bits(costs[1]) and np.isclose(costs[0], ref_costs[0], rtol=1e-13)
    assert it == 1 == ref_it
    # between two healthy problems
    probs = [B.healthy(0), q, B.healthy(1)]
    poses, points, costs, its = call(ctx, ctx.bundle_adjust, B.batch(probs), huber_delta=1.5, max_iterations=15)
    for p, prob in enumerate(probs):
        a, x, c, i = call(ctx, ctx.bundle_adjust, prob, huber_delta=1.5, max_iterations=15)
        Cn, M = len(prob["poses"]), len(prob["points"])
        assert np.array_equal(bits(poses[p, :Cn]), bits(a)) and np.array_equal(bits(points[p, :M]), bits(x)), p
        assert np.array_equal(bits(costs[p]), bits(c)) and its[p] == i, p
    assert its[1] == 1 and bits(costs[1, 0]) == bits(costs[1, 1])
    assert np.array_equal(bits(poses[1, :1]), bits(q["poses"])) and np.array_equal(bits(points[1, :1]), bits(q["points"]))
    assert its[0] > 1 and its[2] > 1 and costs[0, 1] < costs[0, 0] and costs[2, 1] < costs[2, 0]


@pytest.mark.parametrize("scene", B.REJECT_SCENES, ids=lambda s: "C%d-M%d-seed%d-dpos%g-delta%g" % s)
def test_lm_control_follows_the_reference_through_rejected_steps(ctx, scene):
    """The device keeps lambda and the accept flags to itself, so the trajectory is
    read by running from the same start with max_iterations = 1 .. K: step k was
    rejected exactly when costs[1] has the same bits after k and after k - 1
    iterations. K (B.lm_prefix) is the prefix in which float64 and longdouble numpy
    decide alike and every decision is clear, |c_trial - c_cur| > 1e-6 c_cur; the
    CPU companion asserts K >= 8 with at least 3 rejections. For every k <= K the
    pattern equals the reference's, the cost after k iterations lies within 100 x
    the relative float64-vs-longdouble distance of the reference's cost at that k,
    the iteration count is k and the fixed cameras keep their bits.
    Measured on the MI355X, largest over k of (device distance) / (that k's bar) and the
    largest device distance itself (the costs fall to 1e-5 .. 1e-9, where both grow):
      (3, 12, 21, 0.5, 0)  K = 14  aaarrraraaaaaa    0.033 of the bar, 1.3e-8
      (3, 12, 76, 0.5, 2)  K = 16  aaararararararaa  0.057 of the bar, 8.0e-9
      (4, 40, 12, 1.0, 0)  K = 12  aarrraaaaaaa      0.34 of the bar, 5.7e-10"""
    Cn, M, seed, dpos, delta = scene
    q = B.reject_scene(Cn, M, seed, dpos)
    K, h64, hld = B.lm_prefix(q, delta, B.REJECT_ITERATIONS)
    prev, pattern, worst, worst_d = None, "", 0.0, 0.0
    for k in range(1, K + 1):
        poses, points, costs, it = call(ctx, ctx.bundle_adjust, q, huber_delta=delta, max_iterations=k)
        if prev is None:
            prev = costs[0]
            assert np.isclose(costs[0], h64[0]["c_cur"], rtol=1e-10)
        rejected = bits(costs[1]) == bits(prev)
        prev = costs[1]
        pattern += "r" if rejected else "a"
        ref, ld = float(h64[k - 1]["cost"]), hld[k - 1]["cost"]
        bar = 100 * float(abs(h64[k - 1]["cost"] - ld) / abs(ld))
        d = abs(costs[1] - ref) / abs(ref)
        worst, worst_d = max(worst, d / bar if bar else np.inf if d else 0.0), max(worst_d, d)
        print(f"{scene} k={k} {h64[k - 1]['event']}: cost {costs[1]:.9e} ref {ref:.9e} rel diff {d:.3e} bar {bar:.3e}")
        assert rejected == (h64[k - 1]["event"] == "reject"), (k, pattern)
        assert d <= bar, (k, d, bar)
        assert it == k
        assert np.array_equal(bits(poses[:2]), bits(q["poses"][:2]))
    print(f"{scene} K={K} pattern {pattern}: worst distance / bar {worst:.3e}, worst distance {worst_d:.3e}")
    assert pattern.count("r") >= 3


@pytest.mark.parametrize("kind", list(B.POISONED))
def test_values_that_are_not_finite_stay_in_their_problem(ctx, kind):
    """One NaN or infinity in the middle problem of three. The call succeeds (the
    binding raises on any other return code); the bad problem's poses and points
    keep their bits, its costs are NaN and its iteration count 0, as
    include/svo_gpu.h says; the neighbours come out as they do alone."""
    delta = B.POISONED[kind]
    bad = B.poisoned(kind)
    probs = [B.healthy(0), bad, B.healthy(1)]
    poses, points, costs, its = call(ctx, ctx.bundle_adjust, B.batch(probs), huber_delta=delta, max_iterations=15)
    Cn, M = len(bad["poses"]), len(bad["points"])
    assert np.array_equal(bits(poses[1, :Cn]), bits(bad["poses"]))
    assert np.array_equal(bits(points[1, :M]), bits(bad["points"]))
    assert np.all(np.isnan(costs[1])) and its[1] == 0
    for p in (0, 2):
        a, x, c, i = call(ctx, ctx.bundle_adjust, probs[p], huber_delta=delta, max_iterations=15)
        Cp, Mp = len(probs[p]["poses"]), len(probs[p]["points"])
        assert np.array_equal(bits(poses[p, :Cp]), bits(a)) and np.array_equal(bits(points[p, :Mp]), bits(x)), p
        assert np.array_equal(bits(costs[p]), bits(c)) and its[p] == i, p
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(x)) and c[1] < c[0] and i > 0
    # alone it is the same
    a, x, c, i = call(ctx, ctx.bundle_adjust, bad, huber_delta=delta, max_iterations=15)
    assert np.array_equal(bits(a), bits(bad["poses"])) and np.array_equal(bits(x), bits(bad["points"]))
    assert np.all(np.isnan(c)) and i == 0
    # svo_ba_linearize does not look for such values, and they stay in their problem there too
    lin = call(ctx, ctx.ba_linearize, B.batch(probs), lam=LAM, huber_delta=delta)
    for p in (0, 2):
        solo = call(ctx, ctx.ba_linearize, probs[p], lam=LAM, huber_delta=delta)
        Cp, Mp, n = len(probs[p]["poses"]), len(probs[p]["points"]), 6 * int(solo["n_free"])
        assert lin["n_free"][p] == solo["n_free"] and lin["status"][p] == solo["status"] == 0
        for k, cnt in (("U", Cp), ("gc", Cp), ("dc", Cp), ("V", Mp), ("gp", Mp), ("dp", Mp)):
            assert np.array_equal(bits(lin[k][p, :cnt]), bits(solo[k])), (p, k)
        assert bits(lin["cost"][p]) == bits(solo["cost"])
        assert np.array_equal(bits(lin["S"][p, :n, :n]), bits(solo["S"][:n, :n]))
        assert np.array_equal(bits(lin["b"][p, :n]), bits(solo["b"][:n]))
