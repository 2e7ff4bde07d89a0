"""The batched front end on sequences that lose their features (tests/starved_cases.py):
feature sets of 1..9 points (calculatePose's branches: fewer than 4 points, the
direct solve on 4 and 5, RANSAC from 6), dropped frames (a constant image: RANSAC
without a model, a model from garbage matches, a set rebuilt from nothing), a
sequence that never shows a corner, those mixed with healthy sequences in one
batch, and a streamed 4-frame ring on a run that creates more map points than its
map holds. Every step against the oracle loop (tests/oracle_loop.py): counts,
bit-equal feature lists, poses and map points within test_frontend_gpu's bars."""
import numpy as np
import pytest

import oracle as O
import starved_cases as C
import svo_amd as S
from svo_amd.scene import Scene
from test_frontend_gpu import _compare_step

pytestmark = pytest.mark.gpu

KEYS = ("tracked", "lk_iterations", "inliers", "added", "features")
K = Scene(C.W, C.H, seed=0).K  # the intrinsics depend on the size only


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture
def resident(ctx):
    """_resident whose front ends are closed when the test ends, passed or failed (a
    failed test's traceback would otherwise keep them past their context)."""
    made = []

    def make(cases, **kw):
        made.append(_resident(ctx, cases, **kw))
        return made[-1]

    yield make
    for fe in made:
        fe.close()


def _resident(ctx, cases, **kw):
    """A front end with the cases' frames resident, one sequence per case."""
    T, n = cases[0].frames, cases[0].n
    assert all(c.frames == T and c.n == n for c in cases)
    fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, K, n_seq=len(cases), n_frames=T, n_features=n, **kw))
    for s, c in enumerate(cases):
        for t, (L, R) in enumerate(C.frames(c)):
            fe.set_frame(s, t, L, R)
    return fe


def _compare_init(fe, traces):
    for q, tr in enumerate(traces):
        assert np.array_equal(fe.features(q), tr[0].pts), f"seq {q} features at init"
        np.testing.assert_allclose(fe.map_points(q), tr[0].X, rtol=2e-5, atol=1e-6)
        assert np.array_equal(np.r_[fe.pose(q)], np.zeros(6))


def _compare_batch(fe, traces, st, t):
    """_compare_step for every sequence of a batch: the step's counts are sums over
    the batch, the feature lists (hence each sequence's own count), poses and map
    points are per sequence."""
    for k in KEYS:
        want = sum(tr[t].stats[k] for tr in traces)
        assert st[k] == want, f"{k} differs at t={t}: {st[k]} vs {want}"
    # the front end reports counts for the batch only: _compare_step gets the oracle's
    # own statistics twice, so of its checks only the feature list (hence the feature
    # count), the pose and the map points are per sequence here
    for q, tr in enumerate(traces):
        _compare_step(fe, tr[t], tr[t].stats, tr[t].stats, t, seq=q)


def _follow(fe, cases):
    """init + every step of the cases' frames against their oracle loops; returns
    what _compare_step reads, per step and sequence, for bit-equality checks."""
    traces = [C.oracle_trace(c) for c in cases]
    fe.init(0)
    _compare_init(fe, traces)
    seen = []
    for t in range(1, cases[0].frames):
        st = fe.step(t).as_dict()
        _compare_batch(fe, traces, st, t)
        seen.append([(fe.features(q), np.r_[fe.pose(q)], fe.map_points(q)) for q in range(len(cases))])
    return seen


# ---------------------------------------------------------------- 1. small sets
def test_ladder_covers_every_pose_branch():
    """The oracle side of the ladder: tracked counts 0..5 and >= 6 all occur."""
    counts = set()
    for c in C.LADDER:
        counts |= set(C.tracked_counts(c))
    assert {0, 1, 2, 3, 4, 5} <= counts and max(counts) >= 6, sorted(counts)


@pytest.mark.parametrize("case", C.LADDER, ids=lambda c: f"seed{c.seed}-n{c.n}")
def test_small_set_ladder(resident, case):
    """n_features 1..9: with fewer than 4 tracked points the features are kept and
    the pose is the identity (the oracle loop's rule where solvePnPRansac would
    throw), 4 and 5 points are solved directly, 6 and more by RANSAC."""
    fe = resident([case])
    _follow(fe, [case])
    tr = C.oracle_trace(case)
    for t in range(1, case.frames):
        if tr[t].stats["tracked"] < 4:
            assert tr[t].stats["inliers"] == tr[t].stats["tracked"]
            assert not np.any(tr[t].pose[0]) and not np.any(tr[t].pose[1])
    fe.close()


# ---------------------------------------------------------------- 2. dropped frames
def _assert_dropped_conditions(case, garbage):
    stats = [s.stats for s in C.oracle_trace(case)[1:]]
    assert any(C.is_no_model(s) for s in stats), "no step without a model"
    assert any(C.is_rebuild(s) for s in stats), "no step that rebuilds the set from nothing"
    assert any(C.is_garbage_model(s) for s in stats) == garbage, "a model from garbage matches"


@pytest.mark.parametrize("side", ["both", "right", "left"])
@pytest.mark.parametrize("base", [C.DROPPED_64, C.DROPPED_300], ids=["n64", "n300"])
def test_dropped_frames(resident, base, side):
    """A constant-128 image at t = 3 and t = 6, on both sides or one. With the left
    image gone the temporal LK loses most points and matches the rest to noise: at
    N = 64 RANSAC accepts a 6-inlier model out of 36 garbage matches at t = 3 and
    finds none at t = 6; at N = 300 it finds none at either (178 and 170 tracked,
    100 hypotheses). The next frame tracks nothing and rebuilds the set. With only
    the right image gone the keyframe's stereo LK finds nothing to add."""
    case = base._replace(side=side)
    if side != "right":
        _assert_dropped_conditions(case, garbage=base.n == 64)
    else:
        assert all(s.stats["added"] == 0 for t, s in enumerate(C.oracle_trace(case)) if t in case.drops)
    fe = resident([case])
    _follow(fe, [case])
    fe.close()


def test_dropped_frames_bucketed(resident):
    """Bucketing (50, 4) picks other features: 32 and 31 points survive the drops at
    t = 3 and t = 6 and RANSAC finds no model at either, so this run has the
    no-model and the rebuild steps but no model from garbage."""
    case = C.DROPPED_64._replace(bucket=(50, 4))
    _assert_dropped_conditions(case, garbage=False)
    fe = resident([case], bucket_size=50, per_bucket=4)
    _follow(fe, [case])
    fe.close()


# ---------------------------------------------------------------- 3. never a corner
@pytest.mark.parametrize("n_seq", [1, 2])
def test_never_any_corner(resident, n_seq):
    """A constant image from frame 0: no feature at init or at any step, identity
    pose, no error -- alone and as one of two (beside a healthy sequence)."""
    cases = [C.BLANK] + [C.BLANK._replace(blank=False)] * (n_seq - 1)
    fe = resident(cases)
    seen = _follow(fe, cases)
    for step in seen:
        f, pose, X = step[0]
        assert f.shape == (0, 2) and X.shape == (0, 3) and not pose.any()
    fe.close()


# ---------------------------------------------------------------- 4. mixed batch
MIXED = [C.BLANK._replace(blank=False), C.DROPPED_64, C.BLANK, C.BLANK._replace(seed=9, blank=False)]


@pytest.mark.parametrize("spec", ["32", "-1"])
def test_mixed_batch_and_independence(resident, spec, monkeypatch):
    """Healthy, dropped, always blank and a second healthy sequence in one front
    end, each against its own oracle loop; then each healthy sequence alone: the
    starved neighbours change nothing, bit for bit."""
    monkeypatch.setenv("SVO_FE_SPEC_MARGIN", spec)
    fe = resident(MIXED)
    seen = _follow(fe, MIXED)
    fe.close()
    for q in (0, 3):
        solo = resident([MIXED[q]])
        alone = _follow(solo, [MIXED[q]])
        solo.close()
        for t, (a, b) in enumerate(zip(alone, seen), 1):
            for x, y, what in zip(a[0], b[q], ("features", "pose", "map points")):
                assert np.array_equal(x, y), f"seq {q} {what} at t={t}: alone vs in the batch"


# ---------------------------------------------------------------- 5. OpenCV-order LK
def test_dropped_frames_opencv_order(resident):
    """SVO_LK_OPENCV_ORDER against the oracle's ACC_SSE: the float sums move the
    garbage matches (36 and 33 tracked at the drops) and RANSAC finds no model at
    either drop, so no model from garbage here either (N = 64 in the exact order
    has one, test_dropped_frames)."""
    case = C.DROPPED_64._replace(acc=O.ACC_SSE)
    _assert_dropped_conditions(case, garbage=False)
    fe = resident([case], lk_flags=S.LK_GET_MIN_EIGENVALS | S.LK_OPENCV_ORDER)
    _follow(fe, [case])
    fe.close()


# ---------------------------------------------------------------- 6. streamed ring
def _stream_and_follow(ctx, case):
    """The case streamed with queue_frames into a ring of n_frames = 4 (frame t + 2
    queued before step t), every step against its oracle loop."""
    T = case.frames
    fr = C.frames(case)
    tr = C.oracle_trace(case)
    fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, K, n_seq=1, n_frames=4, n_features=case.n))
    try:
        for t in range(3):
            fe.queue_frames(t, [fr[t][0]], [fr[t][1]])
        fe.init(0)
        _compare_init(fe, [tr])
        for t in range(1, T):
            if t + 2 < T:
                fe.queue_frames(t + 2, [fr[t + 2][0]], [fr[t + 2][1]])
            st = fe.step(t).as_dict()
            _compare_step(fe, tr[t], st, tr[t].stats, t)
        fe.upload_wait(T - 1)
    finally:
        fe.close()


def test_streamed_ring_past_the_map_capacity(ctx):
    """queue_frames into a ring of n_frames = 4 with every third frame dropped, 24
    steps: the keyframes create 506 map points in all, 442 by t = 19, against the
    ring's 6 * 64 = 384 map slots. The keyframe that would overflow the map (t = 19,
    a rebuild from nothing: no live feature, so nothing moves) reclaims it, and the
    loop follows the oracle to the end."""
    case = C.STREAMED
    T = case.frames
    cum = C.cumulative_added(case)
    assert cum[T - 2] > 6 * case.n, cum
    full_at = next(t for t in range(T) if cum[t] > 6 * case.n)
    assert C.oracle_trace(case)[full_at].stats["added"] > 0 and full_at < T - 3
    occ = C.map_occupancy(case)
    assert [t for t in range(1, T) if occ[t].reclaim] == [full_at] and occ[full_at].n == 0
    _stream_and_follow(ctx, case)


@pytest.mark.parametrize("spec", ["32", "-1"])
def test_streamed_ring_reclaims_live_map_points(ctx, spec, monkeypatch):
    """The reclaim with live features to move (C.RECLAIM, N = 450: 6 * 512 = 3072 map
    slots). Five dropped frames and their rebuilds create 2512 map points by t = 12;
    from then on every second frame loses the features of its left 100 columns and
    the next frame replaces them (~145 new points). At t = 19 the map holds 2937
    points, the keyframe keeps 269 features -- more than one 256-thread chunk, their
    ids scattered over the map -- and takes 147 candidates: 3084 > 3072, so their
    map points move to slots 0..268 in place. The 5 steps after it gather through
    the renumbered ids (post-LK) and append behind them; map_points every step.
    SVO_FE_SPEC_MARGIN 32: the fused keyframe kernel reclaims; -1: the serial
    tail kernel."""
    monkeypatch.setenv("SVO_FE_SPEC_MARGIN", spec)
    case = C.RECLAIM
    first = C.assert_reclaim_moves_live_points(case)
    assert first <= case.frames - 5  # steps follow that gather through the renumbered ids
    _stream_and_follow(ctx, case)
