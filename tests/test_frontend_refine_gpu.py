"""svo_frontend_refine_poses: the motion-only stereo refinement of the newest
window frame, from the ring on the device, on the smallest healthy sequence of
tests/starved_cases.py. The device path against svo_refine_poses_stereo on the
arrays read back beforehand (bit for bit), with a stereo ring plus
set_stereo_tracking and with a plain ring; nothing but that slot's pose moves and
the loop goes on as if the call had never been made; no window, no call."""
import numpy as np
import pytest

import svo_amd as S
from stereo_rows_reference import DEFAULTS
from test_frontend_window_gpu import HEALTHY, K, bits, same_state, state
from test_frontend_window_stereo_gpu import baseline_of, ctx, make  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

WINDOW, STEPS, DELTA, ITERS = 3, 4, 2.0, 10
CASES = [HEALTHY, HEALTHY._replace(seed=5)]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def started(make, stereo, track):
    fe = make(CASES, window=WINDOW, stereo=stereo)
    if track:
        fe.set_stereo_tracking(S.StereoRowsParams(**DEFAULTS), 4)
    fe.init(0)
    for t in range(1, STEPS + 1):
        fe.step(t)
    return fe


def host_refine(ctx, fe, stereo):
    """svo_refine_poses_stereo on every sequence's newest window frame as the host
    reads it: window(), its right columns, the live map points (the newest frame's
    list is the live one) -> (poses, costs, iterations, counts)."""
    wins = [fe.window(q) for q in range(len(CASES))]
    pts = [fe.map_points(q) for q in range(len(CASES))]
    counts = np.array([len(w["ids"][-1]) for w in wins], np.int32)
    n = max(int(counts.max()), 1)
    X, xy = np.zeros((len(CASES), n, 3)), np.zeros((len(CASES), n, 2), np.float32)
    ur = np.full((len(CASES), n), -1.0, np.float32)
    for q, (w, x) in enumerate(zip(wins, pts)):
        assert len(x) == counts[q] and np.all(np.diff(w["ids"][-1]) > 0)
        X[q, :counts[q]], xy[q, :counts[q]] = x, w["xy"][-1]
        if stereo:
            ur[q, :counts[q]] = w["ur"][-1]
    T = np.stack([w["poses"][-1] for w in wins])
    poses, costs, its, _ = ctx.refine_poses_stereo(X, xy, ur, T, K, baseline_of(fe), counts=counts,
                                                   huber_delta=DELTA, max_iterations=ITERS)
    return poses, costs, its, counts, wins


@pytest.mark.parametrize("stereo", [True, False], ids=["stereo ring + tracking", "plain ring"])
def test_device_equals_host_and_nothing_else_moves(ctx, make, stereo):
    fe = started(make, stereo, track=stereo)
    twin = started(make, stereo, track=stereo)
    want_poses, want_costs, want_its, want_counts, before = host_refine(ctx, fe, stereo)
    if stereo:  # tracked features carry their own columns: most of the list is stereo
        assert all(np.mean(w["ur"][-1] >= 0) > 0.5 for w in before)
    st0 = state(fe, len(CASES))
    costs, its, counts = fe.refine_poses(DELTA, ITERS)
    assert np.array_equal(counts, want_counts) and np.all(counts > 10), (counts, want_counts)
    assert np.array_equal(its, want_its) and np.all(its > 0), (its, want_its)
    assert np.array_equal(bits(costs), bits(want_costs)), (costs, want_costs)
    assert np.all(costs[:, 1] <= costs[:, 0])
    after = [fe.window(q) for q in range(len(CASES))]
    moved = 0
    for q, (a, b) in enumerate(zip(after, before)):
        assert np.array_equal(bits(a["poses"][-1]), bits(want_poses[q])), f"seq {q} newest pose"
        moved += not np.array_equal(bits(a["poses"][-1]), bits(b["poses"][-1]))
        # the older slots' poses and the ring's lists keep their bits
        assert np.array_equal(a["frame_t"], b["frame_t"]) and len(a["frame_t"]) == WINDOW
        assert np.array_equal(bits(a["poses"][:-1]), bits(b["poses"][:-1])), q
        for k in ("ids", "xy") + (("ur",) if stereo else ()):
            assert all(np.array_equal(u32(x) if x.dtype == np.float32 else x, u32(y) if y.dtype == np.float32 else y)
                       for x, y in zip(a[k], b[k])), (q, k)
    assert moved == len(CASES)
    # svo_frontend_pose, features and map_points keep their bits, and the loop goes
    # on as the twin's that never made the call
    assert same_state(state(fe, len(CASES)), st0)
    assert same_state(st0, state(twin, len(CASES)))
    for t in range(STEPS + 1, STEPS + 3):
        a, b = fe.step(t).as_dict(), twin.step(t).as_dict()
        for k in ("tracked", "lk_iterations", "inliers", "added", "features"):
            assert a[k] == b[k], (k, t)
        assert same_state(state(fe, len(CASES)), state(twin, len(CASES))), t
    # a second call starts from the refined pose; max_iterations = 0 only linearises
    c2, i2, n2 = fe.refine_poses(DELTA, 0)
    assert np.all(i2 == 0) and np.array_equal(bits(c2[:, 0]), bits(c2[:, 1]))


def test_without_a_window_the_call_is_refused(ctx, make):
    fe = make(CASES)
    fe.init(0)
    fe.step(1)
    with pytest.raises(S.SvoError):
        fe.refine_poses(DELTA, ITERS)
    assert "no window" in S.lib().svo_last_error(ctx.handle).decode()
    fe = make(CASES, window=WINDOW)
    fe.init(0)
    with pytest.raises(S.SvoError):
        fe.refine_poses(DELTA, 1001)
