"""The batched front end's observation window and its device-resident bundle
adjustment (svo_frontend_window_enable / _window / _bundle_adjust) on the 320x240
sequences of tests/starved_cases.py: the ring's contents against the oracle loop,
off means off, the device path against svo_bundle_adjust on the same window built
on the host (bit for bit), the effect on the loop, degenerate windows, the map
reclaim of a streamed ring, and the argument checks."""
import numpy as np
import pytest

import oracle as O
import starved_cases as C
import svo_amd as S
from svo_amd.scene import Scene

pytestmark = pytest.mark.gpu

K = Scene(C.W, C.H, seed=0).K  # the intrinsics depend on the size only
HEALTHY = C.BLANK._replace(blank=False)
IDENTITY = np.r_[np.eye(3).ravel(), np.zeros(3)]
N_FIXED, DELTA, ITERS = 2, 2.0, 5


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture
def make(ctx):
    """Front ends with the cases' frames resident (one sequence per case), closed when
    the test ends."""
    made = []

    def _make(cases, window=None, steps=None):
        T, n = cases[0].frames, cases[0].n
        fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, K, n_seq=len(cases), n_frames=T, n_features=n))
        made.append(fe)
        for s, c in enumerate(cases):
            for t, (L, R) in enumerate(C.frames(c)):
                fe.set_frame(s, t, L, R)
        if window:
            fe.window_enable(window)
        return fe

    yield _make
    for fe in made:
        fe.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def state(fe, n_seq):
    return [(fe.features(q), np.r_[fe.pose(q)], fe.map_points(q)) for q in range(n_seq)]


def same_state(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) if x.dtype == np.float32
               else np.array_equal(bits(x), bits(y)) for p, q in zip(a, b) for x, y in zip(p, q))


class Points:
    """The map points of each sequence by map id, collected step by step from the
    live features (svo_frontend_map_points reads live features only): an id named
    by a window frame was live at that frame, and a point moves only in a bundle
    adjustment."""

    def __init__(self, n_seq):
        self.by_id = [dict() for _ in range(n_seq)]

    def collect(self, fe):
        for q, d in enumerate(self.by_id):
            w = fe.window(q)
            if len(w["frame_t"]) == 1:  # init, or the map was reclaimed: the ids start over
                d.clear()
            X = fe.map_points(q)
            ids = w["ids"][-1] if len(w["ids"]) else np.zeros(0, np.int32)
            assert len(ids) == len(X)
            for i, x in zip(ids, X):
                d[int(i)] = x.copy()


def host_adjust(ctx, fe, pts, window, n_fixed=N_FIXED, delta=DELTA, iters=ITERS):
    """svo_bundle_adjust on every sequence's window as the host reads it: cameras in
    slot order, points numbered by ascending id, max_points / max_obs the batch's
    largest -> (poses per seq (V, 12), points per seq by id dict, costs, iterations, sizes)."""
    n_seq = len(pts.by_id)
    wins = [fe.window(q) for q in range(n_seq)]
    pids = [np.unique(np.concatenate(w["ids"] + [np.zeros(0, np.int32)])).astype(np.int32) for w in wins]
    nobs = [sum(len(a) for a in w["ids"]) for w in wins]
    Mx, Ox = max(1, max(len(p) for p in pids)), max(1, max(nobs))
    poses = np.zeros((n_seq, window, 12))
    fixed = np.ones((n_seq, window), np.uint8)
    points = np.zeros((n_seq, Mx, 3))
    oc, op = np.zeros((n_seq, Ox), np.int32), np.zeros((n_seq, Ox), np.int32)
    oxy = np.zeros((n_seq, Ox, 2), np.float32)
    nc = np.array([len(w["frame_t"]) for w in wins], np.int32)
    for q, (w, pid) in enumerate(zip(wins, pids)):
        V = nc[q]
        poses[q, :V] = w["poses"]
        fixed[q, :V] = np.arange(V) < n_fixed
        points[q, : len(pid)] = np.array([pts.by_id[q][int(i)] for i in pid]).reshape(-1, 3)
        k = 0
        for j, (ids, xy) in enumerate(zip(w["ids"], w["xy"])):
            assert np.all(np.diff(ids) > 0)
            oc[q, k: k + len(ids)] = j
            op[q, k: k + len(ids)] = np.searchsorted(pid, ids)
            oxy[q, k: k + len(ids)] = xy
            k += len(ids)
    nm, no = np.array([len(p) for p in pids], np.int32), np.array(nobs, np.int32)
    rp, rx, costs, its = ctx.bundle_adjust(poses, fixed, points, oc, op, oxy, K, n_cams=nc, n_points=nm, n_obs=no,
                                           huber_delta=delta, max_iterations=iters)
    by_id = [{int(i): rx[q, k] for k, i in enumerate(pid)} for q, pid in enumerate(pids)]
    return [rp[q, : nc[q]] for q in range(n_seq)], by_id, costs, its, np.stack([nc, nm, no], 1)


def assert_device_equals_host(ctx, fe, pts, window, **kw):
    """The front end's adjustment against host_adjust on the window read just before
    it: window poses, live map points, costs, iterations and sizes, bit for bit."""
    n_seq = len(pts.by_id)
    want_poses, want_pts, want_costs, want_its, want_sizes = host_adjust(ctx, fe, pts, window, **kw)
    live = [fe.window(q)["ids"] for q in range(n_seq)]
    costs, its, sizes = fe.bundle_adjust(kw.get("n_fixed", N_FIXED), kw.get("delta", DELTA), kw.get("iters", ITERS))
    assert np.array_equal(sizes, want_sizes), (sizes, want_sizes)
    assert np.array_equal(its, want_its), (its, want_its)
    assert np.array_equal(bits(costs), bits(want_costs)), (costs, want_costs)
    for q in range(n_seq):
        assert np.array_equal(bits(fe.window(q)["poses"]), bits(want_poses[q])), f"seq {q} poses"
        X = fe.map_points(q)
        ids = live[q][-1] if len(live[q]) else np.zeros(0, np.int32)
        want = np.array([want_pts[q][int(i)] for i in ids]).reshape(-1, 3)
        assert np.array_equal(bits(X), bits(want)), f"seq {q} live map points"
    return costs, its, sizes, want_pts


def run_steps(fe, n_seq, steps, pts=None):
    fe.init(0)
    if pts:
        pts.collect(fe)
    for t in range(1, steps + 1):
        fe.step(t)
        if pts:
            pts.collect(fe)


# ---------------------------------------------------------------- 1. contents
@pytest.mark.parametrize("device_fits", ["0", "1"])
def test_window_contents_follow_the_oracle(make, device_fits, monkeypatch):
    """Window 4 over 7 steps (the ring wraps): after init and every step the valid
    frames, their counts, pixels (bit-identical), map ids (the oracle's creation
    numbers: no reclaim on a resident run) and poses ([R(rvec) | tvec] of the
    oracle's model within the loop's 1e-7; exactly the identity for frame 0). With
    the host's final fits and with the device's (SVO_FE_DEVICE_FITS)."""
    monkeypatch.setenv("SVO_FE_DEVICE_FITS", device_fits)
    tr = C.oracle_trace(HEALTHY)
    fe = make([HEALTHY], window=4)
    fe.init(0)
    for t in range(0, 8):
        if t:
            fe.step(t)
        w = fe.window(0)
        frames = list(range(max(0, t - 3), t + 1))
        assert list(w["frame_t"]) == frames, (t, w["frame_t"])
        for j, f in enumerate(frames):
            assert len(w["ids"][j]) == len(tr[f].pts), (t, f)
            assert np.array_equal(w["xy"][j].view(np.uint32), tr[f].pts.view(np.uint32)), (t, f)
            assert np.array_equal(w["ids"][j], tr[f].mid), (t, f)
            want = np.r_[O.rodrigues(np.asarray(tr[f].pose[0], np.float64)).ravel(), tr[f].pose[1]]
            d = np.abs(w["poses"][j] - want).max()
            print(f"t={t} frame {f}: pose max abs diff {d:.3e}")
            assert d <= 1e-7, (t, f, d)
            if f == 0:
                assert np.array_equal(bits(w["poses"][j]), bits(IDENTITY))
    # the same run read only at its end: every pose found its slot without the
    # reads' synchronisation between the steps
    fe2 = make([HEALTHY], window=4)
    run_steps(fe2, 1, 7)
    w2 = fe2.window(0)
    assert list(w2["frame_t"]) == list(w["frame_t"])
    assert np.array_equal(bits(w2["poses"]), bits(w["poses"]))
    for a, b in zip(w2["ids"] + w2["xy"], w["ids"] + w["xy"]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 2. off means off
def test_enabled_window_changes_nothing(make):
    """The same run with and without window_enable (and no adjustment): features,
    poses and map points bit-identical after every step."""
    cases = [HEALTHY, C.DROPPED_64]
    seen = []
    for window in (None, 4):
        fe = make(cases, window=window)
        fe.init(0)
        run = [state(fe, 2)]
        for t in range(1, 7):
            fe.step(t)
            run.append(state(fe, 2))
        seen.append(run)
        fe.close()
    for t, (a, b) in enumerate(zip(*seen)):
        assert same_state(a, b), f"t={t}"


# ---------------------------------------------------------------- 3. device path = host path
BATCH = [HEALTHY, C.BLANK, C.DROPPED_64]


def _adjusted_batch(ctx, make):
    fe = make(BATCH, window=4)
    pts = Points(len(BATCH))
    run_steps(fe, len(BATCH), 6, pts)
    out = assert_device_equals_host(ctx, fe, pts, 4)
    return fe, out, [fe.window(q)["poses"] for q in range(len(BATCH))], [fe.map_points(q) for q in range(len(BATCH))]


def test_device_adjustment_equals_host_adjustment(ctx, make):
    """Healthy, never-a-corner and dropped-frame sequences in one batch, 6 steps,
    window 4: the device-resident adjustment equals svo_bundle_adjust on the windows
    built on the host, and a second front end gives the same bits."""
    fe, (costs, its, sizes, _), poses, X = _adjusted_batch(ctx, make)
    assert sizes[0, 0] == 4 and sizes[0, 1] > 0 and sizes[0, 2] > sizes[0, 1]  # shared points
    assert list(sizes[1]) == [4, 0, 0]  # the blank sequence: frames without features
    fe.close()
    fe2, (costs2, its2, sizes2, _), poses2, X2 = _adjusted_batch(ctx, make)
    assert np.array_equal(bits(costs), bits(costs2)) and np.array_equal(its, its2)
    for q in range(len(BATCH)):
        assert np.array_equal(bits(poses[q]), bits(poses2[q])) and np.array_equal(bits(X[q]), bits(X2[q])), q


# ---------------------------------------------------------------- 4. effect on the loop
def test_adjustment_lowers_the_cost_and_the_loop_goes_on(ctx, make):
    fe = make([HEALTHY], window=4)
    pts = Points(1)
    run_steps(fe, 1, 6, pts)
    before = fe.window(0)
    costs, its, sizes, refined = assert_device_equals_host(ctx, fe, pts, 4)
    print(f"cost {costs[0, 0]:.6f} -> {costs[0, 1]:.6f} in {its[0]} iterations, sizes {sizes[0]}")
    assert costs[0, 1] <= costs[0, 0]
    after = fe.window(0)
    assert np.array_equal(bits(after["poses"][:N_FIXED]), bits(before["poses"][:N_FIXED]))
    assert not np.array_equal(bits(after["poses"][N_FIXED:]), bits(before["poses"][N_FIXED:]))
    fe.step(7)
    w = fe.window(0)
    X = fe.map_points(0)
    old = [(k, int(i)) for k, i in enumerate(w["ids"][-1]) if int(i) in refined[0]]
    assert len(old) > 10  # features that survive the step
    for k, i in old:
        assert np.array_equal(bits(X[k]), bits(refined[0][i])), (k, i)
    moved = sum(not np.array_equal(bits(refined[0][i]), bits(pts.by_id[0][i])) for _, i in old)
    assert moved > 0  # and the adjustment had moved some of them


# ---------------------------------------------------------------- 5. degenerate windows
@pytest.mark.parametrize("window,steps", [(1, 3), (4, 0)])
def test_degenerate_window_is_left_unchanged(make, window, steps):
    """Window 1, or an adjustment right after init: one frame, which is among the
    fixed ones, and every point is seen once: nothing is free."""
    fe = make([HEALTHY, C.BLANK], window=window)
    run_steps(fe, 2, steps)
    before = [(fe.window(q), fe.map_points(q)) for q in range(2)]
    costs, its, sizes = fe.bundle_adjust(N_FIXED, DELTA, ITERS)
    assert list(sizes[:, 0]) == [1, 1] and sizes[0, 1] > 0 and sizes[1, 1] == 0
    assert np.array_equal(bits(costs[:, 0]), bits(costs[:, 1]))
    for q, (w, X) in enumerate(before):
        assert np.array_equal(bits(fe.window(q)["poses"]), bits(w["poses"])), q
        assert np.array_equal(bits(fe.map_points(q)), bits(X)), q


# ---------------------------------------------------------------- 6. reclaim
def test_reclaim_shortens_the_window(ctx):
    """C.STREAMED into a ring of 4 frames, 24 steps, window 4: on the step whose
    keyframe reclaims the map (starved_cases.map_occupancy) the window holds exactly
    that frame -- the older slots name ids of the old numbering --, then it grows
    again, and an adjustment two steps later equals the host's."""
    case = C.STREAMED
    T = case.frames
    occ = C.map_occupancy(case)
    at = [t for t in range(1, T) if occ[t].reclaim]
    assert len(at) == 1 and at[0] + 2 < T, at
    at = at[0]
    fr = C.frames(case)
    fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, K, n_seq=1, n_frames=4, n_features=case.n))
    try:
        fe.window_enable(4)
        for t in range(3):
            fe.queue_frames(t, [fr[t][0]], [fr[t][1]])
        fe.init(0)
        pts = Points(1)
        pts.collect(fe)
        for t in range(1, T):
            if t + 2 < T:
                fe.queue_frames(t + 2, [fr[t + 2][0]], [fr[t + 2][1]])
            fe.step(t)
            pts.collect(fe)
            frames = list(fe.window(0)["frame_t"])
            if t < at:
                assert frames == list(range(max(0, t - 3), t + 1)), (t, frames)
            else:
                assert frames == list(range(max(at, t - 3), t + 1)), (t, frames)
            if t == at + 2:
                assert_device_equals_host(ctx, fe, pts, 4)
        fe.upload_wait(T - 1)
    finally:
        fe.close()


# ---------------------------------------------------------------- 7. arguments
def test_argument_checks(make):
    fe = make([HEALTHY])
    for bad in (0, 17):
        with pytest.raises(S.SvoError):
            fe.window_enable(bad)
    with pytest.raises(S.SvoError):
        fe.bundle_adjust(2, 0.0, 5)  # no window
    fe.init(0)
    with pytest.raises(S.SvoError):
        fe.window_enable(4)  # after init
    fe2 = make([HEALTHY], window=2)
    fe2.init(0)
    with pytest.raises(S.SvoError):
        fe2.bundle_adjust(-1, 0.0, 5)
    with pytest.raises(S.SvoError):
        fe2.bundle_adjust(1, 0.0, -1)
