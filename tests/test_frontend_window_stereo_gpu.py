"""The batched front end's stereo window (svo_frontend_window_enable_stereo /
_window_right / _bundle_adjust_stereo) on the 320x240 sequences of
tests/starved_cases.py: the ring's right columns against an oracle loop that keeps
the stereo matches the reference drops, off means off, the device path against
svo_bundle_adjust_stereo on the same window built on the host (bit for bit), and
the points of the newest keyframe, which only the stereo adjustment moves."""
import numpy as np
import pytest

import oracle as O
import starved_cases as C
import svo_amd as S
from oracle_loop import STEREO, Y_THRESHOLD, OracleLoop
from test_frontend_window_gpu import DELTA, HEALTHY, ITERS, N_FIXED, K, Points, bits, run_steps, same_state, state

pytestmark = pytest.mark.gpu


class StereoOracleLoop(OracleLoop):
    """OracleLoop that keeps what _keyframe drops: the right points of the matches
    that became features. ur: per current feature the right column of the match
    that created it in this frame, -1 for a feature tracked into it."""

    def _keyframe(self, left, right, cand, T, t):
        new = np.ascontiguousarray(cand, np.float32)
        self.new_ur = np.zeros(0, np.float32)
        if len(new):
            nr, st, _, _ = O.lk(left, right, new, STEREO["win"], STEREO["max_level"], STEREO["criteria"],
                                STEREO["flags"], acc=self.acc, want_err=False)
            keep = (st == 1) & (np.abs(nr[:, 1] - new[:, 1]) < Y_THRESHOLD)
            _, xyz = O.triangulate(self.P_left, self.P_right, new[keep], nr[keep])
            self.new_ur = nr[keep][xyz[:, 2] > 0][:, 0].astype(np.float32)
        out = super()._keyframe(left, right, cand, T, t)
        assert len(out[0]) == len(self.new_ur)
        return out

    @property
    def ur(self):
        return np.r_[np.full(len(self.pts) - len(self.new_ur), -1.0, np.float32), self.new_ur].astype(np.float32)


def stereo_trace(case):
    """Per frame (pts, mid, ur) of the case's oracle loop."""
    fr = C.frames(case)
    ref = StereoOracleLoop(C.scene(case), case.n, bucket=case.bucket, acc=case.acc).init(0, *fr[0])
    out = [(ref.pts.copy(), ref.mid.copy(), ref.ur)]
    for t in range(1, case.frames):
        ref.step(t, *fr[t])
        out.append((ref.pts.copy(), ref.mid.copy(), ref.ur))
    return out


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture
def make(ctx):
    """Front ends with the cases' frames resident (one sequence per case), closed when
    the test ends; stereo: None = no window, False = the plain one, True = the stereo one."""
    made = []

    def _make(cases, window=None, stereo=True):
        T, n = cases[0].frames, cases[0].n
        fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, K, n_seq=len(cases), n_frames=T, n_features=n))
        made.append(fe)
        for s, c in enumerate(cases):
            for t, (L, R) in enumerate(C.frames(c)):
                fe.set_frame(s, t, L, R)
        if window:
            fe.window_enable(window, stereo=stereo)
        return fe

    yield _make
    for fe in made:
        fe.close()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_window_follows(w, tr, frames, tag):
    assert list(w["frame_t"]) == frames, (tag, w["frame_t"])
    for j, f in enumerate(frames):
        pts, _, ur = tr[f]
        assert np.array_equal(u32(w["xy"][j]), u32(pts)), (tag, f)
        assert len(w["ur"][j]) == len(ur) and np.array_equal(u32(w["ur"][j]), u32(ur)), (tag, f, w["ur"][j], ur)


# ---------------------------------------------------------------- 1. contents
def test_ring_keeps_the_creating_match(make):
    """Window 6 over 8 resident frames (the ring wraps): after init and every step
    each valid frame's right columns are the oracle's, bit for bit -- every feature
    of frame 0, the features a later keyframe adds; -1 for the tracked ones."""
    tr = stereo_trace(HEALTHY)
    assert np.all(tr[0][2] >= 0) and len(tr[0][2]) > 0
    created = [t for t in range(1, 8) if np.any(tr[t][2] >= 0)]
    assert created and all(np.any(tr[t][2] < 0) for t in created)  # lists with both kinds
    fe = make([HEALTHY], window=6)
    fe.init(0)
    for t in range(0, 8):
        if t:
            fe.step(t)
        assert_window_follows(fe.window(0), tr, list(range(max(0, t - 5), t + 1)), t)


def test_ring_through_a_map_reclaim(ctx):
    """C.STREAMED into a ring of 4 frames, 24 steps, window 4 (test_frontend_window_gpu's
    reclaim run: dropped frames empty the list and keyframes rebuild it, the map is
    reclaimed once): the right columns of the valid frames follow the oracle throughout."""
    case = C.STREAMED
    T = case.frames
    at = [t for t in range(1, T) if C.map_occupancy(case)[t].reclaim]
    assert len(at) == 1, at
    tr = stereo_trace(case)
    fr = C.frames(case)
    fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, K, n_seq=1, n_frames=4, n_features=case.n))
    try:
        fe.window_enable(4, stereo=True)
        for t in range(3):
            fe.queue_frames(t, [fr[t][0]], [fr[t][1]])
        fe.init(0)
        assert_window_follows(fe.window(0), tr, [0], 0)
        for t in range(1, T):
            if t + 2 < T:
                fe.queue_frames(t + 2, [fr[t + 2][0]], [fr[t + 2][1]])
            fe.step(t)
            first = max(at[0], t - 3) if t >= at[0] else max(0, t - 3)
            assert_window_follows(fe.window(0), tr, list(range(first, t + 1)), t)
        fe.upload_wait(T - 1)
    finally:
        fe.close()


# ---------------------------------------------------------------- 2. off means off
def test_plain_window_is_unchanged_and_refuses_the_stereo_calls(make):
    """The same run with the plain window and with the stereo one: states and window
    readbacks bit-identical after every step; the plain one has no right columns,
    and svo_frontend_window_right / _bundle_adjust_stereo return errors on it."""
    cases = [HEALTHY, C.DROPPED_64]
    seen = []
    for stereo in (False, True):
        fe = make(cases, window=4, stereo=stereo)
        fe.init(0)
        run = []
        for t in range(0, 7):
            if t:
                fe.step(t)
            run.append((state(fe, 2), [fe.window(q) for q in range(2)]))
        if not stereo:
            assert all("ur" not in w for w in run[-1][1])
            with pytest.raises(S.SvoError):
                fe.window_right(0)
            with pytest.raises(S.SvoError):
                fe.bundle_adjust(N_FIXED, DELTA, ITERS, stereo=True)
            assert "no stereo window" in S.lib().svo_last_error(fe.ctx.handle).decode()
        seen.append(run)
        fe.close()
    for t, ((sa, wa), (sb, wb)) in enumerate(zip(*seen)):
        assert same_state(sa, sb), f"t={t}"
        for a, b in zip(wa, wb):
            assert np.array_equal(a["frame_t"], b["frame_t"]) and np.array_equal(bits(a["poses"]), bits(b["poses"])), t
            for k in ("ids", "xy"):
                assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), (t, k)
    # without any window both are refused as well
    fe = make([HEALTHY])
    with pytest.raises(S.SvoError):
        fe.bundle_adjust(N_FIXED, DELTA, ITERS, stereo=True)
    for bad in (0, 17):
        with pytest.raises(S.SvoError):
            fe.window_enable(bad, stereo=True)


# ---------------------------------------------------------------- 3. device path = host path
def baseline_of(fe):
    return -float(fe.cfg.P_right[3]) / float(fe.cfg.P_right[0])


def host_adjust(ctx, fe, pts, window, stereo, n_fixed=N_FIXED, delta=DELTA, iters=ITERS):
    """svo_bundle_adjust(_stereo) on every sequence's window as the host reads it
    (test_frontend_window_gpu.host_adjust with the right columns beside the pixels)
    -> (poses per seq, points per seq by id, costs, iterations, sizes)."""
    n_seq = len(pts.by_id)
    wins = [fe.window(q) for q in range(n_seq)]
    pids = [np.unique(np.concatenate(w["ids"] + [np.zeros(0, np.int32)])).astype(np.int32) for w in wins]
    nobs = [sum(len(a) for a in w["ids"]) for w in wins]
    Mx, Ox = max(1, max(len(p) for p in pids)), max(1, max(nobs))
    poses = np.zeros((n_seq, window, 12))
    fixed = np.ones((n_seq, window), np.uint8)
    points = np.zeros((n_seq, Mx, 3))
    oc, op = np.zeros((n_seq, Ox), np.int32), np.zeros((n_seq, Ox), np.int32)
    oxy, our = np.zeros((n_seq, Ox, 2), np.float32), np.zeros((n_seq, Ox), np.float32)
    nc = np.array([len(w["frame_t"]) for w in wins], np.int32)
    for q, (w, pid) in enumerate(zip(wins, pids)):
        V = nc[q]
        poses[q, :V] = w["poses"]
        fixed[q, :V] = np.arange(V) < n_fixed
        points[q, : len(pid)] = np.array([pts.by_id[q][int(i)] for i in pid]).reshape(-1, 3)
        k = 0
        for j, (ids, xy, ur) in enumerate(zip(w["ids"], w["xy"], w["ur"])):
            oc[q, k: k + len(ids)] = j
            op[q, k: k + len(ids)] = np.searchsorted(pid, ids)
            oxy[q, k: k + len(ids)] = xy
            our[q, k: k + len(ids)] = ur
            k += len(ids)
    nm, no = np.array([len(p) for p in pids], np.int32), np.array(nobs, np.int32)
    kw = dict(obs_ur=our, baseline=baseline_of(fe)) if stereo else {}
    rp, rx, costs, its = ctx.bundle_adjust(poses, fixed, points, oc, op, oxy, K, n_cams=nc, n_points=nm, n_obs=no,
                                           huber_delta=delta, max_iterations=iters, **kw)
    by_id = [{int(i): rx[q, k] for k, i in enumerate(pid)} for q, pid in enumerate(pids)]
    return [rp[q, : nc[q]] for q in range(n_seq)], by_id, costs, its, np.stack([nc, nm, no], 1)


def assert_device_equals_host(ctx, fe, pts, window, stereo):
    """test_frontend_window_gpu.assert_device_equals_host for either adjustment."""
    n_seq = len(pts.by_id)
    want_poses, want_pts, want_costs, want_its, want_sizes = host_adjust(ctx, fe, pts, window, stereo)
    live = [fe.window(q)["ids"] for q in range(n_seq)]
    costs, its, sizes = fe.bundle_adjust(N_FIXED, DELTA, ITERS, stereo=stereo)
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


BATCH = [HEALTHY, C.BLANK, C.DROPPED_64]


def test_device_stereo_adjustment_equals_host_adjustment(ctx, make):
    """Healthy, never-a-corner and dropped-frame sequences in one batch, 7 steps,
    window 5: svo_frontend_bundle_adjust_stereo equals svo_bundle_adjust_stereo on
    the windows built on the host from window() and its right columns; poses, live
    map points, costs, iterations and sizes, bit for bit."""
    fe = make(BATCH, window=5)
    pts = Points(len(BATCH))
    run_steps(fe, len(BATCH), 7, pts)
    assert any(np.any(u >= 0) for u in fe.window(0)["ur"]) and any(np.any(u < 0) for u in fe.window(0)["ur"])
    costs, its, sizes, _ = assert_device_equals_host(ctx, fe, pts, 5, True)
    assert sizes[0, 0] == 5 and sizes[0, 2] > sizes[0, 1] > 0 and list(sizes[1]) == [5, 0, 0]
    assert its[0] > 0 and costs[0, 1] <= costs[0, 0]


# ---------------------------------------------------------------- 4. the newest keyframe
def test_only_the_stereo_adjustment_moves_the_newest_keyframes_points(ctx, make):
    """Two identical runs, 7 steps, window 4: the points created at the newest frame
    are seen by that camera alone. The monocular adjustment returns their bits; the
    stereo one moves every one of them (each has its stereo observation), and both
    equal their host counterparts."""
    moved = {}
    for stereo in (False, True):
        fe = make([HEALTHY], window=4)
        pts = Points(1)
        run_steps(fe, 1, 7, pts)
        w = fe.window(0)
        older = np.concatenate(w["ids"][:-1])
        new = np.flatnonzero(~np.isin(w["ids"][-1], older))
        assert len(new) >= 3 and np.all(w["ur"][-1][new] >= 0) and np.all(w["ur"][-1][np.isin(w["ids"][-1], older)] < 0)
        before = fe.map_points(0)
        assert_device_equals_host(ctx, fe, pts, 4, stereo)
        after = fe.map_points(0)
        moved[stereo] = [not np.array_equal(bits(before[i]), bits(after[i])) for i in new]
        assert not np.array_equal(bits(before), bits(after))  # the shared points move either way
        fe.close()
    assert not any(moved[False]) and all(moved[True]), moved
