"""svo_frontend_set_stereo_tracking: the stereo window's right columns of tracked
features against the restatement loops (tests/stereo_track_reference.py), bit for
bit and frame by frame; everything else against a front end that never made the
call; guide 0, the stereo LK at the keyframe, a map reclaim, streamed frames, the
stereo bundle adjustment from the new window, and the setter's refusals."""
import ctypes as C_

import numpy as np
import pytest

import starved_cases as C
import svo_amd as S
from stereo_rows_reference import DEFAULTS
from stereo_track_reference import (LOOP_FEATURES, LOOP_FRAMES, TrackedStereoLKLoop, loop_scene, tracked_trace)
from test_frontend_window_gpu import Points, same_state, state
from test_frontend_window_stereo_gpu import assert_device_equals_host

pytestmark = pytest.mark.gpu

WINDOW = 4


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_frontend(ctx, scenes, T, n_features, track=4, rows=True, window=WINDOW, resident=True):
    """track: the guide of set_stereo_tracking, None: never called."""
    sc0 = scenes[0]
    P0, P1 = sc0.projections()
    fe = S.Frontend(ctx, S.FrontendConfig(sc0.w, sc0.h, sc0.K, n_seq=len(scenes), n_frames=T, n_features=n_features,
                                          P_left=P0, P_right=P1))
    if rows:
        fe.set_stereo_matcher(S.StereoRowsParams(**DEFAULTS))
    if resident:
        for s, sc in enumerate(scenes):
            for t in range(T):
                fe.set_frame(s, t, sc.frame(t), sc.right(t))
    if window:
        fe.window_enable(window, stereo=True)
    if track is not None:
        fe.set_stereo_tracking(S.StereoRowsParams(**DEFAULTS), track)
    return fe


def assert_window(fe, q, want, t, tag=""):
    """want[f] = (pts, ur) of frame f; the window holds the last WINDOW frames up to t."""
    w = fe.window(q)
    frames = list(range(max(0, t - WINDOW + 1), t + 1))
    assert list(w["frame_t"]) == frames, (tag, t, w["frame_t"])
    for j, f in enumerate(frames):
        pts, ur = want[f]
        assert np.array_equal(u32(w["xy"][j]), u32(pts)), (tag, q, t, f)
        got = w["ur"][j]
        assert len(got) == len(ur), (tag, q, t, f)
        bad = np.flatnonzero(u32(got) != u32(ur))
        assert len(bad) == 0, (tag, q, t, f, len(bad), bad[:5], got[bad[:5]], ur[bad[:5]])
    return w


def follow(ctx, loops, guide, lk=False):
    """Front ends with and without the call in lockstep over the shared loops."""
    kind = loops[0][0]
    scenes = [loop_scene(k, s) for k, s in loops]
    traces = [tracked_trace(k, s, 4, lk) for k, s in loops]
    N, T = LOOP_FEATURES[kind], LOOP_FRAMES
    fe = make_frontend(ctx, scenes, T, N, track=guide, rows=not lk)
    plain = make_frontend(ctx, scenes, T, N, track=None, rows=not lk)
    try:
        for t in range(T):
            if t == 0:
                fe.init(0), plain.init(0)
            else:
                a, b = fe.step(t).as_dict(), plain.step(t).as_dict()
                for k in ("tracked", "lk_iterations", "inliers", "added", "features"):
                    assert a[k] == b[k], (k, t)
            assert same_state(state(fe, len(loops)), state(plain, len(loops))), t
            for q, tr in enumerate(traces):
                if guide:
                    want = [(s.pts, s.ur) for s in tr]
                else:  # the full range for every tracked feature; the created ones as ever
                    want = [(s.pts, np.r_[s.full_ur, s.ur[s.tracked:]].astype(np.float32)) for s in tr]
                w = assert_window(fe, q, want, t, (loops[q], guide))
                wp = plain.window(q)
                assert all(np.array_equal(x, y) for x, y in zip(w["ids"], wp["ids"]))
                assert all(np.array_equal(u32(x), u32(y)) for x, y in zip(w["xy"], wp["xy"]))
                if t:
                    s = tr[t]
                    got = w["ur"][-1][: s.tracked]
                    assert np.sum(got >= 0) >= 0.90 * s.tracked, (loops[q], t, int(np.sum(got >= 0)), s.tracked)
                    assert np.all(wp["ur"][-1][: s.tracked] == -1)
    finally:
        fe.close()
        plain.close()


def test_wide_scene_follows_the_restatement(ctx):
    follow(ctx, [("wide", 3)], 4)


def test_forward_batch_follows_the_restatement(ctx):
    follow(ctx, [("forward", 3), ("forward", 8)], 4)


def test_guide_zero_is_the_full_range(ctx):
    tr = tracked_trace("forward", 3)
    assert any(np.any(u32(s.full_ur) != u32(s.ur[: s.tracked])) for s in tr[1:])  # the two rules are told apart
    follow(ctx, [("forward", 3), ("forward", 8)], 0)


def test_stereo_lk_at_the_keyframe(ctx):
    follow(ctx, [("wide", 3)], 4, lk=True)


def test_map_reclaim_drops_the_priors_for_one_frame(ctx):
    """C.RECLAIM streamed into a ring of 4 frames (test_frontend_starved_gpu's run that
    fills the map while features live): the keyframe of step `first` reclaims the
    map, that frame's tracked features are matched without a prior -- the older slots
    belong to another epoch -- and the window, cut to that frame, grows again."""
    case = C.RECLAIM
    first = C.assert_reclaim_moves_live_points(case)
    occ = C.map_occupancy(case)
    fr = C.frames(case)
    T = case.frames
    sc = C.scene(case)
    ref = TrackedStereoLKLoop(sc, case.n, bucket=case.bucket, acc=case.acc).init(0, *fr[0])
    want = [(ref.pts.copy(), ref.ur.copy())]
    P0, P1 = sc.projections()
    fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, sc.K, n_seq=1, n_frames=4, n_features=case.n, P_left=P0,
                                          P_right=P1))
    try:
        fe.window_enable(WINDOW, stereo=True)
        fe.set_stereo_tracking(S.StereoRowsParams(**DEFAULTS), 4)
        for t in range(3):
            fe.queue_frames(t, [fr[t][0]], [fr[t][1]])
        fe.init(0)
        for t in range(1, T):
            if t + 2 < T:
                fe.queue_frames(t + 2, [fr[t + 2][0]], [fr[t + 2][1]])
            fe.step(t)
            ref.step(t, *fr[t], reclaim=occ[t].reclaim)
            want.append((ref.pts.copy(), ref.ur.copy()))
            if t == first:
                assert ref.tracked_n > 256 and ref.prior_n == 0 and ref.matched_n > 0.9 * ref.tracked_n
            if t == first + 1:
                assert ref.prior_n > 0.9 * ref.tracked_n
            w = fe.window(0)
            lo = max(first, t - WINDOW + 1) if t >= first else max(0, t - WINDOW + 1)
            assert list(w["frame_t"]) == list(range(lo, t + 1)), (t, w["frame_t"])
            for j, f in enumerate(range(lo, t + 1)):
                assert np.array_equal(u32(w["xy"][j]), u32(want[f][0])), (t, f)
                assert len(w["ur"][j]) == len(want[f][1]) and np.array_equal(u32(w["ur"][j]), u32(want[f][1])), (t, f)
        assert len(fe.window(0)["frame_t"]) == WINDOW
        fe.upload_wait(T - 1)
    finally:
        fe.close()


def test_streamed_frames_give_the_resident_columns(ctx):
    """queue_frames into a ring of n_frames = 4 over 8 frames (every slot is streamed
    into again while the match of its previous frame may still be queued) against the
    same frames resident."""
    T, N = 8, LOOP_FEATURES["wide"]
    sc = loop_scene("wide", 3)
    fr = [(np.ascontiguousarray(sc.frame(t)), np.ascontiguousarray(sc.right(t))) for t in range(T)]
    res = make_frontend(ctx, [sc], T, N)
    stream = make_frontend(ctx, [sc], 4, N, resident=False)
    try:
        for t in range(3):
            stream.queue_frames(t, [fr[t][0]], [fr[t][1]])
        res.init(0), stream.init(0)
        for t in range(1, T):
            if t + 2 < T:
                stream.queue_frames(t + 2, [fr[t + 2][0]], [fr[t + 2][1]])
            res.step(t), stream.step(t)
            a, b = res.window(0), stream.window(0)
            assert list(a["frame_t"]) == list(b["frame_t"]) == list(range(max(0, t - WINDOW + 1), t + 1))
            for k in ("xy", "ur"):
                assert all(np.array_equal(u32(x), u32(y)) for x, y in zip(a[k], b[k])), (t, k)
            assert np.sum(a["ur"][-1] >= 0) > 0.9 * len(a["ur"][-1])
        stream.upload_wait(T - 1)
    finally:
        res.close()
        stream.close()


def test_stereo_bundle_adjustment_from_the_tracked_window(ctx):
    """svo_frontend_bundle_adjust_stereo from the window with every frame's columns
    equals svo_bundle_adjust_stereo on the same window built on the host, bit for
    bit; at least 90 % of the staged observations carry a right column."""
    sc = loop_scene("wide", 3)
    fe = make_frontend(ctx, [sc], LOOP_FRAMES, LOOP_FEATURES["wide"])
    try:
        pts = Points(1)
        fe.init(0)
        pts.collect(fe)
        for t in range(1, LOOP_FRAMES):
            fe.step(t)
            pts.collect(fe)
        ur = np.concatenate(fe.window(0)["ur"])
        assert np.sum(ur >= 0) >= 0.90 * len(ur), (int(np.sum(ur >= 0)), len(ur))
        costs, its, sizes, _ = assert_device_equals_host(ctx, fe, pts, WINDOW, True)
        assert sizes[0, 0] == WINDOW and sizes[0, 2] == len(ur) and its[0] > 0 and costs[0, 1] <= costs[0, 0]
    finally:
        fe.close()


def test_the_setter_is_refused_out_of_place_and_on_bad_arguments(ctx):
    sc = loop_scene("wide", 3)
    fn = S.lib().svo_frontend_set_stereo_tracking
    ok = S.StereoRowsParams()

    def fresh(window=True):
        return make_frontend(ctx, [sc], 2, 100, track=None, window=WINDOW if window else 0)

    fe = fresh(window=False)
    assert fn(fe.handle, C_.byref(ok), 4) == -1  # before the stereo window
    assert "no stereo window" in S.lib().svo_last_error(ctx.handle).decode()
    fe.window_enable(WINDOW, stereo=False)
    assert fn(fe.handle, C_.byref(ok), 4) == -1  # a plain window is none either
    fe.close()
    fe = fresh()
    assert fn(None, C_.byref(ok), 4) == -1 and fn(fe.handle, None, 4) == -1
    for guide in (-1, 16):
        assert fn(fe.handle, C_.byref(ok), guide) == -1, guide
    for bad in (dict(radius=0), dict(radius=8), dict(d_min=-17), dict(d_max=256), dict(d_min=0, d_max=1),
                dict(uniq_pct=101), dict(max_cost=-1)):
        assert fn(fe.handle, C_.byref(S.StereoRowsParams(**bad)), 4) == -1, bad
    assert fn(fe.handle, C_.byref(ok), 15) == 0  # the refused calls left it unset
    assert fn(fe.handle, C_.byref(ok), 4) == -1  # twice
    with pytest.raises(S.SvoError):
        fe.set_stereo_tracking()
    fe.close()
    fe = fresh()
    fe.init(0)
    assert fn(fe.handle, C_.byref(ok), 4) == -1  # after init
    assert "before svo_frontend_init" in S.lib().svo_last_error(ctx.handle).decode()
    fe.close()
