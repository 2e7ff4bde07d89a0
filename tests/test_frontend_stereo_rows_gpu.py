"""The batched front end and the host Tracking mirror with row SAD as their stereo
match (svo_frontend_set_stereo_matcher / svo_tracking_set_stereo_matcher) against
the oracle loop with the numpy restatement in findLeftFeaturesInRight's place
(tests/stereo_rows_reference.py), step by step as test_frontend_gpu.py compares."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import svo_amd as S
from stereo_rows_reference import DEFAULTS, RowsOracleLoop, WideScene, WideSceneForward
from svo_amd.scene import Scene
from svo_amd.tracking import Tracking
from test_frontend_gpu import _compare_step

pytestmark = pytest.mark.gpu

KITTI_BASELINE = 0.537  # metres: fx * 0.537 gives the forward scene 9-66 px of disparity


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def make_frontend(ctx, scenes, T, n_features, rows=True, window=0, **kw):
    sc0 = scenes[0]
    P0, P1 = sc0.projections()
    cfg = S.FrontendConfig(sc0.w, sc0.h, sc0.K, n_seq=len(scenes), n_frames=T, n_features=n_features, P_left=P0,
                           P_right=P1, **kw)
    fe = S.Frontend(ctx, cfg)
    if rows:
        fe.set_stereo_matcher(S.StereoRowsParams(**DEFAULTS))
    for s, sc in enumerate(scenes):
        for t in range(T):
            fe.set_frame(s, t, sc.frame(t), sc.right(t))
    if window:
        fe.window_enable(window, stereo=True)
    return fe


def forward(seed):
    sc = WideSceneForward(640, 376, seed=seed)
    sc.bf = float(sc.K[0, 0]) * KITTI_BASELINE
    return sc


def test_frontend_follows_the_restatement_at_kitti_disparities(ctx):
    W, H, N, T = 320, 240, 400, 6
    sc = WideScene(W, H, seed=3)
    fe = make_frontend(ctx, [sc], T, N)
    fe.init(0)
    ref = RowsOracleLoop(WideScene(W, H, seed=3), N).init(0)
    assert len(ref.pts) > 300 and np.array_equal(fe.features(0), ref.pts)
    np.testing.assert_allclose(fe.map_points(0), ref.X, rtol=2e-5, atol=1e-6)
    for t in range(1, T):
        st = fe.step(t).as_dict()
        rs = ref.step(t)
        _compare_step(fe, ref, st, rs, t)
        rv, _ = fe.pose(0)
        assert np.abs(O.rodrigues(rv) - sc.R(t)).max() < 1e-3
    fe.close()


@pytest.mark.parametrize("spec", ["-1", "0", "32"])
def test_frontend_forward_scene_serial_and_fused_keyframes(ctx, spec, monkeypatch):
    """SVO_FE_SPEC_MARGIN -1: always the serial keyframe; 0: the fused one only when
    RANSAC dropped nothing; 32: the default. Two sequences in one batch."""
    monkeypatch.setenv("SVO_FE_SPEC_MARGIN", spec)
    N, T = 800, 6
    seeds = (3, 8)
    fe = make_frontend(ctx, [forward(s) for s in seeds], T, N)
    fe.init(0)
    refs = [RowsOracleLoop(forward(s), N).init(0) for s in seeds]
    serial = 0
    for t in range(1, T):
        st = fe.step(t).as_dict()
        rss = [r.step(t) for r in refs]
        serial += st["serial_keyframe"]
        for k in ("tracked", "lk_iterations", "inliers", "added", "features"):
            assert st[k] == sum(rs[k] for rs in rss), f"{k} differs at t={t}"
        for q, ref in enumerate(refs):
            assert np.array_equal(fe.features(q), ref.pts), f"seq {q} features differ at t={t}"
            rv, tv = fe.pose(q)
            np.testing.assert_allclose(rv, ref.pose[0], atol=1e-7)
            np.testing.assert_allclose(tv, ref.pose[1], atol=1e-6)
            np.testing.assert_allclose(fe.map_points(q), ref.X, rtol=2e-5, atol=1e-6)
    if spec == "-1":
        assert serial == T - 1
    if spec == "32":
        assert serial < T - 1
    fe.close()


def test_frontend_orb_keyframes(ctx):
    N, T = 400, 5
    seeds = (3, 8)
    fe = make_frontend(ctx, [forward(s) for s in seeds], T, N, use_orb=1)
    fe.init(0)
    refs = [RowsOracleLoop(forward(s), N, detector="orb").init(0) for s in seeds]
    for q, ref in enumerate(refs):
        assert len(ref.pts) > 50 and np.array_equal(fe.features(q), ref.pts), f"seq {q} features at init"
    for t in range(1, T):
        st = fe.step(t).as_dict()
        rss = [r.step(t) for r in refs]
        for k in ("tracked", "inliers", "added", "features"):
            assert st[k] == sum(rs[k] for rs in rss), f"{k} at t={t}"
        for q, ref in enumerate(refs):
            assert np.array_equal(fe.features(q), ref.pts), f"seq {q} features at t={t}"
            rv, tv = fe.pose(q)
            np.testing.assert_allclose(rv, ref.pose[0], atol=1e-7)
            np.testing.assert_allclose(tv, ref.pose[1], atol=1e-6)
            np.testing.assert_allclose(fe.map_points(q), ref.X, rtol=2e-5, atol=1e-6)
    fe.close()


def test_stereo_window_keeps_the_matchers_columns(ctx):
    """window_right: per frame of the window, the right column of the match that
    created each feature in that frame (the matcher's xr), -1 for a tracked one."""
    W, H, N, T = 320, 240, 400, 6
    fe = make_frontend(ctx, [WideScene(W, H, seed=3)], T, N, window=4)
    fe.init(0)
    ref = RowsOracleLoop(WideScene(W, H, seed=3), N).init(0)
    seen = []
    for t in range(T):
        if t:
            fe.step(t)
            ref.step(t)
        new = ref.trace["ur"].astype(np.float32)
        seen.append((ref.pts.copy(), np.r_[np.full(len(ref.pts) - len(new), -1.0, np.float32), new]))
        w = fe.window(0)
        frames = list(range(max(0, t - 3), t + 1))
        assert list(w["frame_t"]) == frames
        for j, f in enumerate(frames):
            pts, ur = seen[f]
            assert np.array_equal(w["xy"][j], pts), (t, f)
            assert np.array_equal(w["ur"][j].view(np.uint32), ur.view(np.uint32)), (t, f)
    assert any(np.any(u >= 0) and np.any(u < 0) for _, u in seen[1:])
    fe.close()


def test_a_front_end_without_the_matcher_is_the_front_end(ctx):
    W, H, N, T = 320, 240, 400, 4
    runs = []
    for _ in range(2):
        fe = make_frontend(ctx, [Scene(W, H, seed=3)], T, N, rows=False)
        fe.init(0)
        run = [(fe.features(0).tobytes(), fe.map_points(0).tobytes())]
        for t in range(1, T):
            st = fe.step(t).as_dict()
            run.append((fe.features(0).tobytes(), fe.map_points(0).tobytes(), np.r_[fe.pose(0)].tobytes(),
                        [st[k] for k in ("tracked", "lk_iterations", "inliers", "added", "features")]))
        runs.append(run)
        fe.close()
    assert runs[0] == runs[1]


def test_the_setter_is_refused_late_twice_and_on_bad_parameters(ctx):
    W, H = 320, 240
    sc = Scene(W, H, seed=3)
    fn = S.lib().svo_frontend_set_stereo_matcher
    ok = S.StereoRowsParams()

    def fresh():
        return S.Frontend(ctx, S.FrontendConfig(W, H, sc.K, n_seq=1, n_frames=2, n_features=100))

    fe = fresh()
    assert fn(None, C.byref(ok)) == -1 and fn(fe.handle, None) == -1
    for bad in (dict(radius=0), dict(radius=8), dict(d_min=-17), dict(d_max=256), dict(d_min=0, d_max=1),
                dict(d_min=-16, d_max=240), dict(uniq_pct=101), dict(max_cost=-1)):
        assert fn(fe.handle, C.byref(S.StereoRowsParams(**bad))) == -1, bad
    assert fn(fe.handle, C.byref(ok)) == 0  # the refused calls left it unset
    assert fn(fe.handle, C.byref(ok)) == -1  # twice
    with pytest.raises(S.SvoError):
        fe.set_stereo_matcher()
    fe.close()
    fe = fresh()
    fe.set_frame(0, 0, sc.frame(0), sc.right(0))
    assert fn(fe.handle, C.byref(ok)) == -1  # after the first set_frame
    fe.close()
    fe = fresh()
    for t in range(2):
        fe.set_frame(0, t, sc.frame(t), sc.right(t))
    fe.init(0)
    assert fn(fe.handle, C.byref(ok)) == -1  # after init
    assert "before the first" in S.lib().svo_last_error(ctx.handle).decode()
    fe.close()


def test_tracking_mirror_with_the_matcher_follows_the_restatement():
    """The host Tracking mirror (reference keyframe rule; features_to_track 2^30 makes
    every other frame a keyframe) with the matcher, against the same restatement
    loop: detection, the matcher's output through the trace, the kept pairs, the
    triangulation, the feature lists and the poses, stage by stage."""
    W, H, T = 320, 240, 6
    sc = WideScene(W, H, seed=3)
    P0, P1 = sc.projections()
    tr = Tracking(np.r_[P0.ravel(), P1.ravel()], features_to_track=1 << 30)
    tr.set_stereo_matcher(S.StereoRowsParams(**DEFAULTS))
    with pytest.raises(S.SvoError):
        tr.set_stereo_matcher()  # twice
    ref = RowsOracleLoop(WideScene(W, H, seed=3), 1 << 14, acc=O.ACC_SSE, rule="reference",
                         features_to_track=1 << 30)
    n_kf = 0
    for t in range(T):
        L, R = sc.frame(t), sc.right(t)
        tr.push(L, R)
        assert tr.step()
        if t == 0:
            with pytest.raises(S.SvoError):
                tr.set_stereo_matcher()  # after the first step
            ref.init(0)
            rs = {"keyframe": 1}
        else:
            prev = ref.pts.copy()
            rs = ref.step(t)
            assert np.array_equal(tr.trace("lk_prev"), prev)
            assert int(tr.trace("lk_status").sum()) == rs["tracked"]
            assert len(tr.trace("pnp_inliers")) == rs["inliers"]
            pp = tr.trace("pnp_pose")
            np.testing.assert_allclose(pp[:3], ref.pose[0], atol=1e-7)
            np.testing.assert_allclose(pp[3:6], ref.pose[1], atol=1e-6)
        info = tr.frame_info()
        assert bool(info["keyframe"]) == bool(rs["keyframe"])
        if rs["keyframe"]:
            n_kf += 1
            kps, sr, ss = tr.trace("kps"), tr.trace("stereo_right"), tr.trace("stereo_status")
            assert len(kps) == len(ref.trace["status"]) > 0
            assert np.array_equal(ss, ref.trace["status"])
            assert np.array_equal(sr.view(np.uint32), ref.trace["right"].view(np.uint32))
            kept = (ss == 1) & (np.abs(sr[:, 1] - kps[:, 1]) < 40)
            assert np.array_equal(tr.trace("kept_left"), kps[kept]) and np.array_equal(tr.trace("kept_right"), sr[kept])
            _, ox = O.triangulate(P0, P1, kps[kept], sr[kept])
            assert np.allclose(tr.trace("tri_xyz"), ox, rtol=1e-5, atol=1e-5)
        xy, world, _ = tr.features()
        assert np.array_equal(xy, ref.pts), t
        np.testing.assert_allclose(world, ref.X, rtol=2e-5, atol=1e-6)
    assert n_kf == 3
    tr.close()
