"""Raw camera frames through the batched front end (svo_frontend_set_rectification):
front end A has the rig's maps and is fed raw 352x264 frames, front end B has none
and is fed the same frames rectified by the numpy restatement of cv::remap. The two
must run the same loop -- feature lists, poses, map points and counts identical for
every sequence after init and after every step -- and sequence 0 must be the oracle
loop's on B's frames. Resident (set_frame) and streamed (queue_frames from
page-locked memory into a ring of 4), grey and BGR.

The oracle's run carries the health condition (tracked >= 0.9 x the previous
step's features at every step), so a dead loop cannot pass vacuously. The grey
seed-5 scene gives init 299 and tracked 299, 295, 297, 285, 293, 295, 295 of at
most 300 (worst ratio 0.956); the left map reaches columns 23..328 and rows
16..249 of the 352x264 raw frame."""
import ctypes as C
import functools

import numpy as np
import pytest

import rectify_reference as RR
import svo_amd as S
from oracle_loop import OracleLoop
from svo_amd.scene import Scene, stereo_projections

pytestmark = pytest.mark.gpu

RAW_W, RAW_H, W, H = 352, 264, 320, 240
NS, N, T = 3, 300, 10  # steps 1 .. 7; the streamed loop queues frame t + 2 before step t
DIST_L, RVEC_L = (-0.08, 0.02, 5e-4, -3e-4, 0, 0, 0, 0), (0.004, -0.003, 0.002)
DIST_R, RVEC_R = (-0.075, 0.018, -4e-4, 2e-4, 0, 0, 0, 0), (0.004, 0.003, 0.002)


class _Rig:
    """What OracleLoop reads of a scene: the rectified rig's K and projections."""

    def __init__(self, K):
        self.K = K

    def projections(self):
        return stereo_projections(self.K)


@functools.lru_cache(maxsize=None)
def _rig():
    K = Scene(RAW_W, RAW_H, seed=5).K  # the raw cameras' matrix
    newK = K.copy()
    newK[0, 2] -= 16
    newK[1, 2] -= 12
    maps_l = RR.init_maps(K, DIST_L, RR.rodrigues(*RVEC_L), newK, W, H)
    maps_r = RR.init_maps(K, DIST_R, RR.rodrigues(*RVEC_R), newK, W, H)
    Kf = newK.astype(np.float32).astype(np.float64)  # the front end's K, float32-rounded as intrinsics()
    return K, newK, Kf, maps_l, maps_r


@functools.lru_cache(maxsize=None)
def _frames(bgr):
    """-> raw [side][t][s] (grey or BGR), rectified grey [side][t][s] by numpy."""
    _, _, _, maps_l, maps_r = _rig()
    scenes = [Scene(RAW_W, RAW_H, seed=5 + s) for s in range(NS)]
    raw = [[[None] * NS for _ in range(T)] for _ in range(2)]
    rect = [[[None] * NS for _ in range(T)] for _ in range(2)]
    for t in range(T):
        for s, sc in enumerate(scenes):
            for side, (g, maps) in enumerate(((sc.frame(t), maps_l), (sc.right(t), maps_r))):
                px = RR.bgr_of(g, 1000 * t + 10 * s + side) if bgr else np.ascontiguousarray(g)
                raw[side][t][s] = px
                rect[side][t][s] = RR.remap(RR.gray_of(px) if bgr else px, *maps)
    return raw, rect


@functools.lru_cache(maxsize=None)
def _oracle(bgr):
    """The oracle loop of sequence 0 on the numpy-rectified frames: the feature list
    after init and after every step, with the health condition."""
    _, rect = _frames(bgr)
    _, _, Kf, _, _ = _rig()
    ref = OracleLoop(_Rig(Kf), N).init(0, rect[0][0][0], rect[1][0][0])
    pts = [ref.pts.copy()]
    assert len(ref.pts) > 0.9 * N
    for t in range(1, T - 2):
        n_prev = len(ref.pts)
        st = ref.step(t, rect[0][t][0], rect[1][t][0])
        print(f"oracle bgr={bgr} t={t}: tracked {st['tracked']} of {n_prev}, inliers {st['inliers']}")
        assert st["tracked"] >= 0.9 * n_prev, f"oracle loop unhealthy at t={t}: {st['tracked']} of {n_prev}"
        pts.append(ref.pts.copy())
    return pts


def _config(n_frames):
    _, _, Kf, _, _ = _rig()
    return S.FrontendConfig(W, H, Kf, n_seq=NS, n_frames=n_frames, n_features=N)


def _maps(ctx):
    _, _, _, maps_l, maps_r = _rig()
    return S.RectMaps(ctx, RAW_W, RAW_H, *maps_l), S.RectMaps(ctx, RAW_W, RAW_H, *maps_r)


def _same_state(a, b, ref_pts, where):
    for s in range(NS):
        assert np.array_equal(a.features(s), b.features(s)), f"features, seq {s} {where}"
        assert np.array_equal(np.r_[a.pose(s)], np.r_[b.pose(s)]), f"pose, seq {s} {where}"
        assert np.array_equal(a.map_points(s), b.map_points(s)), f"map points, seq {s} {where}"
    assert np.array_equal(a.features(0), ref_pts), f"oracle {where}"


def _same_counts(sa, sb, where):
    sa, sb = sa.as_dict(), sb.as_dict()
    for k in ("tracked", "inliers", "added", "features", "lk_iterations", "keyframes"):
        assert sa[k] == sb[k], f"{k} {where}"
    assert sa["tracked"] > 0


def _resident_b(ctx, rect):
    """Front end B: no rectification, every numpy-rectified frame resident."""
    b = S.Frontend(ctx, _config(T))
    for t in range(T):
        for s in range(NS):
            b.set_frame(s, t, rect[0][t][s], rect[1][t][s])
    b.init(0)
    return b


@pytest.mark.parametrize("bgr", [False, True])
def test_resident_raw_frames_match_rectified_frames(bgr):
    ctx = S.Context(0)
    raw, rect = _frames(bgr)
    ref = _oracle(bgr)
    ml, mr = _maps(ctx)
    a = S.Frontend(ctx, _config(T))
    a.set_rectification(ml, mr)
    for t in range(T):
        for s in range(NS):
            a.set_frame(s, t, raw[0][t][s], raw[1][t][s])
    a.init(0)
    b = _resident_b(ctx, rect)
    _same_state(a, b, ref[0], "after init")
    for t in range(1, T - 2):
        _same_counts(a.step(t), b.step(t), f"at t={t}")
        _same_state(a, b, ref[t], f"at t={t}")
    for o in (a, b, ml, mr, ctx):
        o.close()


@pytest.mark.parametrize("bgr", [False, True])
def test_streamed_raw_frames_match_rectified_frames(bgr):
    ctx = S.Context(0)
    raw, rect = _frames(bgr)
    ref = _oracle(bgr)
    ml, mr = _maps(ctx)
    # the raw frames in one page-locked block per eye, [t][s]: consecutive sequences
    # follow each other in memory, one H2D copy per eye and step
    shape = (T, NS, RAW_H, RAW_W, 3) if bgr else (T, NS, RAW_H, RAW_W)
    pl, pr = S.PinnedBuffer(shape), S.PinnedBuffer(shape)
    for t in range(T):
        for s in range(NS):
            pl.array[t, s] = raw[0][t][s]
            pr.array[t, s] = raw[1][t][s]
    a = S.Frontend(ctx, _config(4))
    a.set_rectification(ml, mr)
    for t in range(3):
        a.queue_frames(t, list(pl.array[t]), list(pr.array[t]))
    a.init(0)
    b = _resident_b(ctx, rect)
    _same_state(a, b, ref[0], "after init")
    for t in range(1, T - 2):
        a.queue_frames(t + 2, list(pl.array[t + 2]), list(pr.array[t + 2]))
        _same_counts(a.step(t), b.step(t), f"at t={t}")
        _same_state(a, b, ref[t], f"at t={t}")
    a.upload_wait(T - 1)
    with pytest.raises(S.SvoError):  # frames of the config's size are no raw frames
        a.queue_frames(T, [rect[0][0][s] for s in range(NS)], [rect[1][0][s] for s in range(NS)])
    for o in (a, b, ml, mr):
        o.close()
    pl.close()
    pr.close()
    ctx.close()


def test_set_rectification_rejections():
    ctx = S.Context(0)
    raw, rect = _frames(False)
    ml, mr = _maps(ctx)
    cfg1 = S.FrontendConfig(W, H, _rig()[2], n_seq=1, n_frames=4, n_features=N)
    # after set_frame, after queue_frames, after init
    fe = S.Frontend(ctx, cfg1)
    fe.set_frame(0, 0, rect[0][0][0], rect[1][0][0])
    with pytest.raises(S.SvoError):
        fe.set_rectification(ml, mr)
    fe.close()
    fe = S.Frontend(ctx, cfg1)
    fe.queue_frames(0, [rect[0][0][0]], [rect[1][0][0]])
    with pytest.raises(S.SvoError):
        fe.set_rectification(ml, mr)
    fe.upload_wait(0)
    fe.close()
    fe = S.Frontend(ctx, cfg1)
    for t in range(2):
        fe.set_frame(0, t, rect[0][t][0], rect[1][t][0])
    fe.init(0)
    with pytest.raises(S.SvoError):
        fe.set_rectification(ml, mr)
    fe.close()
    # maps of another output size; eyes of different raw sizes; null maps; a second call
    fe = S.Frontend(ctx, cfg1)
    m1 = np.zeros((H, W + 1, 2), np.int16)
    wide = S.RectMaps(ctx, RAW_W, RAW_H, m1, np.zeros((H, W + 1), np.uint16))
    other_raw = S.RectMaps(ctx, RAW_W + 1, RAW_H, *_rig()[3])
    with pytest.raises(S.SvoError):
        fe.set_rectification(wide, mr)
    with pytest.raises(S.SvoError):
        fe.set_rectification(ml, wide)
    with pytest.raises(S.SvoError):
        fe.set_rectification(ml, other_raw)
    assert S.lib().svo_frontend_set_rectification(fe.handle, ml.handle, None) == -1
    fe.set_rectification(ml, mr)  # the refused calls left it unset
    with pytest.raises(S.SvoError):
        fe.set_rectification(ml, mr)
    # set_frame: a stride below the raw row; the wrapper refuses frames of the config's size
    u8p = C.POINTER(C.c_uint8)
    L, R = raw[0][0][0], raw[1][0][0]
    assert S.lib().svo_frontend_set_frame(fe.handle, 0, 0, L.ctypes.data_as(u8p), R.ctypes.data_as(u8p),
                                          RAW_W - 1) == -1
    assert S.lib().svo_frontend_set_frame(fe.handle, 0, 0, L.ctypes.data_as(u8p), R.ctypes.data_as(u8p), W) == -1
    with pytest.raises(S.SvoError):
        fe.set_frame(0, 0, rect[0][0][0], rect[1][0][0])
    fe.set_frame(0, 0, L, R)
    for o in (fe, wide, other_raw, ml, mr, ctx):
        o.close()
