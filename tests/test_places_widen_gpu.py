"""svo_frontend_places_widen on the dropped-frame sequences
of tests/starved_cases.py, 320x240: after the bounded query of frame 4 the widened
pairs, counts, inliers and pose of every sequence against the restatement
(tests/match_projected_reference.py) run on the front end's own records, lists and
frame; the `which` mask, a frame_t of -1 and one that has left a ring of two
slots; the thin sequence; a front end left bit for bit as one that never made the
call; and the error returns."""
import ctypes

import numpy as np
import pytest

import match_projected_cases as MC
import match_projected_reference as MP
import places_cases as P
import starved_cases as C
import svo_amd as S
from test_places_gpu import BATCH, K, _follow, _resident, _want_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture
def made():
    fes = []
    yield fes
    for fe in fes:
        fe.close()


def _want_widen(fe, rec, cur, rvec, tvec, **prm):
    """The restatement on a record and the query set, under the pose the query gave."""
    cfg = fe.cfg
    return MP.widen(rec["xyz"], rec["desc"], cur["xy"], cur["desc"], rvec, tvec, K, (C.W, C.H),
                    **{**MP.DEFAULTS, **prm}, iterations=cfg.pnp_iterations, reproj=cfg.pnp_reproj,
                    confidence=cfg.pnp_confidence)


def _same_widen(got, s, want):
    assert got["n_pairs"][s] == len(want["pairs"]), (got["n_pairs"][s], len(want["pairs"]))
    assert np.array_equal(got["pairs"][s], want["pairs"])
    assert got["ok"][s] == int(want["ok"])
    assert got["n_inliers"][s] == len(want["inliers"]) and np.array_equal(got["inliers"][s], want["inliers"])
    np.testing.assert_allclose(got["rvec"][s], want["rvec"], atol=1e-7)
    np.testing.assert_allclose(got["tvec"][s], want["tvec"], atol=1e-6)


def _untouched(got, s):
    assert got["n_pairs"][s] == 0 and got["n_inliers"][s] == 0 and got["ok"][s] == 0
    assert not got["rvec"][s].any() and not got["tvec"][s].any()
    assert len(got["pairs"][s]) == 0 and len(got["inliers"][s]) == 0


def test_widen_after_the_bounded_query(ctx, made):
    """DROPPED_300 beside its healthy twin, one launch chain for both."""
    fe = _resident(ctx, made, BATCH)
    fe.places_enable(8, 1, 31)
    wants = _follow(fe, BATCH, P.REBUILD_T, 8)
    res = fe.places_query(*P.BOUND)
    assert res["frame_t"][0] == P.PICKED["n300"]["frame"] and res["frame_t"][1] >= 0
    got = fe.places_widen(res)
    for s in range(2):
        want = _want_widen(fe, wants[res["frame_t"][s]][s], wants[P.REBUILD_T][s], res["rvec"][s], res["tvec"][s])
        _same_widen(got, s, want)
        assert want["ok"] and len(want["pairs"]) >= 100
        print(f"seq {s}: query {res['n_pairs'][s]} pairs / {res['n_inliers'][s]} inliers -> widened "
              f"{got['n_pairs'][s]} / {got['n_inliers'][s]}")
    m = MC.MEASURED["n300"]  # the dropped sequence's lists are the oracle loop's
    assert (res["n_pairs"][0], res["n_inliers"][0]) == m["first"]
    assert (got["n_pairs"][0], got["n_inliers"][0]) == m["widened"]
    import orb_describe_cases as ODC
    rot, trans = ODC.pose_error(C.scene(C.DROPPED_300), P.REBUILD_T, got["rvec"][0], got["tvec"][0])
    assert rot <= 2 * m["rot_deg"] and trans <= 2 * m["trans_m"]
    # other parameters
    for prm in (dict(radius=12.0, max_dist=40, ratio_pct=70), dict(radius=1.5, max_dist=256, ratio_pct=0)):
        g = fe.places_widen(res, S.ProjMatchParams(**prm))
        for s in range(2):
            _same_widen(g, s, _want_widen(fe, wants[res["frame_t"][s]][s], wants[P.REBUILD_T][s], res["rvec"][s],
                                          res["tvec"][s], **prm))
    # a mask, and a sequence without a result
    g = fe.places_widen(res, which=[0, 1])
    _untouched(g, 0)
    assert np.array_equal(g["pairs"][1], got["pairs"][1]) and np.array_equal(g["inliers"][1], got["inliers"][1])
    none = dict(res, frame_t=np.array([-1, res["frame_t"][1]], np.int32))
    g = fe.places_widen(none)
    _untouched(g, 0)
    assert np.array_equal(g["pairs"][1], got["pairs"][1]) and g["ok"][1] == 1
    # a frame no record holds
    gone = dict(res, frame_t=np.array([7, 3], np.int32))  # (frame 3 of the healthy sequence is there)
    g = fe.places_widen(gone)
    _untouched(g, 0)
    assert g["n_pairs"][1] == len(_want_widen(fe, wants[3][1], wants[P.REBUILD_T][1], res["rvec"][1],
                                               res["tvec"][1])["pairs"])
    # the widening left the records and the loop alone
    fe.step(5)
    tr = C.oracle_trace(C.DROPPED_300)
    assert np.array_equal(fe.features(0), tr[5].pts)


def test_a_frame_that_left_a_ring_of_two_slots(ctx, made):
    fe = _resident(ctx, made, BATCH)
    fe.places_enable(2, 1, 31)
    fe.init(0)
    for t in range(1, P.REBUILD_T + 1):
        fe.step(t)
    cur = [_want_record(fe, c, s, P.REBUILD_T) for s, c in enumerate(BATCH)]
    assert [fe.place(0, k)["frame_t"] for k in range(2)] == [4, 3]
    res = fe.places_query()  # the frame's own record: every feature matches itself
    assert res["frame_t"].tolist() == [4, 4]
    got = fe.places_widen(res)
    for s in range(2):
        _same_widen(got, s, _want_widen(fe, cur[s], cur[s], res["rvec"][s], res["tvec"][s]))
        assert got["n_pairs"][s] >= len(cur[s]["desc"]) // 2
    old = dict(res, frame_t=np.array([1, 4], np.int32))  # frame 1 was overwritten by frame 3
    g = fe.places_widen(old)
    _untouched(g, 0)
    assert np.array_equal(g["pairs"][1], got["pairs"][1])


def test_thin_sequence_and_an_unchanged_front_end(ctx, made):
    """DROPPED_64: 14 widened pairs. Features, poses and map points before and after
    the call, and over the rest of the run against a front end that never made it."""
    case = C.DROPPED_64

    def state(fe):
        return fe.features(0), np.r_[fe.pose(0)], fe.map_points(0)

    runs = []
    for call in (True, False):
        fe = _resident(ctx, made, [case])
        fe.places_enable(8, 1, 31)
        seen = []
        if call:
            wants = _follow(fe, [case], P.REBUILD_T, 8)
        else:
            fe.init(0)
            for t in range(1, P.REBUILD_T + 1):
                fe.step(t)
        seen.append(state(fe))
        if call:
            res = fe.places_query(*P.BOUND)
            got = fe.places_widen(res)
            after = state(fe)
            for x, y in zip(seen[0], after):
                assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
            want = _want_widen(fe, wants[res["frame_t"][0]][0], wants[P.REBUILD_T][0], res["rvec"][0], res["tvec"][0])
            _same_widen(got, 0, want)
            m = MC.MEASURED["n64"]
            assert (res["n_pairs"][0], res["n_inliers"][0]) == m["first"]
            assert (got["n_pairs"][0], got["n_inliers"][0]) == m["widened"] and got["ok"][0] == 1
            print(f"thin: query {res['n_pairs'][0]} / {res['n_inliers'][0]} -> widened {got['n_pairs'][0]} / "
                  f"{got['n_inliers'][0]}")
            # a window too small for any candidate: fewer than 4 pairs, no model
            g = fe.places_widen(res, S.ProjMatchParams(radius=1e-3, max_dist=0))
            assert g["ok"][0] == 0 and g["n_pairs"][0] < 4 and g["n_inliers"][0] == 0 and not g["rvec"][0].any()
        for t in range(P.REBUILD_T + 1, case.frames):
            fe.step(t)
            seen.append(state(fe))
        runs.append(seen)
        fe.close()
    for k, (a, b) in enumerate(zip(*runs)):
        for x, y, what in zip(a, b, ("features", "pose", "map points")):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}, frame {4 + k}"


def test_error_returns(ctx, made):
    case = C.DROPPED_64
    fe = _resident(ctx, made, [case])
    res = dict(frame_t=np.zeros(1, np.int32), rvec=np.zeros((1, 3)), tvec=np.zeros((1, 3)))
    with pytest.raises(S.SvoError):  # before enabling
        fe.places_widen(res)
    fe.places_enable(4, 1, 31)
    with pytest.raises(S.SvoError):  # before init
        fe.places_widen(res)
    fe.init(0)
    for bad in [dict(radius=0), dict(radius=float("nan")), dict(radius=float("inf")), dict(max_dist=-1),
                dict(max_dist=257), dict(ratio_pct=-1)]:
        with pytest.raises(S.SvoError):
            fe.places_widen(res, S.ProjMatchParams(**bad))
    with pytest.raises(S.SvoError):
        fe.places_widen(res, which=[1, 0])
    lib = S.lib()
    prm = S.ProjMatchParams()
    i, d = np.full(1, -9, np.int32), np.full(3, -9.0)
    ip, dp = i.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    pp = ctypes.addressof(prm)
    good = [fe.handle, None, ip, dp, dp, pp, ip, ip, ip, dp, dp, None, None, 0]
    for k in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10):  # each required argument null in turn
        a = list(good)
        a[k] = None
        assert lib.svo_frontend_places_widen(*a) == -1, k
    assert lib.svo_frontend_places_widen(*good[:-1], -1) == -1
    assert np.all(i == -9) and np.all(d == -9)  # nothing written
    # the init frame against its own record, under the identity: every entry pairs with itself
    got = fe.places_widen(res)
    rec = fe.place(0, 0)
    assert got["ok"][0] == 1 and len(rec["desc"]) - 2 <= got["n_pairs"][0] <= len(rec["desc"])
    assert np.array_equal(got["pairs"][0][:, 0], got["pairs"][0][:, 1])
