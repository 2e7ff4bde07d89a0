"""The batched front end's place memory (svo_frontend_places_*; DESIGN.md section
3e) on the dropped-frame sequences of tests/starved_cases.py, 320x240: every
record against the restatement (tests/places_reference.py) run on the front end's
own lists and frame, the query against the restatement's query and the oracle's
RANSAC, a front end with the memory enabled against one without, the streamed
ring against the resident run, and the error returns."""
import ctypes

import numpy as np
import pytest

import orb_describe_cases as ODC
import places_cases as P
import places_reference as PR
import starved_cases as C
import svo_amd as S
from test_frontend_gpu import _compare_step

pytestmark = pytest.mark.gpu

K = P.SCENE_K
HEALTHY_300 = C.DROPPED_300._replace(drops=())
BATCH = [C.DROPPED_300, HEALTHY_300]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture
def made():
    """Front ends closed when the test ends, passed or failed."""
    fes = []
    yield fes
    for fe in fes:
        fe.close()


def _resident(ctx, made, cases, n_frames=None, **kw):
    T, n = cases[0].frames, cases[0].n
    fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, K, n_seq=len(cases), n_frames=n_frames or T, n_features=n, **kw))
    made.append(fe)
    if n_frames is None:
        for s, c in enumerate(cases):
            for t, (L, R) in enumerate(C.frames(c)):
                fe.set_frame(s, t, L, R)
    return fe


def _want_record(fe, case, seq, t, patch_size=31):
    """The restatement on what the front end holds after frame t: its list, its map
    points (final: map_points synchronises) and the frame."""
    return PR.record(C.frames(case)[t][0], fe.features(seq), fe.map_points(seq), patch_size)


def _same_record(got, want, frame_t, what):
    assert got["frame_t"] == frame_t, what
    assert got["desc"].shape == want["desc"].shape, (what, got["desc"].shape, want["desc"].shape)
    assert np.array_equal(got["desc"], want["desc"]), f"{what}: descriptors"
    assert np.array_equal(got["xy"].view(np.uint32), want["xy"].view(np.uint32)), f"{what}: pixels"
    assert np.array_equal(got["xyz"].view(np.uint64), want["xyz"].view(np.uint64)), f"{what}: map points"


def _follow(fe, cases, upto, slots, every=1, patch_size=31):
    """init and the steps 1 .. upto; after each recorded frame the newest record of
    every sequence against the restatement, and every older slot against what it
    held. Returns {frame: [record per sequence]} of every recorded frame."""
    wants, held = {}, {}
    for t in range(upto + 1):
        if t == 0:
            fe.init(0)
        else:
            fe.step(t)
        if t % every:
            continue
        slot = (t // every) % slots
        wants[t] = [_want_record(fe, c, s, t, patch_size) for s, c in enumerate(cases)]
        held[slot] = t
        for k in range(slots):
            for s in range(len(cases)):
                got = fe.place(s, k)
                if k in held:
                    _same_record(got, wants[held[k]][s], held[k], f"t={t} seq {s} slot {k} (frame {held[k]})")
                else:
                    assert got["frame_t"] == -1 and len(got["desc"]) == 0
    return wants


# ---------------------------------------------------------------- records
@pytest.mark.parametrize("slots,every,patch_size", [(8, 1, 31), (2, 1, 31), (8, 3, 31), (8, 1, 15)],
                         ids=["8slots", "2slots-wrap", "every3", "patch15"])
def test_records_match_the_restatement(ctx, made, slots, every, patch_size):
    """All 9 frames of a dropped and a healthy sequence in one batch. The blank frames
    3 and 6 leave empty records in the dropped sequence; with 8 slots frame 8
    overwrites slot 0, with 2 the ring wraps every second frame."""
    fe = _resident(ctx, made, BATCH)
    fe.places_enable(slots, every, patch_size)
    wants = _follow(fe, BATCH, 8, slots, every, patch_size)
    assert sorted(wants) == list(range(0, 9, every))
    for t in (3, 6):
        if t in wants:
            assert len(wants[t][0]["desc"]) == 0 and len(wants[t][1]["desc"]) > 100
    sizes = [len(wants[t][0]["desc"]) for t in sorted(wants)]
    print("record sizes of the dropped sequence:", sizes)
    if patch_size == 31:  # the oracle loop's lists give the same records (features are bit-equal)
        assert sizes == [P.RECORD_SIZES["n300"][t] for t in sorted(wants)]
    else:
        assert all(a >= b for a, b in zip(sizes, P.RECORD_SIZES["n300"]))  # a narrower border keeps more
    if slots == 8 and every == 1:
        assert fe.place(0, 0)["frame_t"] == 8 and fe.place(0, 1)["frame_t"] == 1


# ---------------------------------------------------------------- query
@pytest.fixture
def at_frame_4(ctx, made):
    fe = _resident(ctx, made, BATCH)
    fe.places_enable(8, 1, 31)
    return fe, _follow(fe, BATCH, P.REBUILD_T, 8)


def _want_query(wants, seq, t_lo, t_hi, **kw):
    t = max(wants)
    q = wants[t][seq]
    # (the record of the queried frame is in the ring too: the query searches it when the bound lets it)
    recs = {f: w[seq] for f, w in wants.items()}
    return PR.query(dict(desc=q["desc"], xy=q["xy"]), recs, t_lo, t_hi, K, **kw)


def _same_query(res, s, want, slot_of):
    assert res["frame_t"][s] == want["frame_t"]
    assert res["n_pairs"][s] == want["n_pairs"]
    for f, k in slot_of.items():
        assert res["slot_pairs"][s, k] == want["counts"].get(f, -1), (f, k)
    assert res["ok"][s] == int(want["ok"])
    assert np.array_equal(res["pairs"][s], want["pairs"])
    assert np.array_equal(res["inliers"][s], want["inliers"])
    assert res["n_inliers"][s] == len(want["inliers"])
    np.testing.assert_allclose(res["rvec"][s], want["rvec"], atol=1e-7)
    np.testing.assert_allclose(res["tvec"][s], want["tvec"], atol=1e-6)


def test_bounded_query_recovers_the_old_world(ctx, at_frame_4):
    fe, wants = at_frame_4
    slot_of = {f: f for f in range(5)}
    res = fe.places_query(*P.BOUND)
    assert np.all(res["slot_pairs"][:, 5:] == -1)
    for s in range(2):
        want = _want_query(wants, s, *P.BOUND)
        _same_query(res, s, want, slot_of)
        assert want["ok"] and len(want["pairs"]) >= 100
    # the dropped sequence: frame 1, 172 pairs (the tie with frame 2 to the older), the old world's pose
    pick = P.PICKED["n300"]
    assert res["frame_t"][0] == pick["frame"] and res["n_pairs"][0] == pick["pairs"]
    assert res["slot_pairs"][0, 1] == res["slot_pairs"][0, 2]
    rot, trans = ODC.pose_error(C.scene(C.DROPPED_300), P.REBUILD_T, res["rvec"][0], res["tvec"][0])
    print(f"bounded query of frame 4: frame {res['frame_t'][0]}, {res['n_pairs'][0]} pairs, "
          f"{res['n_inliers'][0]} inliers, rot {rot:.4f} deg, |t| {trans:.4f} m")
    assert rot <= 2 * pick["rot_deg"] and trans <= 2 * pick["trans_m"]
    # without a bound the frame's own record wins (every feature matches itself)
    free = fe.places_query()
    for s in range(2):
        _same_query(free, s, _want_query(wants, s, 0, 1 << 30), slot_of)
        assert free["frame_t"][s] == P.REBUILD_T
    # no cross-check, another ratio
    loose = fe.places_query(*P.BOUND, ratio_pct=95, cross_check=False)
    for s in range(2):
        _same_query(loose, s, _want_query(wants, s, *P.BOUND, ratio_pct=95, cross_check=False), slot_of)


def test_query_mask_and_no_result(ctx, at_frame_4):
    fe, wants = at_frame_4
    slot_of = {f: f for f in range(5)}
    full = fe.places_query(*P.BOUND)
    # a mask that leaves sequence 1 out: its outputs stay as initialised
    out = {k: np.full_like(v, -5) for k, v in full.items() if isinstance(v, np.ndarray)}
    res = fe.places_query(*P.BOUND, which=[1, 0], out=out)
    _same_query(res, 0, _want_query(wants, 0, *P.BOUND), slot_of)
    for k in ("frame_t", "n_pairs", "n_inliers", "ok", "rvec", "tvec", "slot_pairs"):
        assert np.all(res[k][1] == -5), k
    # a bound that selects only the empty record of the blank frame 3
    res = fe.places_query(3, 3)
    assert res["frame_t"][0] == -1 and res["ok"][0] == 0 and res["n_pairs"][0] == 0 and res["n_inliers"][0] == 0
    assert res["slot_pairs"][0].tolist() == [-1, -1, -1, 0, -1, -1, -1, -1]
    assert not res["rvec"][0].any() and not res["tvec"][0].any() and len(res["pairs"][0]) == 0
    _same_query(res, 1, _want_query(wants, 1, 3, 3), slot_of)  # the healthy sequence has a record there
    assert res["frame_t"][1] == 3
    # a bound no record lies in
    res = fe.places_query(10, 20)
    assert np.all(res["frame_t"] == -1) and np.all(res["slot_pairs"] == -1) and not res["ok"].any()
    # min_pairs above the best count
    best = int(full["n_pairs"][0])
    res = fe.places_query(*P.BOUND, which=[1, 0], min_pairs=best + 1)
    assert res["frame_t"][0] == -1 and res["n_pairs"][0] == best and res["ok"][0] == 0
    assert fe.places_query(*P.BOUND, which=[1, 0], min_pairs=best)["frame_t"][0] == 1
    # the queries left the records and the loop alone
    fe.step(5)
    _same_record(fe.place(0, 5), _want_record(fe, C.DROPPED_300, 0, 5), 5, "frame 5 after the queries")
    tr = C.oracle_trace(C.DROPPED_300)
    assert np.array_equal(fe.features(0), tr[5].pts)


def test_thin_sequence_query(ctx, made):
    """DROPPED_64: 24 .. 38 entries per record, 14-15 pairs, a record of 5 entries
    (frame 3) and, later, of none."""
    case = C.DROPPED_64
    fe = _resident(ctx, made, [case])
    fe.places_enable(8, 1, 31)
    wants = _follow(fe, [case], P.REBUILD_T, 8)
    assert [len(wants[t][0]["desc"]) for t in range(5)] == P.RECORD_SIZES["n64"][:5]
    slot_of = {f: f for f in range(5)}
    res = fe.places_query(*P.BOUND)
    _same_query(res, 0, _want_query(wants, 0, *P.BOUND), slot_of)
    pick = P.PICKED["n64"]
    assert res["frame_t"][0] == pick["frame"] and res["n_pairs"][0] == pick["pairs"] and res["ok"][0] == 1
    rot, trans = ODC.pose_error(C.scene(case), P.REBUILD_T, res["rvec"][0], res["tvec"][0])
    print(f"thin query of frame 4: {res['n_pairs'][0]} pairs, {res['n_inliers'][0]} inliers, rot {rot:.4f} deg, "
          f"|t| {trans:.4f} m")
    assert rot <= 2 * pick["rot_deg"] and trans <= 2 * pick["trans_m"]
    res = fe.places_query(3, 3)  # the 5-entry record
    _same_query(res, 0, _want_query(wants, 0, 3, 3), slot_of)


# ---------------------------------------------------------------- unchanged front end
def test_front_end_is_unchanged_by_the_memory(ctx, made):
    case = C.DROPPED_64
    runs = []
    for on in (False, True):
        fe = _resident(ctx, made, [case])
        if on:
            fe.places_enable(2, 1, 31)
        fe.init(0)
        seen = [(fe.features(0), np.r_[fe.pose(0)], fe.map_points(0))]
        for t in range(1, case.frames):
            fe.step(t)
            seen.append((fe.features(0), np.r_[fe.pose(0)], fe.map_points(0)))
        runs.append(seen)
        fe.close()
    for t, (a, b) in enumerate(zip(*runs)):
        for x, y, what in zip(a, b, ("features", "pose", "map points")):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what} at t={t}"


# ---------------------------------------------------------------- streamed
def test_streamed_records_equal_the_resident_run(ctx, made):
    """STREAMED (25 frames, every third dropped) through a ring of 4 image slots,
    frame t + 2 queued before step t and no synchronisation between the steps: the
    records' points are copied behind each next step's post-LK, and the uploads
    wait for the describe pass that reads their slot. Every record equals the
    resident run's record of the same frame."""
    case = C.STREAMED
    T, slots = case.frames, 16
    fr = C.frames(case)
    res = _resident(ctx, made, [case])
    res.places_enable(slots, 1, 31)
    wants = _follow(res, [case], T - 1, slots)
    res.close()
    fe = _resident(ctx, made, [case], n_frames=4)
    fe.places_enable(slots, 1, 31)
    for t in range(3):
        fe.queue_frames(t, [fr[t][0]], [fr[t][1]])
    fe.init(0)

    def check(upto):
        for f in range(max(0, upto - slots + 1), upto + 1):
            _same_record(fe.place(0, f % slots), wants[f][0], f, f"streamed frame {f}")

    for t in range(1, T):
        if t + 2 < T:
            fe.queue_frames(t + 2, [fr[t + 2][0]], [fr[t + 2][1]])
        st = fe.step(t).as_dict()
        if t == 12:
            check(12)  # frames 0 .. 12, before the ring wraps
    check(T - 1)
    tr = C.oracle_trace(case)
    _compare_step(fe, tr[T - 1], st, tr[T - 1].stats, T - 1)
    fe.upload_wait(T - 1)
    assert sum(len(wants[f][0]["desc"]) == 0 for f in wants) >= 4  # the dropped frames' empty records


# ---------------------------------------------------------------- errors
def test_error_returns(ctx, made):
    case = C.DROPPED_64
    fe = _resident(ctx, made, [case])
    with pytest.raises(S.SvoError):  # before enabling
        fe.places_query()
    with pytest.raises(S.SvoError):
        fe.place(0, 0)
    for slots, every, patch in [(0, 1, 31), (S.PLACES_MAX_SLOTS + 1, 1, 31), (4, 0, 31), (4, 1, 30), (4, 1, 3),
                                (4, 1, 33)]:
        with pytest.raises(S.SvoError):
            fe.places_enable(slots, every, patch)
    with pytest.raises(S.SvoError):  # a pattern entry outside [-hp, hp]
        fe.places_enable(4, 1, 15, np.full((512, 2), 8, np.int8))
    fe.places_enable(4, 1, 31)
    with pytest.raises(S.SvoError):  # twice
        fe.places_enable(4, 1, 31)
    with pytest.raises(S.SvoError):  # before init
        fe.places_query()
    assert fe.place(0, 0)["frame_t"] == -1
    fe.init(0)
    for bad in [dict(t_lo=3, t_hi=2), dict(ratio_pct=-1), dict(min_pairs=-1)]:
        with pytest.raises(S.SvoError):
            fe.places_query(**bad)
    for seq, slot in [(0, 4), (0, -1), (1, 0), (-1, 0)]:
        with pytest.raises(S.SvoError):
            fe.place(seq, slot)
    # null arguments
    lib = S.lib()
    i, d = (ctypes.c_int * 1)(), (ctypes.c_double * 3)()
    ip, dp = ctypes.cast(i, ctypes.POINTER(ctypes.c_int)), ctypes.cast(d, ctypes.POINTER(ctypes.c_double))
    assert lib.svo_frontend_places_query(fe.handle, None, 0, 9, 80, 1, 4, None, ip, ip, ip, dp, dp, None, None, None,
                                         0) == -1
    assert lib.svo_frontend_places_query(None, None, 0, 9, 80, 1, 4, ip, ip, ip, ip, dp, dp, None, None, None, 0) == -1
    assert lib.svo_frontend_places_enable(None, 4, 1, 31, None) == -1
    assert lib.svo_frontend_place(None, 0, 0, None, None, None, None, None, 0) == -1
    assert lib.svo_frontend_place(fe.handle, 0, 0, None, None, None, None, None, 0) == 0  # every output may be NULL
    with pytest.raises(S.SvoError):  # after init
        late = _resident(ctx, made, [case])
        late.init(0)
        late.places_enable(4, 1, 31)
    assert fe.places_query()["frame_t"][0] == 0  # the init frame against its own record
