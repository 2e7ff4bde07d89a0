"""The deferred keyframe: behind RANSAC only the outlier
compaction runs ahead of the next temporal LK; the stereo LK of exactly the take,
the append and a second LK launch over the new features run beside it. Nothing
about the results changes: every step against the oracle loop, and array for
array against the speculative schedule (SVO_FE_DEFER_KF=0, or an explicitly set
SVO_FE_SPEC_MARGIN). It is the default from 128,000 features a batch on (where the
next LK is long enough to hide it); the small batches here select it with
SVO_FE_DEFER_KF=1. 320x240 sequences of tests/starved_cases.py."""
import contextlib
import os

import numpy as np
import pytest

import starved_cases as C
import svo_amd as S
from stereo_rows_reference import DEFAULTS, RowsOracleLoop, WideScene
from svo_amd.scene import Scene

pytestmark = pytest.mark.gpu

K = Scene(C.W, C.H, seed=0).K
SWITCHES = ("SVO_FE_DEFER_KF", "SVO_FE_SPEC_MARGIN", "SVO_FE_SPEC_EARLY")
KEYS = ("tracked", "lk_iterations", "inliers", "added", "features")
DEFER, SPECULATE = dict(SVO_FE_DEFER_KF="1"), dict(SVO_FE_DEFER_KF="0")
# three healthy sequences, 12 steps
HEALTHY = [C.Case(seed, 200, 13) for seed in (3, 5, 9)]
# healthy | both images dropped at t = 3, 6 (loses everything, rebuilds) | healthy | never
# a corner (takes nothing, ever)
MIXED = [C.BLANK._replace(blank=False), C.DROPPED_64, C.BLANK._replace(seed=9, blank=False), C.BLANK]


@contextlib.contextmanager
def switches(**kv):
    """The schedule's environment switches for the front ends created inside: the
    three unset (the default environment) except those given."""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _make(ctx, cases, n_frames=None, **kw):
    T, n = cases[0].frames, cases[0].n
    return S.Frontend(ctx, S.FrontendConfig(C.W, C.H, K, n_seq=len(cases), n_frames=n_frames or T, n_features=n, **kw))


def _resident(ctx, cases, **kw):
    fe = _make(ctx, cases, **kw)
    for s, c in enumerate(cases):
        for t, (L, R) in enumerate(C.frames(c)):
            fe.set_frame(s, t, L, R)
    return fe


def _snapshot(fe, n_seq, st=None):
    """What a step leaves, as bytes: the batch's counts, then per sequence the
    feature list, the pose and the map points of its features (gathered by map id)."""
    out = [tuple(st[k] for k in KEYS)] if st is not None else [()]
    for q in range(n_seq):
        out.append((fe.features(q).tobytes(), np.r_[fe.pose(q)].tobytes(), fe.map_points(q).tobytes()))
    return out


def _run(fe, cases, steps=None, each=None):
    """init + the steps; the snapshots and the steps' statistics."""
    fe.init(0)
    snaps, stats = [_snapshot(fe, len(cases))], []
    for t in range(1, (steps or cases[0].frames - 1) + 1):
        st = fe.step(t).as_dict()
        stats.append(st)
        snaps.append(_snapshot(fe, len(cases), st))
        if each:
            each(t, st)
    return snaps, stats


def _against_oracle(fe, cases, snaps_out=None, deferred=True):
    """Every step of the cases against their oracle loops (test_frontend_gpu's
    bars): counts, bit-equal feature lists, poses, map points; the schedule's report
    (deferred: no serial keyframe, no margin; else: the speculation's margin)."""
    traces = [C.oracle_trace(c) for c in cases]
    fe.init(0)
    for q, tr in enumerate(traces):
        assert np.array_equal(fe.features(q), tr[0].pts), f"seq {q} features at init"
    for t in range(1, cases[0].frames):
        st = fe.step(t).as_dict()
        for k in KEYS:
            want = sum(tr[t].stats[k] for tr in traces)
            assert st[k] == want, f"{k} differs at t={t}: {st[k]} vs {want}"
        assert st["serial_keyframe"] == 0, t
        assert st["spec_margin"] == 0 if deferred else st["spec_margin"] >= 32, (t, st["spec_margin"])
        for q, tr in enumerate(traces):
            assert np.array_equal(fe.features(q), tr[t].pts), f"seq {q} features differ at t={t}"
            rv, tv = fe.pose(q)
            np.testing.assert_allclose(rv, tr[t].pose[0], atol=1e-7)
            np.testing.assert_allclose(tv, tr[t].pose[1], atol=1e-6)
            np.testing.assert_allclose(fe.map_points(q), tr[t].X, rtol=2e-5, atol=1e-6)
        if snaps_out is not None:
            snaps_out.append(_snapshot(fe, len(cases), st))


# ---------------------------------------------------------------- 1. the default path
def test_deferred_follows_the_oracle_and_equals_the_other_schedules(ctx):
    """Three sequences, 12 steps, deferred: every step equals the oracle loop and
    reports neither a serial keyframe nor a speculation margin. With nothing set (a
    batch this small speculates by default) every step equals the oracle loop too,
    and that run, the speculative schedule (margin 32), the serial one (-1) and
    SVO_FE_DEFER_KF=0 leave the deferred run's arrays at every step."""
    with switches(**DEFER):
        fe = _resident(ctx, HEALTHY)
        deferred = []
        _against_oracle(fe, HEALTHY, deferred)
        fe.close()
    with switches():
        fe = _resident(ctx, HEALTHY)
        default = []
        _against_oracle(fe, HEALTHY, default, deferred=False)
        fe.close()
    assert default == deferred
    assert any(C.oracle_trace(c)[t].stats["added"] > 0 for c in HEALTHY for t in range(1, 13))
    for env in (dict(SVO_FE_SPEC_MARGIN="32"), dict(SVO_FE_SPEC_MARGIN="-1"), dict(SVO_FE_DEFER_KF="0")):
        with switches(**env):
            fe = _resident(ctx, HEALTHY)
            snaps, stats = _run(fe, HEALTHY)
            fe.close()
        assert snaps[1:] == deferred, env
        if env.get("SVO_FE_SPEC_MARGIN") == "-1":
            assert all(st["serial_keyframe"] == 1 for st in stats)
        else:
            assert all(st["spec_margin"] >= 32 for st in stats), env  # the speculation went out


# ---------------------------------------------------------------- 2. the first index
@pytest.mark.parametrize("n", [5, 7])
def test_kept_counts_off_the_wave_size(ctx, n):
    """n_features 5 and 7, one sequence: the second LK launch starts at a kept count
    that is no multiple of the four features a wave tracks; in other steps the take's
    stereo match adds nothing, or nothing is taken."""
    case = next(c for c in C.LADDER if c.n == n and c.seed == 5)
    st = [s.stats for s in C.oracle_trace(case)[1:]]
    assert any(s["added"] > 0 and (s["features"] - s["added"]) % 4 != 0 for s in st[:-1]), st
    assert any(s["take"] > 0 and s["added"] == 0 for s in st) and any(s["take"] == 0 for s in st), st
    with switches(**DEFER):
        fe = _resident(ctx, [case])
        _against_oracle(fe, [case])
        fe.close()


# ---------------------------------------------------------------- 3. empty and full takes
def test_empty_second_range_and_a_take_of_everything(ctx):
    """One batch: a sequence that takes nothing (the second LK range is empty)
    beside sequences that add, and a sequence that loses everything, so that fewer
    than 4 points are tracked and the take is n_features."""
    tr = [C.oracle_trace(c) for c in MIXED]
    T, n = MIXED[0].frames, MIXED[0].n
    steps = range(1, T)
    assert any(tr[3][t].stats["take"] == 0 and tr[0][t].stats["added"] > 0 for t in steps)
    assert any(tr[1][t].stats["tracked"] < 4 and tr[1][t].stats["take"] == n for t in steps)
    with switches(**DEFER):
        fe = _resident(ctx, MIXED)
        _against_oracle(fe, MIXED)
        fe.close()


# ---------------------------------------------------------------- 4. bucketed, row SAD
def _rows_frontend(ctx, scenes, T, n):
    P0, P1 = scenes[0].projections()
    fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, scenes[0].K, n_seq=len(scenes), n_frames=T, n_features=n,
                                          P_left=P0, P_right=P1))
    fe.set_stereo_matcher(S.StereoRowsParams(**DEFAULTS))
    for s, sc in enumerate(scenes):
        for t in range(T):
            fe.set_frame(s, t, sc.frame(t), sc.right(t))
    return fe


@pytest.mark.parametrize("kind", ["bucketed", "rows"])
def test_bucketed_and_row_sad_equal_their_speculative_runs(ctx, kind):
    """6 steps each, deferred against SVO_FE_DEFER_KF=0 of the same configuration."""
    cases = [C.Case(seed, 200, 7) for seed in (3, 5)]
    runs = []
    for env in (DEFER, SPECULATE):
        with switches(**env):
            if kind == "bucketed":
                fe = _resident(ctx, cases, bucket_size=50, per_bucket=4)
            else:
                fe = _rows_frontend(ctx, [WideScene(C.W, C.H, seed=s) for s in (3, 5)], 7, 200)
            snaps, stats = _run(fe, cases, steps=6)
            fe.close()
        runs.append(snaps)
        assert sum(st["added"] for st in stats) > 0
        if env == DEFER:
            assert all(st["serial_keyframe"] == 0 and st["spec_margin"] == 0 for st in stats)
    assert runs[0] == runs[1]


def test_row_sad_deferred_follows_its_restatement(ctx):
    """The row-SAD matcher's deferred run against the oracle loop with the numpy
    restatement in the stereo LK's place (the speculative run's own reference)."""
    with switches(**DEFER):
        fe = _rows_frontend(ctx, [WideScene(C.W, C.H, seed=3)], 5, 200)
        fe.init(0)
        ref = RowsOracleLoop(WideScene(C.W, C.H, seed=3), 200).init(0)
        assert np.array_equal(fe.features(0), ref.pts)
        for t in range(1, 5):
            st = fe.step(t).as_dict()
            rs = ref.step(t)
            for k in KEYS:
                assert st[k] == rs[k], (k, t)
            assert np.array_equal(fe.features(0), ref.pts), t
            np.testing.assert_allclose(fe.map_points(0), ref.X, rtol=2e-5, atol=1e-6)
        fe.close()


# ---------------------------------------------------------------- 5. streamed frames
def test_streamed_ring_equals_the_resident_run(ctx):
    """queue_frames into a ring of 4, 10 steps: frame t's slot is released only
    behind the second LK launch of step t + 1 (frame t's right image is read by the
    deferred stereo LK beside LK(t + 1)), so the streamed run equals the resident one."""
    cases = [C.Case(seed, 200, 11) for seed in (3, 5)]
    fr = [C.frames(c) for c in cases]
    with switches(**DEFER):
        fe = _resident(ctx, cases)
        want, _ = _run(fe, cases)
        fe.close()
        fe = _make(ctx, cases, n_frames=4)
        for t in range(3):
            fe.queue_frames(t, [f[t][0] for f in fr], [f[t][1] for f in fr])
        fe.init(0)
        got = [_snapshot(fe, len(cases))]
        for t in range(1, cases[0].frames):
            if t + 2 < cases[0].frames:
                fe.queue_frames(t + 2, [f[t + 2][0] for f in fr], [f[t + 2][1] for f in fr])
            st = fe.step(t).as_dict()
            assert st["serial_keyframe"] == 0
            got.append(_snapshot(fe, len(cases), st))
        fe.upload_wait(cases[0].frames - 1)
        fe.close()
    assert got == want


# ---------------------------------------------------------------- 6. window, place memory
def test_window_and_place_records_equal_the_speculative_runs(ctx):
    """A window of 4 and a place memory of 8 records, 8 steps: the recorded lists
    (frames, map ids, pixels; descriptors, pixels, world points) are those of the
    speculative run, and the window's ids those of the oracle loop."""
    cases = [C.Case(seed, 200, 9) for seed in (3, 5)]
    runs = []
    for env in (DEFER, SPECULATE):
        with switches(**env):
            fe = _resident(ctx, cases)
            fe.window_enable(4)
            fe.places_enable(8, 1, 31)
            seen = []

            def each(t, st):
                for q in range(len(cases)):
                    w = fe.window(q)
                    seen.append((list(w["frame_t"]), [i.tobytes() for i in w["ids"]], [x.tobytes() for x in w["xy"]]))
                    if env == DEFER:
                        tr = C.oracle_trace(cases[q])[t]
                        assert w["frame_t"][-1] == t and np.array_equal(w["ids"][-1], tr.mid), (q, t)
                        assert np.array_equal(w["xy"][-1], tr.pts), (q, t)

            snaps, _ = _run(fe, cases, each=each)
            places = [[(p["frame_t"], p["desc"].tobytes(), p["xy"].tobytes(), p["xyz"].tobytes())
                       for p in (fe.place(q, k) for k in range(8))] for q in range(len(cases))]
            assert sorted(p[0] for p in places[0]) == list(range(1, 9))
            fe.close()
        runs.append((snaps, seen, places))
    assert runs[0] == runs[1]


# ---------------------------------------------------------------- 7. the other schedules
def test_reference_rule_and_orb_keep_their_schedule(ctx):
    """SVO_KF_REFERENCE and ORB never defer: with nothing set and with
    SVO_FE_DEFER_KF=1 they report what they report with SVO_FE_DEFER_KF=0 -- the
    reference rule its speculation (a margin of at least 32), ORB the serial keyframe
    at every step."""
    cases = [C.Case(seed, 200, 6) for seed in (3, 5)]
    for kw in (dict(keyframe_rule=S.KF_REFERENCE, features_to_track=1 << 30), dict(use_orb=1)):
        runs = []
        for env in ({}, DEFER, SPECULATE):
            with switches(**env):
                fe = _resident(ctx, cases, **kw)
                snaps, stats = _run(fe, cases)
                fe.close()
            runs.append((snaps, [(st["serial_keyframe"], st["spec_margin"], st["keyframes"]) for st in stats]))
        assert runs[0] == runs[1] == runs[2], kw
        if "use_orb" in kw:
            assert all(s == 1 and m == 0 for s, m, _ in runs[0][1]), runs[0][1]
        else:
            assert all(m >= 32 for _, m, _ in runs[0][1]), runs[0][1]
            assert 0 < sum(k for _, _, k in runs[0][1]) < 5 * len(cases)


# ---------------------------------------------------------------- 8. the default
def test_large_batches_defer_by_default(ctx):
    """64 sequences of 2,000 features (128,000 a batch) with nothing set: deferred --
    no serial keyframe, no speculation margin --, and equal to SVO_FE_DEFER_KF=0 at
    the first, a middle and the last sequence; 63 sequences speculate."""
    case = C.Case(3, 2000, 4)
    fr = C.frames(case)
    runs = []
    for n_seq, env in ((64, {}), (64, SPECULATE), (63, {})):
        with switches(**env):
            fe = S.Frontend(ctx, S.FrontendConfig(C.W, C.H, K, n_seq=n_seq, n_frames=4, n_features=2000))
            for s in range(n_seq):
                for t, (L, R) in enumerate(fr):
                    fe.set_frame(s, t, L, R)
            fe.init(0)
            run = []
            for t in range(1, 4):
                st = fe.step(t).as_dict()
                run.append((st["serial_keyframe"], st["spec_margin"], [st[k] // n_seq for k in KEYS],
                            [(fe.features(q).tobytes(), fe.map_points(q).tobytes()) for q in (0, 31, n_seq - 1)]))
            fe.close()
        runs.append(run)
    assert all(s == 0 and m == 0 for s, m, _, _ in runs[0]), [(s, m) for s, m, _, _ in runs[0]]
    for other in runs[1:]:
        assert all(m >= 32 for _, m, _, _ in other)
        assert [r[2:] for r in other] == [r[2:] for r in runs[0]]
    assert runs[0][-1][2][3] > 0  # features were added
