"""CPU companions of test_frontend_starved_gpu.py: the oracle-side input conditions
of the starved cases (tests/starved_cases.py), checked wherever the suite runs, so
that a change of the scene generator cannot hollow the GPU tests out; and the
product's host SQPnP against the oracle's on every RANSAC fit of those loops."""
import numpy as np
import pytest

import starved_cases as C
import svo_amd as S
from svo_amd.scene import Scene


def test_ladder_tracked_counts_cover_every_pose_branch():
    """n_features 1..9 x seeds (2, 5): calculatePose sees 0, 1, 2, 3 points (features
    kept, identity pose), 4 and 5 (direct solve) and 6 or more (RANSAC)."""
    counts, hyps = set(), set()
    for c in C.LADDER:
        counts |= set(C.tracked_counts(c))
        for s in C.oracle_trace(c)[1:]:
            st = s.stats
            if st["tracked"] < 4:
                assert "hypotheses" not in st and st["inliers"] == st["tracked"]
                assert not np.any(s.pose[0]) and not np.any(s.pose[1])
            else:
                hyps.add((min(st["tracked"], 6), st["hypotheses"] > 0))
    assert {0, 1, 2, 3, 4, 5} <= counts and max(counts) >= 6, sorted(counts)
    assert {(4, True), (5, True), (6, True)} <= hyps, hyps


@pytest.mark.parametrize("case,garbage", [(C.DROPPED_64, True), (C.DROPPED_300, False),
                                          (C.DROPPED_64._replace(side="left"), True)],
                         ids=["n64", "n300", "n64-left"])
def test_dropped_frames_conditions(case, garbage):
    """A constant image at t = 3 and t = 6: a step whose RANSAC finds no model (100
    hypotheses, 0 inliers, 0 features), a step with nothing tracked that rebuilds
    the set, and at N = 64 a model accepted from garbage (inliers < tracked / 2)."""
    stats = [s.stats for s in C.oracle_trace(case)[1:]]
    assert any(C.is_no_model(s) for s in stats)
    assert any(C.is_rebuild(s) for s in stats)
    assert any(C.is_garbage_model(s) for s in stats) == garbage
    # the frames in between recover: a healthy set again two frames after each drop
    assert stats[-1]["tracked"] >= 0.9 * case.n and stats[-1]["inliers"] == stats[-1]["tracked"]


def test_right_image_dropped_adds_nothing():
    tr = C.oracle_trace(C.DROPPED_64._replace(side="right"))
    for t in C.DROPPED_64.drops:
        assert tr[t].stats["added"] == 0 and tr[t].stats["tracked"] > 0


def test_blank_sequence_has_no_features():
    for s in C.oracle_trace(C.BLANK):
        assert len(s.pts) == 0 and not np.any(s.pose[0]) and not np.any(s.pose[1])


def test_streamed_run_outgrows_a_four_frame_ring():
    """Every third frame dropped, 24 steps at N = 64: the keyframes create more map
    points than the 6 * 64 slots a ring of n_frames = 4 owns, well before the end
    (379 by t = 18, 442 by t = 19, 506 in all)."""
    case = C.STREAMED
    cum = C.cumulative_added(case)
    assert cum[case.frames - 2] > 6 * case.n
    full_at = next(t for t in range(case.frames) if cum[t] > 6 * case.n)
    assert full_at == 19 and cum[18] == 379 and cum[19] == 442 and cum[-1] == 506, cum
    assert C.oracle_trace(case)[full_at].stats["added"] == 63


def test_streamed_reclaim_case_moves_live_points():
    """C.RECLAIM's first overflowing keyframe is t = 19 with 269 live features (two
    256-thread chunks) whose map ids are scattered, 147 candidates taken and five
    steps left; C.STREAMED's only reclaim (t = 19) has no live feature."""
    assert C.assert_reclaim_moves_live_points(C.RECLAIM) == 19
    occ = C.map_occupancy(C.RECLAIM)
    assert (occ[19].map_n, occ[19].n, occ[19].take, occ[19].slots) == (2937, 269, 147, 3072)
    assert [t for t in range(1, C.RECLAIM.frames) if occ[t].reclaim] == [19]
    occ = C.map_occupancy(C.STREAMED)
    assert [t for t in range(1, C.STREAMED.frames) if occ[t].reclaim] == [19] and occ[19].n == 0


SQPNP_LOOPS = [C.STREAMED._replace(seed=sd) for sd in (4, 7, 9)] + [C.DROPPED_64, C.DROPPED_300] + C.LADDER
# 4 x the measured worst case (docstring below), capped at the loop tests' bars
RV_BAR = min(4 * 1.91e-8, 1e-7)
TV_BAR = min(4 * 1.58e-7, 1e-6)


def test_sqpnp_fit_matches_oracle_on_starved_loops():
    """Every RANSAC fit (6 or more tracked points, a model found) of the dropped-frame
    loops (seeds 4, 7, 9 with every third frame dropped; seed 4 with drops at 3 and
    6, N = 64 and 300) and of the ladder: svo_solve_pnp_sqpnp on the oracle's inlier
    set against the oracle's pose. These fits are ill-conditioned on purpose (5 to 7
    inliers out of 15 to 36 garbage matches, |t| of 7 to 15).
    Measured: 73 fits, none refused; worst |d rvec| 1.903e-8, |d tvec| 1.572e-7,
    both on seed 9, t = 3 (5 inliers of 22, |t| = 7.0); the ladder's worst is
    3.2e-9 / 5.4e-8 (seed 5, n = 9, t = 2); healthy frames agree to ~1e-9."""
    K = Scene(C.W, C.H, seed=0).K
    worst_rv = worst_tv = (0.0, None)
    fits = garbage = 0
    for case in SQPNP_LOOPS:
        for t, s in enumerate(C.oracle_trace(case)):
            st = s.stats
            if st is None or st["tracked"] < 6 or st["inliers"] == 0:
                continue
            n = st["inliers"]
            ok, rv, tv = S.solve_pnp_sqpnp(s.X[:n].astype(np.float32).astype(np.float64), s.pts[:n], K)
            assert ok, (case, t)
            fits += 1
            garbage += C.is_garbage_model(st)
            where = (case.seed, case.n, t, n, st["tracked"])
            worst_rv = max(worst_rv, (np.abs(rv - s.pose[0]).max(), where), key=lambda x: x[0])
            worst_tv = max(worst_tv, (np.abs(tv - s.pose[1]).max(), where), key=lambda x: x[0])
    print(f"{fits} fits ({garbage} from garbage): worst |d rvec| {worst_rv[0]:.4g} at {worst_rv[1]}, "
          f"|d tvec| {worst_tv[0]:.4g} at {worst_tv[1]}")
    assert fits >= 60 and garbage >= 5
    assert worst_rv[0] <= RV_BAR, worst_rv
    assert worst_tv[0] <= TV_BAR, worst_tv
