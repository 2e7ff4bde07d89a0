"""The place memory's rules on the CPU: the restatement
(tests/places_reference.py) on the dropped-frame sequences, the conditions the
GPU tests rely on, and the figures recorded in tests/places_cases.py, recomputed.
No GPU."""
import numpy as np
import pytest

import places_cases as P
import places_reference as PR
import starved_cases as C
import svo_amd as S

NEW = ["svo_frontend_places_enable", "svo_frontend_place", "svo_frontend_places_query", "svo_frontend_places_time",
       "svo_match_filter_batch"]


def test_new_symbols_are_declared_and_bound():
    assert set(NEW) <= set(S.SYMBOLS)
    assert S.PLACES_MAX_SLOTS == 16
    for name in ("places_enable", "place", "places_query"):
        assert hasattr(S.Frontend, name)
    assert hasattr(S.Context, "match_filter_batch")


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_loss_and_rebuild_conditions(name):
    """Frame 4 is a rebuild from nothing under the identity pose; the blank frames'
    records are empty at N = 300, and frame 6's at N = 64 (frame 3 keeps the 6
    survivors of a garbage model there, 5 of them valid)."""
    tr = C.oracle_trace(P.CASES[name])
    assert C.is_rebuild(tr[P.REBUILD_T].stats)
    assert not np.any(tr[P.REBUILD_T].pose[0]) and not np.any(tr[P.REBUILD_T].pose[1])
    sizes = [len(P.records(name)[t]["desc"]) for t in range(P.CASES[name].frames)]
    print(name, "record sizes", sizes)
    assert sizes == P.RECORD_SIZES[name]
    assert sizes[6] == 0 and (sizes[3] == 0 if name == "n300" else sizes[3] == 5)
    for t, r in P.records(name).items():  # a record is an ordered subset of the frame's list
        pts = tr[t].pts
        at = [int(np.flatnonzero((pts == p).all(axis=1))[0]) for p in r["xy"]]
        assert at == sorted(at) and len(r["xyz"]) == len(r["xy"]) == len(r["desc"])


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_bounded_query_finds_the_old_world(name):
    """Frame 4 against [0, 2] picks frame 1 (N = 300: 172 pairs, the tie with frame 2
    going to the older; N = 64: 15 pairs, the same tie) and its pose is the old
    world's; the recorded figures hold."""
    res = P.query(name, P.REBUILD_T, *P.BOUND)
    want = P.PICKED[name]
    print(name, "bounded query of frame 4:", res["counts"], res["frame_t"], len(res["inliers"]))
    assert res["ok"] and res["frame_t"] == want["frame"] == 1 and res["n_pairs"] == want["pairs"]
    assert res["counts"][1] == res["counts"][2] > res["counts"][0]
    assert np.all(np.diff(res["pairs"][:, 0]) > 0)  # ascending query index
    import orb_describe_cases as K
    rot, trans = K.pose_error(C.scene(P.CASES[name]), P.REBUILD_T, res["rvec"], res["tvec"])
    assert abs(rot - want["rot_deg"]) < 1e-3 and abs(trans - want["trans_m"]) < 1e-3
    # the unbounded query of the same frame searches the empty record of frame 3 too and picks the same
    free = P.query(name, P.REBUILD_T)
    assert free["frame_t"] == 1 and free["counts"][3] == 0


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_unbounded_query_prefers_the_new_world(name):
    """As soon as a record made after the loss exists, it wins on pairs: query 5
    picks frame 4 -- a pose in the wrong world (the rotation since the rebuild, about
    2.2 degrees), which is why the query takes a bound."""
    res = P.query(name, 5)
    assert res["frame_t"] == 4 and res["n_pairs"] == P.MEASURED[name][(5, 4)]["pairs"]
    assert P.query(name, 5, *P.BOUND)["frame_t"] in (0, 1, 2)


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_recorded_figures(name):
    for (tq, tr), want in P.MEASURED[name].items():
        got = P.row(name, tq, tr)
        print(name, (tq, tr), got)
        for k in ("nq", "nt", "pairs", "inliers"):
            assert got[k] == want[k], (name, tq, tr, k, got[k])
        assert abs(got["rot_deg"] - want["rot_deg"]) < 1e-3 and abs(got["trans_m"] - want["trans_m"]) < 1e-3


def test_query_rule_edges():
    """No record in the bound, only empty records, and min_pairs above the best count give no result."""
    q = P.records("n300")[4]
    qs = dict(desc=q["desc"], xy=q["xy"])
    recs = {f: r for f, r in P.records("n300").items() if f < 4}
    assert PR.query(qs, recs, 10, 20, P.SCENE_K)["frame_t"] == -1
    r = PR.query(qs, recs, 3, 3, P.SCENE_K)
    assert r["frame_t"] == -1 and r["counts"] == {3: 0} and not r["ok"]
    r = PR.query(qs, recs, 0, 2, P.SCENE_K, min_pairs=173)
    assert r["frame_t"] == -1 and r["n_pairs"] == 172 and not r["ok"]
    assert PR.query(qs, recs, 0, 2, P.SCENE_K, min_pairs=172)["frame_t"] == 1
