"""The pieces compose (320x240): the dropped-frame sequence of tests/starved_cases.py
loses its features at frame 3 and rebuilds them at frame 4 in a new world; the
bounded places_query finds a record made before the loss, places_widen confirms
frame 4's pose in the old world, and one loop edge from that record's frame to
frame 4 lets svo_pose_graph_optimize carry frames 4 and 5 back into it."""
import numpy as np
import pytest

import match_projected_cases as MC
import places_cases as P
import pose_graph_reference as R
import starved_cases as C
import svo_amd as S
from test_places_gpu import BATCH, _resident

pytestmark = pytest.mark.gpu

FRAMES = [0, 1, 2, 4, 5]  # the graph's nodes (frame 3 is the blank one)
INFO = R.info_diag(0.02, 0.002)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture
def made():
    fes = []
    yield fes
    for fe in fes:
        fe.close()


def truth_distance(T, t):
    """(rotation error in degrees against Scene.R(t), |t| in metres: the camera only rotates)"""
    dR = T[:9].reshape(3, 3) @ C.scene(C.DROPPED_300).R(t).T
    return float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))), float(np.linalg.norm(T[9:]))


def test_a_loop_edge_from_place_memory_rejoins_the_old_world(ctx, made):
    fe = _resident(ctx, made, BATCH)
    fe.places_enable(8, 1, 31)
    pose = {}
    fe.init(0)
    pose[0] = [S.pose_from_rvec(*fe.pose(s)) for s in range(2)]
    for t in range(1, P.REBUILD_T + 1):
        fe.step(t)
        pose[t] = [S.pose_from_rvec(*fe.pose(s)) for s in range(2)]
    res = fe.places_query(*P.BOUND)
    wide = fe.places_widen(res)
    assert res["frame_t"][0] == P.PICKED["n300"]["frame"] and wide["ok"][0] == 1
    fe.step(5)
    pose[5] = [S.pose_from_rvec(*fe.pose(s)) for s in range(2)]

    rec = int(res["frame_t"][0])  # the record's frame, a node of the graph
    T4_old = S.pose_from_rvec(wide["rvec"][0], wide["tvec"][0])  # frame 4 in the record's world
    edge = ctx.pose_graph_edge
    ij = np.array([(0, 1), (1, 2), (3, 4), (FRAMES.index(rec), 3)], np.int32)
    probs = []
    for s in range(2):
        T = [pose[t][s] for t in FRAMES]
        Z = [edge(T[0], T[1]), edge(T[1], T[2]), edge(T[3], T[4])]
        # the dropped sequence: the widened pose against the record frame's; the healthy one: its own poses
        Z.append(edge(T[FRAMES.index(rec)], T4_old if s == 0 else T[3]))
        probs.append((np.array(T), np.array(Z)))
    poses = np.stack([p[0] for p in probs])
    fixed = np.zeros((2, 5), np.uint8)
    fixed[:, 0] = 1
    out, costs, its, cgs = ctx.pose_graph_optimize(poses, fixed, np.stack([ij, ij]), np.stack([p[1] for p in probs]),
                                                   np.tile(INFO, (2, 4, 1)), max_iterations=30)
    # the dropped sequence: a tree, so every measurement is met
    Z = probs[0][1]
    want4 = R.compose(Z[3], poses[0, FRAMES.index(rec)], np.longdouble)
    want5 = R.compose(Z[2], want4, np.longdouble)
    d4, d5 = np.abs(out[0, 3] - want4).max(), np.abs(out[0, 4] - want5).max()
    before = [truth_distance(poses[0, k], FRAMES[k]) for k in (3, 4)]
    after = [truth_distance(out[0, k], FRAMES[k]) for k in (3, 4)]
    print(f"dropped: cost {costs[0, 0]:.3e} -> {costs[0, 1]:.3e} in {its[0]} iterations / {cgs[0]} products; "
          f"frame 4 off its composed pose by {d4:.2e}, frame 5 by {d5:.2e}")
    print(f"frame 4 against the truth: {before[0][0]:.3f} deg / {before[0][1]:.3f} m -> {after[0][0]:.3f} deg / "
          f"{after[0][1]:.3f} m; frame 5: {before[1][0]:.3f} deg / {before[1][1]:.3f} m -> {after[1][0]:.3f} deg / "
          f"{after[1][1]:.3f} m")
    assert d4 < 1e-8 and d5 < 1e-8
    assert np.abs(out[0, 3] - T4_old).max() < 1e-8
    assert np.abs(out[0, :3] - poses[0, :3]).max() < 1e-8
    assert np.array_equal(out[0, 0].view(np.uint64), poses[0, 0].view(np.uint64))  # the fixed node
    assert costs[0, 1] < 1e-12 * costs[0, 0]
    # DESIGN.md section 3e's bar for frame 4 (the widened pose's), and no more
    m = MC.MEASURED["n300"]
    assert after[0][0] <= 2 * m["rot_deg"] and after[0][1] <= 2 * m["trans_m"]
    assert before[0][0] > 1.0  # the new world's frame 4 was the identity: degrees off the old world's
    # the healthy sequence: nothing to correct
    assert costs[1, 0] < 1e-20 and costs[1, 1] <= costs[1, 0]
    assert np.abs(out[1] - poses[1]).max() < 1e-12
