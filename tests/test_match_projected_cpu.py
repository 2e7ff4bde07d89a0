"""svo_match_projected without a GPU: the symbols, the
restatement (tests/match_projected_reference.py) against the brute-force matcher's
restatement and at the pair rule's edges, the recorded figures recomputed, and the
conditions the synthetic generator promises the GPU test."""
import ctypes
import os

import numpy as np
import pytest

import match_projected_cases as MC
import match_projected_reference as MP
import oracle as O
import orb_describe_reference as R
import svo_amd as S
from test_capi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["svo_match_projected", "svo_match_projected_time", "svo_pose_from_rvec", "svo_frontend_places_widen"]


def test_symbols_declared_bound_and_exported():
    assert set(NEW) <= set(declared_symbols())
    assert set(NEW) <= set(S.SYMBOLS)
    lib = ctypes.CDLL(S.lib_path())
    for name in NEW:
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "svo_gpu.h")).read()
    assert "typedef struct svo_proj_match_params {" in header
    p = S.ProjMatchParams()
    assert (p.radius, p.max_dist, p.ratio_pct) == (4.0, 64, 80) and ctypes.sizeof(p) == 12
    assert MP.DEFAULTS == dict(radius=p.radius, max_dist=p.max_dist, ratio_pct=p.ratio_pct)
    for name in ("match_projected", "relocalize_guided"):
        assert callable(getattr(S.Context, name))
    assert callable(S.Frontend.places_widen)


def test_null_context_is_refused_without_a_device():
    lib = S.lib()
    prm = S.ProjMatchParams()
    assert lib.svo_match_projected(None, 0, None, None, 0, 0, None, None, None, None, None, None, 64, 48,
                                   ctypes.addressof(prm), None, None, None, None, None) == -1
    assert lib.svo_match_projected_time(None, 0, None, None, 0, 0, None, None, None, None, None, None, 64, 48,
                                        ctypes.addressof(prm), 1, None) == -1
    assert lib.svo_frontend_places_widen(None, None, None, None, None, ctypes.addressof(prm), None, None, None, None,
                                         None, None, None, 0) == -1
    assert lib.svo_pose_from_rvec(None, None, None) == -1


def test_pose_from_rvec_is_the_oracles_rodrigues():
    rng = np.random.default_rng(5)
    for rv in [np.zeros(3), np.array([0.3, -0.2, 0.1]), rng.uniform(-2, 2, 3), np.array([1e-20, 0, 0])]:
        tv = rng.uniform(-1, 1, 3)
        T = S.pose_from_rvec(rv, tv)
        assert np.array_equal(T[9:], tv)
        np.testing.assert_allclose(T[:9].reshape(3, 3), O.rodrigues(rv), atol=1e-15, rtol=0)
        assert np.array_equal(MP.pose12(rv, tv)[9:], tv)


@pytest.mark.parametrize("name", sorted(MC.MEASURED))
def test_measured_figures_recomputed(name):
    got = MC.measured_row(name)
    print(name, got)
    assert got == MC.MEASURED[name]
    d, wn = MC.scene_inputs(name), MC.scene_want(name)
    # the pairs are (frame, map) in ascending frame index, every index once
    p = wn["pairs"]
    assert np.all(np.diff(p[:, 0]) > 0) and len(set(p[:, 1].tolist())) == len(p)
    assert p[:, 0].max() < len(d["kxy"]) and p[:, 1].max() < len(d["map_xyz"])


def test_a_window_over_the_whole_frame_is_the_brute_force_matcher():
    """radius >= max(w, h) and every point visible: idx / dist equal R.knn2 against
    the usable keypoints (their indices mapped back)."""
    rng = np.random.default_rng(11)
    w, h = MC.W, MC.H
    s = MC.synth(65, 257)
    kxy = s["kxy"].copy()
    kxy[::9] = [-3.0, 5.0]          # outside
    kxy[4::31, 1] = np.nan          # not a number
    kxy[7] = [w, 3.0]               # on the far edge: not usable
    kdesc = s["kdesc"].copy()
    kdesc[100:140] = kdesc[100]     # ties: the lowest index wins both places
    px = rng.uniform(0, 1, (65, 2)) * [w - 1, h - 1]
    xyz = np.c_[(px[:, 0] - s["K4"][2]) / s["K4"][0] * 3.0, (px[:, 1] - s["K4"][3]) / s["K4"][1] * 3.0, np.full(65, 3.0)]
    T = np.r_[np.eye(3).ravel(), np.zeros(3)]
    assert MP.project(xyz, T, s["K4"], (w, h))[1].all()
    use = np.nonzero(MP.usable(kxy, (w, h)))[0]
    assert 200 < len(use) < 257
    for radius in (float(max(w, h)), 1e6):
        idx, dist, _, ncand = MP.match_projected(xyz, s["pdesc"], kxy, kdesc, T, s["K4"], (w, h), radius)
        ki, kd = R.knn2(s["pdesc"], kdesc[use])
        assert np.array_equal(idx, use[ki].astype(np.int32)) and np.array_equal(dist, kd)
        assert np.all(ncand == len(use))


def _pairs_of(rows, **kw):
    idx = np.array([r[:2] for r in rows], np.int32)
    dist = np.array([r[2:] for r in rows], np.int32)
    return MP.pairs(idx, dist, **kw).tolist()


def test_pair_rule_edges():
    # a single candidate passes the ratio test; a failed ratio does not bid; no candidate, no bid
    rows = [(3, -1, 40, 257), (5, 6, 40, 50), (7, 8, 40, 51), (-1, -1, 257, 257)]
    assert _pairs_of(rows) == [[3, 0], [7, 2]]        # 40 * 100 < 80 * 51, and not < 80 * 50
    assert _pairs_of(rows, ratio_pct=0) == [[3, 0], [5, 1], [7, 2]]
    # max_dist is inclusive; 0 keeps only identical descriptors, 256 everything
    rows = [(1, -1, 0, 257), (2, -1, 64, 257), (3, -1, 65, 257), (4, -1, 256, 257)]
    assert _pairs_of(rows, max_dist=64) == [[1, 0], [2, 1]]
    assert _pairs_of(rows, max_dist=0) == [[1, 0]]
    assert _pairs_of(rows, max_dist=256) == [[1, 0], [2, 1], [3, 2], [4, 3]]
    # a contested keypoint goes to the smallest distance, then to the lowest point; ascending keypoint
    rows = [(9, -1, 30, 257), (9, -1, 20, 257), (9, -1, 20, 257), (2, -1, 5, 257)]
    assert _pairs_of(rows) == [[2, 3], [9, 1]]
    assert _pairs_of([]) == []


def test_best_two_ties_go_to_the_lowest_keypoint():
    """257 keypoints on one pixel, equal descriptors in groups: (d, j) lexicographic."""
    kxy = np.tile(np.float32([10.25, 7.5]), (257, 1))
    kdesc = np.zeros((257, 32), np.uint8)
    kdesc[:200, 0] = 0xFF           # distance 8 from a zero descriptor
    kdesc[200:, 0] = 0x0F           # distance 4: the best two are 200 and 201
    xyz = np.array([[(10.0 - 32) / 50 * 2, (7.0 - 24) / 50 * 2, 2.0]] * 4)
    T = np.r_[np.eye(3).ravel(), np.zeros(3)]
    idx, dist, proj, ncand = MP.match_projected(xyz, np.zeros((4, 32), np.uint8), kxy, kdesc, T, MC.K4, (MC.W, MC.H))
    assert idx.tolist() == [[200, 201]] * 4 and dist.tolist() == [[4, 4]] * 4 and np.all(ncand == 257)
    assert MP.pairs(idx, dist).tolist() == []                  # 4 * 100 < 80 * 4 fails
    assert MP.pairs(idx, dist, ratio_pct=0).tolist() == [[200, 0]]  # four equal bids: the lowest point


@pytest.mark.parametrize("n_pts", [255, 256, 257])
@pytest.mark.parametrize("n_kp", [255, 256, 257])
def test_generator_conditions(n_pts, n_kp):
    seed = MC.seed_of(n_pts, n_kp)
    s, w = MC.synth(n_pts, n_kp, seed), MC.synth_want(n_pts, n_kp, seed)
    assert MP.usable(s["kxy"], s["size"]).sum() >= n_kp - 1  # uniform over the frame (a cast can reach the far edge)
    vis = MP.project(s["xyz"], s["T"], s["K4"], s["size"])[1]
    nc = w["ncand"][vis]
    bid_for = w["idx"][MP.bids(w["idx"], w["dist"]), 0]
    print(n_pts, n_kp, "visible", vis.sum(), ">= 2 candidates", (nc >= 2).sum(), "none", (nc == 0).sum(),
          "contested keypoints", (np.bincount(bid_for) >= 2).sum(), "pairs", len(w["pairs"]))
    assert 0 < vis.sum() < n_pts                     # some points are behind the camera or outside
    assert 2 * (nc >= 2).sum() >= vis.sum()
    assert (nc == 0).sum() > 0
    assert (np.bincount(bid_for) >= 2).sum() > 0
    assert len(w["pairs"]) >= 50
    proj = w["proj"]
    assert np.any(np.all(proj == -1, axis=1))        # a point with pz <= 0
