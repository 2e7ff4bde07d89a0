"""svo_match_projected on the device against the numpy
restatement (tests/match_projected_reference.py), bit for bit in every output:
the synthetic problems of tests/match_projected_cases.py at every count around
the wave and the block, the rules' edges built by hand, the existing brute-force
matcher as a second witness, a batch, the error returns, and the recorded scenes
with Context.relocalize_guided."""
import ctypes

import numpy as np
import pytest

import match_projected_cases as MC
import match_projected_reference as MP
import svo_amd as S

pytestmark = pytest.mark.gpu

EYE = np.r_[np.eye(3).ravel(), np.zeros(3)]
K64 = np.array([64.0, 64.0, 32.0, 24.0])  # powers of two: the projections below are exact


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(got, want, what=""):
    """got: Context.match_projected's tuple of one problem; want: dict of idx, dist, proj, pairs."""
    idx, dist, proj, pairs, n = got
    assert np.array_equal(idx, want["idx"]), f"{what}: idx"
    assert np.array_equal(dist, want["dist"]), f"{what}: dist"
    assert np.array_equal(_u32(proj), _u32(want["proj"])), f"{what}: proj"
    assert n == len(want["pairs"]), f"{what}: n_pairs {n} != {len(want['pairs'])}"
    assert np.array_equal(pairs[:n], want["pairs"]), f"{what}: pairs"
    assert np.all(pairs[n:] == -1), f"{what}: rows past n_pairs written"


def _want(xyz, pdesc, kxy, kdesc, T, K, size, radius=4.0, max_dist=64, ratio_pct=80):
    idx, dist, proj, ncand = MP.match_projected(xyz, pdesc, kxy, kdesc, T, K, size, radius)
    return dict(idx=idx, dist=dist, proj=proj, ncand=ncand, pairs=MP.pairs(idx, dist, max_dist, ratio_pct))


def _both(ctx, xyz, pdesc, kxy, kdesc, T, K, size, what="", **prm):
    want = _want(xyz, pdesc, kxy, kdesc, T, K, size, **prm)
    got = ctx.match_projected(xyz, pdesc, kxy, kdesc, T, K, size, S.ProjMatchParams(**prm))
    _check(got, want, what)
    return got, want


def _at(px, z=1.0):
    """World points (identity pose, K64) that project exactly onto the pixels px."""
    px = np.asarray(px, np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(px),))
    return np.c_[(px[:, 0] - 32.0) / 64.0 * z, (px[:, 1] - 24.0) / 64.0 * z, z]


# ---------------------------------------------------------------- synthetic problems
def test_every_count_around_the_wave_and_the_block(ctx):
    """Counts 0, 1, 63, 64, 65, 255, 256, 257 for the points and for the keypoints:
    64 problems, each alone."""
    seen = 0
    for n_pts in MC.COUNTS:
        for n_kp in MC.COUNTS:
            seed = MC.seed_of(n_pts, n_kp)
            s = MC.synth(n_pts, n_kp, seed)
            got = ctx.match_projected(s["xyz"], s["pdesc"], s["kxy"], s["kdesc"], s["T"], s["K4"], s["size"])
            _check(got, MC.synth_want(n_pts, n_kp, seed), f"{n_pts} points, {n_kp} keypoints")
            seen += got[4]
    assert seen > 1000


def test_32_problems_in_one_launch_leave_the_padding_alone(ctx):
    sizes = [(a, b) for a in MC.COUNTS[1:] for b in MC.COUNTS[1:]][5:37]
    sizes[3], sizes[17] = (0, 64), (65, 0)
    assert len(sizes) == 32 and len(set(sizes)) == 32
    P, ps, ks = 32, 300, 280
    xyz = np.full((P, ps, 3), np.nan)
    pdesc = np.full((P, ps, 32), 0xAA, np.uint8)
    kxy = np.full((P, ks, 2), 5.0, np.float32)   # padding that would match if it were read
    kdesc = np.full((P, ks, 32), 0xAA, np.uint8)
    T = np.zeros((P, 12))
    for p, (a, b) in enumerate(sizes):
        s = MC.synth(a, b, MC.seed_of(a, b))
        xyz[p, :a], pdesc[p, :a], kxy[p, :b], kdesc[p, :b], T[p] = s["xyz"], s["pdesc"], s["kxy"], s["kdesc"], s["T"]
    held = dict(idx=np.full((P, ps, 2), -7, np.int32), dist=np.full((P, ps, 2), -7, np.int32),
                proj=np.full((P, ps, 2), -7, np.float32), pairs=np.full((P, ks, 2), -7, np.int32))
    idx, dist, proj, pairs, n = ctx.match_projected(xyz, pdesc, kxy, kdesc, T, MC.synth(1, 1)["K4"], (MC.W, MC.H),
                                                    n_pts=[a for a, _ in sizes], n_kp=[b for _, b in sizes], **held)
    assert idx is held["idx"] and pairs is held["pairs"]
    for p, (a, b) in enumerate(sizes):
        w = MC.synth_want(a, b, MC.seed_of(a, b))
        assert np.array_equal(idx[p, :a], w["idx"]) and np.array_equal(dist[p, :a], w["dist"]), p
        assert np.array_equal(_u32(proj[p, :a]), _u32(w["proj"])), p
        assert n[p] == len(w["pairs"]) and np.array_equal(pairs[p, : n[p]], w["pairs"]), p
        assert np.all(idx[p, a:] == -7) and np.all(dist[p, a:] == -7) and np.all(proj[p, a:] == -7), p
        assert np.all(pairs[p, n[p]:] == -7), p


def test_radius_40_on_320x240_spans_cells_and_the_border(ctx):
    s = MC.synth(257, 257, 0, 320, 240)
    for radius in (40.0, 7.5, 0.5):
        got, want = _both(ctx, s["xyz"], s["pdesc"], s["kxy"], s["kdesc"], s["T"], s["K4"], s["size"],
                          f"radius {radius}", radius=radius)
        print(f"320x240 radius {radius}: candidates per visible point "
              f"{want['ncand'][want['idx'][:, 0] >= 0].mean() if (want['idx'][:, 0] >= 0).any() else 0:.1f}, "
              f"{got[4]} pairs")
    assert _want(s["xyz"], s["pdesc"], s["kxy"], s["kdesc"], s["T"], s["K4"], s["size"], 40.0)["ncand"].max() > 20


def test_thresholds_of_the_pair_rule(ctx):
    s = MC.synth(257, 257, 3)
    counts = {}
    for prm in [dict(max_dist=0), dict(max_dist=256), dict(ratio_pct=0), dict(max_dist=256, ratio_pct=0),
                dict(ratio_pct=100), dict(ratio_pct=1000000), dict(max_dist=20, ratio_pct=60)]:
        got, _ = _both(ctx, s["xyz"], s["pdesc"], s["kxy"], s["kdesc"], s["T"], s["K4"], s["size"], str(prm), **prm)
        counts[str(prm)] = got[4]
    print(counts)
    assert counts[str(dict(max_dist=256, ratio_pct=0))] > counts[str(dict(ratio_pct=0))] > 0


# ---------------------------------------------------------------- the rules' edges
def test_depth_and_frame_edges(ctx):
    """pz < 0, pz == 0, u exactly 0 (visible), u exactly w (not), v exactly h (not), a
    projection far outside, a NaN point."""
    xyz = np.vstack([_at([[10, 10]], -1.0), [[0.1, 0.1, 0.0]], _at([[0, 10], [64, 10], [10, 48], [10, 0], [1e6, 10]]),
                     [[np.nan, 0.0, 1.0]], _at([[63.999, 47.999]])])
    n = len(xyz)
    kxy = np.float32([[10, 10], [0, 10], [63.5, 10], [10, 47.5], [10, 0], [63.9, 47.9], [1, 11]])
    rng = np.random.default_rng(3)
    pdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kdesc = rng.integers(0, 256, (len(kxy), 32), dtype=np.uint8)
    got, want = _both(ctx, xyz, pdesc, kxy, kdesc, EYE, K64, (64, 48), "edges", max_dist=256, ratio_pct=0)
    idx, _, proj = got[:3]
    assert proj[0].tolist() == [-1, -1] and proj[1].tolist() == [-1, -1]      # behind, and on the camera plane
    assert proj[2].tolist() == [0, 10] and sorted(idx[2].tolist()) == [1, 6]  # u = 0 is inside
    assert proj[3].tolist() == [64, 10] and idx[3].tolist() == [-1, -1]       # u = w is not (a keypoint lies 0.5 px away)
    assert proj[4].tolist() == [10, 48] and idx[4].tolist() == [-1, -1]
    assert idx[5, 0] == 4 and idx[6].tolist() == [-1, -1] and idx[7].tolist() == [-1, -1]
    assert proj[7].tolist() == [-1, -1] and idx[8, 0] == 5   # 0 * NaN: pz is no number, and a NaN fails


def test_window_edge_is_included_and_the_next_float_is_not(ctx):
    up = np.nextafter(np.float32(14), np.float32(np.inf))
    down = np.nextafter(np.float32(6), np.float32(-np.inf))
    kxy = np.float32([[14, 10], [up, 10], [10, 14], [10, up], [6, 6], [down, 6], [np.nan, 10], [10, np.nan],
                      [-0.5, 10], [10, -1], [64, 10], [10, 48], [np.inf, 10]])
    xyz = _at([[10, 10]] * 3 + [[1, 14], [14, 2]])  # the last two: beside the unusable keypoints 8 and 9 alone
    rng = np.random.default_rng(4)
    kdesc = rng.integers(0, 256, (len(kxy), 32), dtype=np.uint8)
    pdesc = np.vstack([kdesc[1], kdesc[3], kdesc[5], kdesc[8], kdesc[9]])  # each its excluded neighbour's descriptor
    got, want = _both(ctx, xyz, pdesc, kxy, kdesc, EYE, K64, (64, 48), "window", max_dist=256, ratio_pct=0)
    assert want["ncand"].tolist() == [3, 3, 3, 0, 0]
    assert set(got[0][:3].ravel().tolist()) <= {0, 2, 4} and np.all(got[0][3:] == -1)
    # the same with a radius that is no integer, and one far past the frame
    for radius in (3.9999998, 4.0000005, 1e30):
        _both(ctx, xyz, pdesc, kxy, kdesc, EYE, K64, (64, 48), f"radius {radius}", radius=radius)


def test_257_keypoints_on_one_pixel(ctx):
    """One cell holds everything; ties go to the lowest keypoint, then the lowest point."""
    kxy = np.tile(np.float32([10.25, 7.5]), (257, 1))
    kdesc = np.zeros((257, 32), np.uint8)
    kdesc[:200, 0] = 0xFF
    kdesc[200:, 0] = 0x0F
    xyz = _at([[10, 7]] * 4)
    pdesc = np.zeros((4, 32), np.uint8)
    got, _ = _both(ctx, xyz, pdesc, kxy, kdesc, EYE, K64, (64, 48), "one pixel", ratio_pct=0)
    assert got[0].tolist() == [[200, 201]] * 4 and got[1].tolist() == [[4, 4]] * 4
    assert got[4] == 1 and got[3][0].tolist() == [200, 0]
    got, _ = _both(ctx, xyz, pdesc, kxy, kdesc, EYE, K64, (64, 48), "one pixel, ratio")
    assert got[4] == 0
    kdesc[:] = 0  # all equal: the best two are keypoints 0 and 1
    got, _ = _both(ctx, xyz, pdesc, kxy, kdesc, EYE, K64, (64, 48), "one pixel, equal", ratio_pct=0)
    assert got[0].tolist() == [[0, 1]] * 4 and got[3][0].tolist() == [0, 0]


def test_two_equal_bids_go_to_the_lowest_point(ctx):
    kxy = np.float32([[20, 20], [40, 30]])
    kdesc = np.zeros((2, 32), np.uint8)
    pdesc = np.zeros((5, 32), np.uint8)
    pdesc[:, 0] = [0x03, 0x01, 0x01, 0x07, 0x01]  # distances 2 1 1 3 1 to either keypoint
    xyz = _at([[21, 20], [19, 21], [20, 19], [40, 30], [41, 31]])
    got, _ = _both(ctx, xyz, pdesc, kxy, kdesc, EYE, K64, (64, 48), "bids")
    assert got[3][: got[4]].tolist() == [[0, 1], [1, 4]]


def test_a_window_over_the_frame_equals_match_hamming(ctx):
    """The existing brute-force kernel as a second witness."""
    s = MC.synth(257, 257, 3)
    rng = np.random.default_rng(9)
    kxy = (rng.uniform(0, 1, (257, 2)) * [63, 47]).astype(np.float32)      # every keypoint usable
    xyz = _at(rng.uniform(0, 1, (257, 2)) * [63, 47], rng.uniform(1, 9, 257))
    assert MP.project(xyz, EYE, K64, (64, 48))[1].all()
    bi, bd = ctx.match_hamming(s["pdesc"], s["kdesc"])
    for radius in (64.0, 1e9):
        idx, dist, _, _, _ = ctx.match_projected(xyz, s["pdesc"], kxy, s["kdesc"], EYE, K64, (64, 48),
                                                 S.ProjMatchParams(radius=radius))
        assert np.array_equal(idx, bi) and np.array_equal(dist, bd)


def test_a_quarter_wave_per_point_gives_the_same(ctx, monkeypatch):
    """Rule 5: nothing depends on how lanes share the work. SVO_PROJ_LANES=16 (the A/B
    hook of the launch shape) runs proj_match_kernel with 16 lanes per point."""
    monkeypatch.setenv("SVO_PROJ_LANES", "16")
    test_every_count_around_the_wave_and_the_block(ctx)
    test_32_problems_in_one_launch_leave_the_padding_alone(ctx)
    test_radius_40_on_320x240_spans_cells_and_the_border(ctx)
    test_depth_and_frame_edges(ctx)
    test_window_edge_is_included_and_the_next_float_is_not(ctx)
    test_257_keypoints_on_one_pixel(ctx)
    test_two_equal_bids_go_to_the_lowest_point(ctx)
    test_a_window_over_the_frame_equals_match_hamming(ctx)


# ---------------------------------------------------------------- the C ABI
def _raw(ctx, s, prm, idx=None, dist=None, proj=None, pairs=None, n_pairs=None, **over):
    a = dict(P=1, n_pts=np.array([len(s["xyz"])], np.int32), n_kp=np.array([len(s["kxy"])], np.int32),
             ps=len(s["xyz"]), ks=len(s["kxy"]), xyz=np.ascontiguousarray(s["xyz"]), pdesc=np.ascontiguousarray(s["pdesc"]),
             kxy=np.ascontiguousarray(s["kxy"]), kdesc=np.ascontiguousarray(s["kdesc"]), T=np.ascontiguousarray(s["T"]),
             K4=np.ascontiguousarray(s["K4"]), w=s["size"][0], h=s["size"][1], handle=ctx.handle,
             prm=ctypes.addressof(prm) if prm is not None else None)
    a.update(over)

    def ptr(x, t):
        return None if x is None else x.ctypes.data_as(ctypes.POINTER(t))

    return S.lib().svo_match_projected(
        a["handle"], a["P"], ptr(a["n_pts"], ctypes.c_int), ptr(a["n_kp"], ctypes.c_int), a["ps"], a["ks"],
        ptr(a["xyz"], ctypes.c_double), ptr(a["pdesc"], ctypes.c_uint8), ptr(a["kxy"], ctypes.c_float),
        ptr(a["kdesc"], ctypes.c_uint8), ptr(a["T"], ctypes.c_double), ptr(a["K4"], ctypes.c_double), a["w"], a["h"],
        a["prm"], ptr(idx, ctypes.c_int), ptr(dist, ctypes.c_int), ptr(proj, ctypes.c_float), ptr(pairs, ctypes.c_int),
        ptr(n_pairs, ctypes.c_int))


def _outs(s, fill=-9):
    n, m = len(s["xyz"]), len(s["kxy"])
    return dict(idx=np.full((n, 2), fill, np.int32), dist=np.full((n, 2), fill, np.int32),
                proj=np.full((n, 2), fill, np.float32), pairs=np.full((m, 2), fill, np.int32),
                n_pairs=np.full(1, fill, np.int32))


def test_optional_outputs_may_be_null(ctx):
    s, w = MC.synth(65, 255), MC.synth_want(65, 255)
    prm = S.ProjMatchParams()
    for keep in (["idx"], ["dist"], ["proj"], ["pairs", "n_pairs"], ["idx", "pairs", "n_pairs"], []):
        o = _outs(s)
        assert _raw(ctx, s, prm, **{k: o[k] for k in keep}) == 0, keep
        for k in keep:
            if k == "n_pairs":
                assert o[k][0] == len(w["pairs"])
            elif k == "pairs":
                assert np.array_equal(o[k][: len(w["pairs"])], w["pairs"]) and np.all(o[k][len(w["pairs"]):] == -9)
            else:
                assert np.array_equal(o[k].view(np.uint32), w[k].view(np.uint32)), k
    assert _raw(ctx, s, prm, P=0) == 0 and _raw(ctx, s, prm, P=0, n_pts=None, n_kp=None, xyz=None) == 0


def test_error_returns_write_nothing(ctx):
    s = MC.synth(65, 255)
    good = S.ProjMatchParams()
    bad_prm = [S.ProjMatchParams(radius=0), S.ProjMatchParams(radius=-1), S.ProjMatchParams(radius=float("nan")),
               S.ProjMatchParams(radius=float("inf")), S.ProjMatchParams(max_dist=-1), S.ProjMatchParams(max_dist=257),
               S.ProjMatchParams(ratio_pct=-1)]
    cases = [dict(prm=p) for p in bad_prm] + [
        dict(prm=good, handle=None), dict(prm=None), dict(prm=good, P=-1), dict(prm=good, P=65536),
        dict(prm=good, n_pts=np.array([-1], np.int32)), dict(prm=good, n_kp=np.array([-1], np.int32)),
        dict(prm=good, n_pts=np.array([66], np.int32)), dict(prm=good, n_kp=np.array([256], np.int32)),
        dict(prm=good, ps=-1), dict(prm=good, ks=(1 << 20) + 1), dict(prm=good, ps=(1 << 20) + 1),
        dict(prm=good, w=0), dict(prm=good, h=0), dict(prm=good, w=-5),
        dict(prm=good, n_pts=None), dict(prm=good, n_kp=None), dict(prm=good, xyz=None), dict(prm=good, pdesc=None),
        dict(prm=good, kxy=None), dict(prm=good, kdesc=None), dict(prm=good, T=None), dict(prm=good, K4=None)]
    for c in cases:
        o = _outs(s)
        prm = c.pop("prm")
        assert _raw(ctx, s, prm, **o, **c) == -1, c
        for k, v in o.items():
            assert np.all(v == -9), (c, k)
    o = _outs(s)
    assert _raw(ctx, s, good, pairs=o["pairs"]) == -1 and np.all(o["pairs"] == -9)  # pairs without n_pairs
    with pytest.raises(S.SvoError):
        ctx.match_projected(s["xyz"], s["pdesc"], s["kxy"], s["kdesc"], s["T"], s["K4"], s["size"],
                            S.ProjMatchParams(radius=0))
    ms = np.zeros(3)
    assert S.lib().svo_match_projected_time(ctx.handle, 0, None, None, 0, 0, None, None, None, None, None, None, 64, 48,
                                            ctypes.addressof(good), 0, ms.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    # the context still works
    _check(ctx.match_projected(s["xyz"], s["pdesc"], s["kxy"], s["kdesc"], s["T"], s["K4"], s["size"]),
           MC.synth_want(65, 255), "after the errors")
    t = ctx.match_projected_time(s["xyz"][None], s["pdesc"][None], s["kxy"][None], s["kdesc"][None], s["T"][None],
                                 s["K4"], s["size"], [65], [255], reps=2)
    assert t.shape == (3,) and np.all(t > 0)


# ---------------------------------------------------------------- the recorded scenes
@pytest.mark.parametrize("name", sorted(MC.MEASURED))
def test_scene_match_and_guided_relocalisation(ctx, name):
    d, want = MC.scene_inputs(name), MC.scene_want(name)
    # the whole map under the restatement's first pose: every output
    T = MP.pose12(d["first"]["rvec"], d["first"]["tvec"])
    full = _want(d["map_xyz"], d["map_desc"], d["kxy"], d["kdesc"], T, d["K"], d["size"])
    got = ctx.match_projected(d["map_xyz"], d["map_desc"], d["kxy"], d["kdesc"], T, d["K"], d["size"])
    _check(got, full, name)
    assert np.array_equal(full["pairs"], want["pairs"]) and got[4] == MC.MEASURED[name]["widened"][0]
    # the chain: relocalize, match_projected under its pose, solve_pnp_ransac
    rvec, tvec, inl_pairs, first = ctx.relocalize_guided(d["map_desc"], d["map_xyz"], d["kdesc"], d["kxy"], d["K"],
                                                         d["size"])
    assert np.array_equal(first[2], d["first"]["pairs"][d["first"]["inliers"]])
    np.testing.assert_allclose(first[0], d["first"]["rvec"], atol=1e-7)
    np.testing.assert_allclose(first[1], d["first"]["tvec"], atol=1e-6)
    assert np.array_equal(inl_pairs, want["pairs"][want["inliers"]])
    np.testing.assert_allclose(rvec, want["rvec"], atol=1e-7)
    np.testing.assert_allclose(tvec, want["tvec"], atol=1e-6)
    rot, trans = d["pose_error"](rvec, tvec)
    m = MC.MEASURED[name]
    print(f"{name}: first {len(d['first']['pairs'])} pairs, widened {got[4]} pairs / {len(inl_pairs)} inliers, "
          f"rot {rot:.4f} deg, |t| {trans:.4f} m")
    assert len(inl_pairs) == m["widened"][1]
    assert rot <= 2 * m["rot_deg"] and trans <= 2 * m["trans_m"]
    with pytest.raises(S.SvoError):  # too few first-pass matches is an error, as relocalize's
        ctx.relocalize_guided(d["map_desc"][:3], d["map_xyz"][:3], d["kdesc"][:3], d["kxy"][:3], d["K"], d["size"])
