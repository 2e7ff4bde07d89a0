"""svo_orb_compute, svo_orb_detect_and_compute and svo_orb_blur_level on the GPU
against the numpy restatement (tests/orb_describe_reference.py, the rules of
DESIGN.md section 3d): blurred levels, descriptors and validity bit for bit, the
reported angle to 1e-3 degree; hand-placed keypoints at the validity border, on a
constant patch and in counts around one wave; the quarter-turn property on the
device; and relocalisation of a rotated frame against a described map, equal to
the same chain on the restatement's descriptors.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import orb_describe_cases as K
import orb_describe_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import svo_amd as S
    return S.Context(0)


def _angles_close(a, b):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return np.minimum(d, 360.0 - d).max(initial=0.0) < 1e-3


@pytest.mark.parametrize("name,pid", K.CASES)
def test_gpu_blur_levels_match_restatement(ctx, name, pid):
    img = K.image(name)
    g = ctx.image(img, max_levels=0)
    prm = K.orb_params(pid)
    lv, bl, _ = K.pyramid(name, prm.nlevels)
    for l in range(prm.nlevels):
        got = ctx.orb_blur_level(g, prm, l)
        assert got.shape == lv[l].shape, f"level {l} size"
        bad = np.argwhere(got != bl[l])
        assert len(bad) == 0, f"level {l}: {len(bad)} pixels differ, first (y, x) = {bad[0]}"


@pytest.mark.parametrize("w,h,scale,nlevels", [(24, 20, 1.2, 8), (40, 2, 1.5, 3), (70, 5, 1.2, 4), (130, 17, 2.0, 3)])
def test_gpu_blur_levels_narrower_than_the_kernel(ctx, w, h, scale, nlevels):
    """Levels with fewer rows than the kernel has taps, down to one pixel (three rows
    and fewer: REFLECT_101 reflected more than once), tiles cut on both sides, more
    than one tile across; and no keypoint is valid on a level smaller than the
    patch's reach."""
    import svo_amd as S
    rng = np.random.default_rng(w * h)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    prm = S.OrbParams(scale_factor=scale, nlevels=nlevels, wta_k=2)
    lv, ls = R.levels_of(img, scale, nlevels)
    assert min(min(a.shape) for a in lv) < 7
    g = ctx.image(img, max_levels=0)
    for l in range(nlevels):
        got = ctx.orb_blur_level(g, prm, l)
        assert got.shape == lv[l].shape and np.array_equal(got, R.blur(lv[l])), l
    kp = np.array([[w // 2, h // 2]] * nlevels, np.float32)
    desc, angle, valid = ctx.orb_compute(g, kp, np.arange(nlevels), prm)
    assert not valid.any() and not desc.any() and (angle == -1).all()


@pytest.mark.parametrize("corners", [False, True], ids=["default_pattern", "corner_pattern"])
@pytest.mark.parametrize("name,pid", K.CASES)
def test_gpu_compute_matches_restatement(ctx, name, pid, corners):
    img = K.image(name)
    prm = K.orb_params(pid)
    ek, eo = K.oracle_detect(name, pid)
    # the input reaches what the case is for: keypoints on every octave it can have
    counts = np.bincount(eo, minlength=prm.nlevels)
    assert (counts[: K.OCTAVES[(name, pid)]] > 0).all(), counts
    g = ctx.image(img, max_levels=0)
    gk, go = ctx.orb_detect(g, prm)
    # detection is what it was: the oracle's keypoints bit for bit, same order
    assert np.array_equal(go, eo) and np.array_equal(gk.view(np.uint32), ek.view(np.uint32))
    pat = K.corner_pattern(prm.patch_size) if corners else None
    if corners:
        hp = prm.patch_size // 2
        assert {(hp, hp), (-hp, -hp), (-hp, hp), (hp, -hp)} <= {tuple(p) for p in pat.tolist()}
    desc, angle, valid = ctx.orb_compute(g, gk, go, prm, pat)
    ed, ea, ev = K.reference(name, pid, corners)
    assert ev.all() and len(ed) > 0
    assert np.array_equal(valid, ev.astype(bool))
    bad = np.argwhere((desc != ed).any(axis=1)).ravel()
    assert len(bad) == 0, f"{len(bad)} of {len(ed)} descriptors differ, first: keypoint {bad[0]} octave {go[bad[0]]}"
    assert _angles_close(angle, ea)
    # the explicit default pattern is the NULL pattern
    if not corners:
        import svo_amd as S
        d2, _, _ = ctx.orb_compute(g, gk, go, prm, S.orb_default_pattern(prm.patch_size))
        assert np.array_equal(d2, desc)


@pytest.mark.parametrize("name,pid", [("big", "def"), ("crop", "p15")])
def test_gpu_detect_and_compute_is_detect_then_compute(ctx, name, pid):
    img = K.image(name)
    prm = K.orb_params(pid)
    g = ctx.image(img, max_levels=0)
    gk, go = ctx.orb_detect(g, prm)
    desc, angle, valid = ctx.orb_compute(g, gk, go, prm)
    k2, o2, d2, a2, v2 = ctx.orb_detect_and_compute(g, prm)
    assert np.array_equal(k2.view(np.uint32), gk.view(np.uint32)) and np.array_equal(o2, go)
    assert np.array_equal(d2, desc) and np.array_equal(v2, valid)
    assert np.array_equal(a2.view(np.uint32), angle.view(np.uint32))
    # with a mask, and truncated at cap: n_out is svo_orb_detect's total
    mask = np.full(img.shape, 255, np.uint8)
    mask[:, : img.shape[1] // 2] = 0
    mk, mo = ctx.orb_detect(g, prm, mask)
    assert 0 < len(mk) < len(gk)
    k3, o3, d3, _, v3 = ctx.orb_detect_and_compute(g, prm, mask, cap=7)
    assert np.array_equal(k3.view(np.uint32), mk[:7].view(np.uint32)) and np.array_equal(o3, mo[:7])
    md, _, mv = ctx.orb_compute(g, mk[:7], mo[:7], prm)
    assert np.array_equal(d3, md) and np.array_equal(v3, mv)


def test_gpu_hand_placed_keypoints(ctx):
    img = K.image("big").copy()
    img[100:160, 200:260] = 131  # a constant patch around (230, 130)
    prm = K.orb_params("def")
    lv, ls = R.levels_of(img, 1.2, 8)
    bl = [R.blur(a) for a in lv]
    rch = R.reach(31)
    assert rch == 21
    g = ctx.image(img, max_levels=0)
    rows = []  # (x, y, octave): level pixels scaled back to level 0, as svo_orb_detect reports them
    for l in (0, 2, 5):
        lh, lw = lv[l].shape
        for cx, cy in ((rch, rch + 3), (lw - 1 - rch, lh - 1 - rch), (rch - 1, rch + 3), (lw - rch, rch + 3),
                       (rch + 5, rch - 1), (rch + 5, lh - rch)):
            rows.append((np.float32(cx) * ls[l], np.float32(cy) * ls[l], l))
    rows.append((230.0, 130.0, 0))
    kp = np.array([r[:2] for r in rows], np.float32)
    octv = np.array([r[2] for r in rows], np.int32)
    desc, angle, valid = ctx.orb_compute(g, kp, octv, prm)
    ed, ea, ev = R.compute(lv, bl, ls, kp, octv, 31)
    assert ev.tolist() == [1, 1, 0, 0, 0, 0] * 3 + [1]  # the border cases are what they are meant to be
    assert np.array_equal(valid, ev.astype(bool))
    assert np.array_equal(desc, ed)
    assert not desc[~valid].any() and (angle[~valid] == -1).all()
    assert _angles_close(angle, ea)
    # the constant patch: c = 1, s = 0, angle 0; the descriptor is the unsteered pattern's
    assert R.moments(img, 230, 130, 31) == (0, 0) and angle[-1] == 0
    # counts around one wave and one block; n = 0
    ek, eo = K.oracle_detect("big", "def")
    rd, ra, rv = R.compute(lv, bl, ls, ek[:, :2], eo, 31)
    for n in (0, 1, 3, 4, 5, 64, 65):
        d, a, v = ctx.orb_compute(g, ek[:n], eo[:n], prm)
        assert d.shape == (n, 32) and np.array_equal(d, rd[:n]) and np.array_equal(v, rv[:n].astype(bool)), n
        assert _angles_close(a, ra[:n])


def test_gpu_argument_errors_write_nothing(ctx):
    import svo_amd as S
    img = K.image("crop")
    g = ctx.image(img, max_levels=0)
    kp = np.array([[60.0, 60.0, 0.0]], np.float32)
    octv = np.zeros(1, np.int32)
    u8p, f32p, i32p, i8p = (C.POINTER(t) for t in (C.c_uint8, C.c_float, C.c_int, C.c_int8))

    def call(prm, pattern=None, octave=octv, n=1):
        desc = np.full((1, 32), 0xA5, np.uint8)
        ang = np.full(1, -7.5, np.float32)
        val = np.full(1, 9, np.uint8)
        rc = S.lib().svo_orb_compute(ctx.handle, g.handle, C.byref(prm), None if pattern is None
                                     else pattern.ctypes.data_as(i8p), kp.ctypes.data_as(f32p),
                                     octave.ctypes.data_as(i32p), n, desc.ctypes.data_as(u8p),
                                     ang.ctypes.data_as(f32p), val.ctypes.data_as(u8p))
        untouched = (desc == 0xA5).all() and ang[0] == -7.5 and val[0] == 9
        return rc, untouched

    assert call(S.OrbParams(nlevels=2, wta_k=2))[0] == 0
    for bad in (S.OrbParams(nlevels=2, wta_k=4), S.OrbParams(nlevels=2, wta_k=3),
                S.OrbParams(nlevels=2, wta_k=2, patch_size=30, edge_threshold=31),
                S.OrbParams(nlevels=2, wta_k=2, patch_size=33, edge_threshold=31),
                S.OrbParams(nlevels=2, wta_k=2, patch_size=3, edge_threshold=31)):
        assert call(bad) == (-1, True)
    fl = S.OrbParams(nlevels=2, wta_k=2)
    fl.first_level = 1
    assert call(fl) == (-1, True)
    pat = S.orb_default_pattern(15)
    p15 = S.OrbParams(nlevels=2, wta_k=2, patch_size=15, edge_threshold=15)
    assert call(p15, pat)[0] == 0
    pat[100, 1] = 8  # hp = 7
    assert call(p15, pat) == (-1, True)
    assert call(S.OrbParams(nlevels=2, wta_k=2), octave=np.array([2], np.int32)) == (-1, True)
    assert call(S.OrbParams(nlevels=2, wta_k=2), octave=np.array([-1], np.int32)) == (-1, True)
    assert call(S.OrbParams(nlevels=2, wta_k=2), n=-1) == (-1, True)
    assert call(S.OrbParams(nlevels=2, wta_k=2), n=0) == (0, True)
    with pytest.raises(S.SvoError):
        ctx.orb_detect_and_compute(g, S.OrbParams(nlevels=2))  # the reference's WTA_K 4
    with pytest.raises(S.SvoError):
        ctx.orb_blur_level(g, S.OrbParams(nlevels=2, wta_k=2), 2)


def test_gpu_descriptor_turns_with_the_image(ctx):
    """The quarter-turn property of tests/test_orb_describe_cpu.py, on the device,
    at level 0: np.rot90 sends pixel (x, y) of a w-wide image to (y, w - 1 - x)."""
    img = K.image("big")
    h, w = img.shape
    rot = np.rot90(img).copy()
    prm = K.orb_params("nl3")
    ek, eo = K.oracle_detect("big", "nl3")
    kp = ek[eo == 0][:, :2]
    assert len(kp) > 20 and (kp == np.rint(kp)).all()
    kr = np.stack([kp[:, 1], w - 1 - kp[:, 0]], axis=1)
    z = np.zeros(len(kp), np.int32)
    d0, a0, v0 = ctx.orb_compute(ctx.image(img, max_levels=0), kp, z, prm)
    d1, a1, v1 = ctx.orb_compute(ctx.image(rot, max_levels=0), kr, z, prm)
    assert v0.all() and v1.all()
    assert np.array_equal(d0, d1)
    assert np.abs((a0.astype(np.float64) - a1) % 360.0 - 90.0).max() < 1e-3


def test_gpu_relocalize_matches_restatement_chain(ctx):
    d = K.reloc_inputs()
    sc, t = d["scene"], K.RELOC["t"]
    import svo_amd as S
    prm = S.OrbParams(nfeatures=K.RELOC["nfeatures"], wta_k=2)
    frames = {}
    for key in ("map", "cur"):
        kp, octv, desc, _, valid = ctx.orb_detect_and_compute(ctx.image(d[key]["img"], max_levels=0), prm)
        assert np.array_equal(kp.view(np.uint32), d[key]["kp"].view(np.uint32)) and np.array_equal(octv, d[key]["octave"])
        assert valid.all() and np.array_equal(desc, d[key]["desc"])
        frames[key] = (kp, desc)
    (mk, md), (ck, cd) = frames["map"], frames["cur"]
    xyz = sc.map_points(mk[:, :2], 0)
    rvec, tvec, pairs = ctx.relocalize(md, xyz, cd, ck, sc.K)
    # the same chain on the restatement's descriptors: same inputs, the same bits
    ref_pairs = K.reloc_pairs()
    assert len(ref_pairs) >= 30
    ok, rr, rt, inl = ctx.solve_pnp_ransac(d["xyz"][ref_pairs[:, 1]], d["cur"]["kp"][ref_pairs[:, 0], :2], sc.K)
    assert ok
    assert np.array_equal(pairs, ref_pairs[inl])
    assert np.array_equal(rvec.view(np.uint64), rr.view(np.uint64)) and np.array_equal(tvec.view(np.uint64), rt.view(np.uint64))
    # the rule itself: within twice what the restatement's chain reaches on the CPU
    rot, trans = K.pose_error(sc, t, rvec, tvec)
    share = K.match_share(sc, t, xyz, ck[:, :2], ref_pairs)
    print(f"relocalize: {len(ref_pairs)} pairs, {len(pairs)} inliers, share {share:.4f}, rot {rot:.4f} deg, |t| {trans:.4f} m")
    assert rot <= 2 * K.RELOC_MEASURED["rot_deg"] and trans <= 2 * K.RELOC_MEASURED["trans_m"]
    assert share >= 0.9 * K.RELOC_MEASURED["share"]
    # too few matches is an error, not a pose
    with pytest.raises(S.SvoError):
        ctx.relocalize(md[:3], xyz[:3], cd[:3], ck[:3], sc.K, ratio_pct=0, cross_check=False)
