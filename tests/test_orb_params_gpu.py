"""svo_orb_detect off the reference's defaults (tests/orb_param_cases.py): other
scale factors (1.05, 1.5, an exact 2.0, 3.0 with skipped source pixels), level
counts, edge thresholds down to the supported 4 (keypoints on the outermost
columns and rows the border filter admits, Harris windows touching the level's
edge), FAST thresholds at and beyond 0 and 255, quotas of 0, binding prefilters,
levels too small for FAST, masks with values other than 0 and 255, and images
without a corner. Two comparisons per case, both bit for bit against the oracle:
the detection (count, octaves, x, y, response, order) and every level of the
scale and mask pyramids (svo_orb_level: the pyramid code svo_orb_detect runs)
against the chain of oracle resizes.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O  # noqa: F401  (the cases module computes with it)
import orb_param_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import svo_amd as S
    return S.Context(0)


def _orb_params(cid):
    import svo_amd as S
    p = P.params(cid)
    return S.OrbParams(nfeatures=p["nfeatures"], scale_factor=p["scale"], nlevels=p["nlevels"],
                       patch_size=p["patch"], fast_threshold=p["thr"], edge_threshold=p["edge"],
                       score_type=S.OrbParams.HARRIS if p["harris"] else S.OrbParams.FAST)


@pytest.mark.parametrize("cid", list(P.CASES))
def test_gpu_orb_detect_matches_oracle_off_defaults(ctx, cid):
    P.check_reaches_target(cid)
    img, mask = P.inputs(cid)
    ek, eo = P.oracle_detect(cid)
    gk, go = ctx.orb_detect(ctx.image(img, max_levels=0), _orb_params(cid), mask)
    assert len(gk) == len(ek)
    assert np.array_equal(go, eo)
    assert np.array_equal(gk.view(np.uint32), ek.view(np.uint32))  # x, y, response bit for bit, same order


@pytest.mark.parametrize("cid", list(P.CASES))
def test_gpu_orb_levels_match_oracle_resize_chain(ctx, cid):
    img, mask = P.inputs(cid)
    lw, lh, _, _ = P.level_info(cid)
    lv, mk = P.oracle_levels(cid)
    g = ctx.image(img, max_levels=0)
    prm = _orb_params(cid)
    for l in range(len(lw)):
        gi, gm = ctx.orb_level(g, prm, mask, l)
        assert gi.shape == (lh[l], lw[l]), f"level {l} size"
        bad = np.argwhere(gi != lv[l])
        assert len(bad) == 0, f"level {l}: {len(bad)} pixels differ, first (y, x) = {bad[0]}"
        if mask is None:
            assert gm is None
        else:
            bad = np.argwhere(gm != mk[l])
            assert len(bad) == 0, f"mask level {l}: {len(bad)} pixels differ, first (y, x) = {bad[0]}"


def test_gpu_orb_truncates_at_cap(ctx):
    import svo_amd as S
    img, _ = P.inputs("base")
    ek, eo = P.oracle_detect("base")
    assert len(ek) > 16
    g = ctx.image(img, max_levels=0)
    prm = _orb_params("base")
    gk, go = ctx.orb_detect(g, prm, cap=10)
    assert np.array_equal(gk.view(np.uint32), ek[:10].view(np.uint32)) and np.array_equal(go, eo[:10])
    # the raw entry: n_out is the untruncated total, nothing past `cap` rows is written
    out = np.full((16, 3), -7.25, np.float32)
    octv = np.full(16, -77, np.int32)
    n = C.c_int(-1)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int)
    rc = S.lib().svo_orb_detect(ctx.handle, g.handle, C.byref(prm), None, out.ctypes.data_as(f32p),
                                octv.ctypes.data_as(i32p), 10, C.byref(n))
    assert rc == 0
    assert n.value == len(ek)
    assert np.array_equal(out[:10].view(np.uint32), ek[:10].view(np.uint32)) and np.array_equal(octv[:10], eo[:10])
    assert (out[10:] == -7.25).all() and (octv[10:] == -77).all()
