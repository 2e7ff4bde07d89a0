"""The batched ORB detector (orb_batch_detect: its own workspace layout, batched
resize and Harris kernels, per-level strides of the keypoint readback, host
selection per sequence) off the reference's defaults, inside the front end:
other scale factors, level counts, edge thresholds and FAST thresholds, Harris
and FAST scoring, every step against the oracle loop with the same ORB
parameters (test_frontend_orb_matches_oracle_loop runs the defaults)."""
import numpy as np
import pytest

import svo_amd as S
from oracle_loop import OracleLoop
from svo_amd.scene import SceneForward
from test_frontend_gpu import make_frontend

pytestmark = pytest.mark.gpu

SEEDS = (3, 8)
T = 7
CONFIGS = {
    # id: W, H, N, features_to_track, ORB parameters
    "A": (320, 240, 1024, 200, dict(nfeatures=300, scale_factor=1.5, nlevels=4, edge_threshold=8, patch_size=8,
                                    fast_threshold=10, harris=True)),
    "B": (240, 160, 512, 120, dict(nfeatures=200, scale_factor=1.35, nlevels=5, edge_threshold=6, patch_size=6,
                                   fast_threshold=12, harris=False)),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_frontend_orb_off_defaults_matches_oracle_loop(cfg):
    W, H, N, F, orb = CONFIGS[cfg]
    prm = S.OrbParams(nfeatures=orb["nfeatures"], scale_factor=orb["scale_factor"], nlevels=orb["nlevels"],
                      patch_size=orb["patch_size"], fast_threshold=orb["fast_threshold"],
                      edge_threshold=orb["edge_threshold"],
                      score_type=S.OrbParams.HARRIS if orb["harris"] else S.OrbParams.FAST)
    ctx = S.Context(0)
    fe = make_frontend(ctx, [SceneForward(W, H, seed=sd) for sd in SEEDS], T, N, use_orb=1, orb=prm,
                       keyframe_rule=S.KF_REFERENCE, features_to_track=F)
    fe.init(0)
    refs = [OracleLoop(SceneForward(W, H, seed=sd), N, rule="reference", features_to_track=F, detector="orb",
                       orb=dict(orb)).init(0) for sd in SEEDS]
    for q, ref in enumerate(refs):
        assert len(ref.pts) > 0
        assert np.array_equal(fe.features(q), ref.pts), f"seq {q} features at init"
    kf = np.zeros((T, len(SEEDS)), int)  # the oracle loop's keyframes [t][sequence]
    for t in range(1, T):
        st = fe.step(t).as_dict()
        rss = [r.step(t) for r in refs]
        kf[t] = [rs["keyframe"] for rs in rss]
        for k in ("tracked", "inliers", "added", "features"):
            assert st[k] == sum(rs[k] for rs in rss), f"{k} at t={t}"
        assert st["keyframes"] == kf[t].sum(), f"keyframes at t={t}"
        assert st["kf_overflow"] == 0
        for q, ref in enumerate(refs):
            assert np.array_equal(fe.features(q), ref.pts), f"seq {q} features at t={t}"
            rv, tv = fe.pose(q)
            np.testing.assert_allclose(rv, ref.pose[0], atol=1e-7)
            np.testing.assert_allclose(tv, ref.pose[1], atol=1e-6)
    # what the configuration is there for (properties of the oracle loop)
    if cfg == "A":
        assert (kf.sum(axis=0) >= 1).all(), f"every sequence a keyframe after init: {kf.tolist()}"
        assert kf[2].sum() == 1, "step 2: a keyframe and a tracking-only sequence in one batch"
    else:
        assert kf[[2, 4, 6], 0].all(), f"seed 3: keyframes at steps 2, 4 and 6: {kf.tolist()}"
