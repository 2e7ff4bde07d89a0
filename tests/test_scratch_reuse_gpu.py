"""Results do not depend on what used the context before: the single-call entry
points that carve a context's scratch buffers (and those that used to share one)
run interleaved on ONE context at n = 1, then 300, then 37 points -- every buffer
grows once and is then reused at a smaller size -- with their optional outputs
asked for and left out, and every output must equal, bit for bit, the same call
made on a fresh context.

solve_pnp_ransac needs four points, so its n = 1 pass runs on four."""
import ctypes as C

import numpy as np
import pytest

import ba_reference as B
import pose_refine_reference as Q
import svo_amd as S
from svo_amd.scene import Scene

pytestmark = pytest.mark.gpu

W, H = 160, 120
SIZES = (1, 300, 37)


class Env:
    """A context and, made on first use, the images the image calls read: "a" and
    "b" two frames, "r" the right image of "a", "c" the one the BGR uploads fill."""

    def __init__(self, sc, grays):
        self.ctx, self.sc, self.grays, self._img = S.Context(0), sc, grays, {}

    def img(self, name):
        if name not in self._img:
            self._img[name] = self.ctx.image(self.grays[name], 3)
        return self._img[name]


def inputs(sc, n):
    """Everything the calls of one size read, from n alone."""
    rng = np.random.default_rng(1000 + n)
    d = {"n": n}
    d["pts"] = np.c_[rng.uniform(14, W - 14, n), rng.uniform(14, H - 14, n)].astype(np.float32)
    d["ages"] = rng.integers(0, 50, n).astype(np.int32)
    npnp = max(n, 4)
    px = np.c_[rng.uniform(5, W - 5, npnp), rng.uniform(5, H - 5, npnp)]
    d["obj"] = sc.map_points(px, 0)
    d["img1"] = (sc.project(d["obj"], 1) + rng.normal(0, 0.3, (npnp, 2))).astype(np.float32)
    d["hyps"] = np.array([np.r_[sc.R(t).ravel(), 0.01 * t, 0, 0] for t in (1, 2, 3)])
    X, xy, ur, T = Q.stereo_scene(n, 7 + n, noise=0.5, outliers=0.1)
    d["rs"] = (X[None], xy[None], ur[None], Q.start_pose(T, n, 0.3, 0.03)[None])
    d["prior"] = np.where(rng.random(n) < 0.3, S.STEREO_NO_PRIOR, rng.integers(0, 40, n)).astype(np.int32)
    d["mid"] = np.sort(rng.choice(4 * n + 8, n, replace=False)).astype(np.int32)
    d["prev_mid"] = np.sort(rng.choice(4 * n + 8, n, replace=False)).astype(np.int32)
    d["prev_xy"] = np.c_[rng.uniform(40, W, n), rng.uniform(0, H, n)].astype(np.float32)
    d["prev_ur"] = (d["prev_xy"][:, 0] - rng.uniform(0, 30, n)).astype(np.float32)
    d["bgr"] = [np.stack([sc.frame(t), sc.frame(t + 1), sc.frame(t + 2)], -1) for t in (2, 3, 4)]
    Xs, xys, _, _ = Q.stereo_scene(5 * n, 90 + n)
    d["subsets"] = np.c_[Xs.reshape(n, 15), xys.reshape(n, 10)].astype(np.float32)
    ids = np.stack([np.sort(rng.choice(2 * n + 2, n, replace=False)) for _ in range(2)])[None]
    d["lists"] = (np.array([[n, (n + 1) // 2]], np.int32), ids.astype(np.int32),
                  rng.uniform(0, W, (1, 2, n, 2)).astype(np.float32))
    d["ba"] = B.perturbed(B.window_scene(C=3, M=n, seed=n, drop=0.0, noise=0.3), n, n_fixed=1)
    return d


def pnp_residuals_bare(ctx, obj, img_pts, hyps, K):
    """svo_pnp_residuals with err, mask and counts all left out (the binding always asks for two)."""
    obj, img_pts = np.ascontiguousarray(obj, np.float32), np.ascontiguousarray(img_pts, np.float32)
    hyps, K = np.ascontiguousarray(hyps, np.float64), np.ascontiguousarray(K, np.float64).reshape(9)
    f32, f64 = C.POINTER(C.c_float), C.POINTER(C.c_double)
    return S.lib().svo_pnp_residuals(ctx.handle, obj.ctypes.data_as(f32), img_pts.ctypes.data_as(f32), len(obj),
                                     hyps.ctypes.data_as(f64), len(hyps), K.ctypes.data_as(f64), C.c_float(64.0),
                                     None, None, None)


def calls(d, opt):
    """(name, call) in the order they run: neighbours never share a buffer's old slot."""
    n = d["n"]
    X, xy, ur, T0 = d["rs"]
    cnt = np.array([(n + 1) // 2], np.int32) if opt else None
    q = d["ba"]

    def upload_then(what):
        def run(e):
            img = e.img("c")
            for bgr in d["bgr"]:  # three in a row: both ingest buffers, the first one again
                img.upload_bgr(bgr)
            return what(e), img.level(0), img.level(2)
        return run

    return [
        ("bucket_features", lambda e: e.ctx.bucket_features(d["pts"], W, H, 20, 2, ages=d["ages"] if opt else None)),
        ("lk", lambda e: e.ctx.calc_optical_flow_pyr_lk(e.img("a"), e.img("b"), d["pts"], want_err=opt)),
        ("upload_bgr+scharr", upload_then(lambda e: e.img("c").scharr(1))),
        ("solve_pnp_ransac", lambda e: e.ctx.solve_pnp_ransac(d["obj"], d["img1"], e.sc.K, iterations=60)),
        ("stereo_match_rows", lambda e: e.ctx.stereo_match_rows(e.img("a"), e.img("r"), d["pts"], want_cost=opt)),
        ("upload_bgr+epnp_subsets", upload_then(lambda e: e.ctx.epnp_subsets(d["subsets"], B.K, device=1))),
        ("refine_poses", lambda e: e.ctx.refine_poses(X, xy, T0, B.K, counts=cnt, max_iterations=5)),
        ("stereo_match_rows_guided", lambda e: e.ctx.stereo_match_rows_guided(e.img("a"), e.img("r"), d["pts"],
                                                                              d["prior"], 4, want_cost=opt)),
        ("upload_bgr+ba_stage_lists", upload_then(lambda e: e.ctx.ba_stage_lists(*d["lists"]))),
        ("stereo_row_priors", lambda e: e.ctx.stereo_row_priors(d["mid"], d["prev_mid"], d["prev_xy"], d["prev_ur"])),
        ("pnp_residuals", lambda e: (e.ctx.pnp_residuals(d["obj"], d["img1"], d["hyps"], e.sc.K, want_err=True)
                                     if opt else pnp_residuals_bare(e.ctx, d["obj"], d["img1"], d["hyps"], e.sc.K))),
        ("bundle_adjust", lambda e: e.ctx.bundle_adjust(q["poses"], q["fixed"], q["points"], q["obs_cam"],
                                                        q["obs_point"], q["obs_xy"], B.K, max_iterations=4)),
        ("refine_poses_stereo", lambda e: e.ctx.refine_poses_stereo(X, xy, ur, T0, B.K, Q.BASELINE, counts=cnt,
                                                                    max_iterations=5)),
        ("pnp_residuals_counts", lambda e: e.ctx.pnp_residuals(d["obj"], d["img1"], d["hyps"], e.sc.K,
                                                               want_err=not opt)),
    ]


def flat(out):
    """The bytes of every array (and the value of every scalar) of a call's result."""
    if isinstance(out, dict):
        return [(k, x) for key in sorted(out) for k, x in flat(out[key])]
    if isinstance(out, (tuple, list)):
        return [(k, x) for o in out for k, x in flat(o)]
    if out is None:
        return [("none", b"")]
    a = np.ascontiguousarray(out)
    return [(f"{a.dtype}{a.shape}", a.tobytes())]


def test_results_do_not_depend_on_the_contexts_history():
    sc = Scene(W, H, seed=5)
    grays = {"a": sc.frame(0), "b": sc.frame(1), "r": sc.right(0), "c": sc.frame(0)}
    passes = [(inputs(sc, n), opt) for n in SIZES for opt in (True, False)]
    want = {}
    for d, opt in passes:  # every call on a context (and images) of its own
        for name, call in calls(d, opt):
            e = Env(sc, grays)
            want[d["n"], opt, name] = flat(call(e))
            e.ctx.close()
    shared = Env(sc, grays)
    differ = []
    for d, opt in passes:
        for name, call in calls(d, opt):
            got = flat(call(shared))
            if got != want[d["n"], opt, name]:
                differ.append((d["n"], opt, name))
    assert not differ, f"(n, optional outputs, call) that differ from a fresh context: {differ}"
