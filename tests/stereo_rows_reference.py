"""Row SAD restated in numpy (TEST INFRASTRUCTURE): the rule of
svo_stereo_match_rows (include/svo_gpu.h) step by step, in
integers up to the sub-pixel step and in float32 from there, so the device's
outputs are compared bit for bit. Also the scene and the oracle loop the
matcher's tests share: a rig at KITTI's own fx * b and the reference loop with
the row search in findLeftFeaturesInRight's place.
"""
from __future__ import annotations

import numpy as np

import oracle as O
from oracle_loop import Y_THRESHOLD, OracleLoop, transform
from svo_amd.scene import Scene, SceneForward

PAD = 32  # kPyrPad: the REFLECT_101 border every level is stored with
KITTI_BF = 386.1448  # KITTI's fx * b (P1[0, 3]); svo_amd.scene.STEREO_BF is a quarter of it
DEFAULTS = dict(radius=5, d_min=-1, d_max=128, uniq_pct=80, max_cost=0)


def params_ok(radius=5, d_min=-1, d_max=128, uniq_pct=80, max_cost=0):
    span = d_max - d_min + 1
    return (1 <= radius <= 7 and d_min >= -16 and d_max <= 255 and 3 <= span <= 256 and 0 <= uniq_pct <= 100
            and max_cost >= 0)


def match_rows(left, right, pts, radius=5, d_min=-1, d_max=128, uniq_pct=80, max_cost=0):
    """-> next_xy (n, 2) float32, status (n,) uint8, disparity (n,) int32, cost (n,) int32."""
    if not params_ok(radius, d_min, d_max, uniq_pct, max_cost):
        raise ValueError("row SAD parameters out of range")
    left = np.ascontiguousarray(left, np.uint8)
    right = np.ascontiguousarray(right, np.uint8)
    assert left.shape == right.shape
    h, w = left.shape
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    r, side = radius, 2 * radius + 1
    Lp = np.pad(left, PAD, mode="reflect").astype(np.int32)
    Rp = np.pad(right, PAD, mode="reflect").astype(np.int32)
    nxt = pts.copy()
    status = np.zeros(n, np.uint8)
    disp = np.zeros(n, np.int32)
    cost = np.zeros(n, np.int32)
    for k in range(n):
        x, y = pts[k]
        # 1. cvRound, half to even; the range test on the rounded floats
        rx, ry = np.rint(x), np.rint(y)
        if not (0 <= rx <= w - 1 and 0 <= ry <= h - 1):
            continue
        xi, yi = int(rx), int(ry)
        # 2. the candidates keep the right centre inside the image
        dlo, dhi = max(d_min, xi - (w - 1)), min(d_max, xi)
        ncand = dhi - dlo + 1
        if ncand < 3:
            continue
        # 3. the integer costs
        patch = Lp[PAD + yi - r: PAD + yi + r + 1, PAD + xi - r: PAD + xi + r + 1]
        strip = Rp[PAD + yi - r: PAD + yi + r + 1, PAD + xi - dhi - r: PAD + xi - dlo + r + 1]
        win = np.lib.stride_tricks.sliding_window_view(strip, (side, side))[0]  # [column start]
        c = np.abs(win - patch).sum(axis=(1, 2))[::-1]  # c[j]: disparity dlo + j
        # 4. the smallest d of minimal cost (argmin takes the first); no bracket at the ends
        j = int(np.argmin(c))
        if j == 0 or j == ncand - 1:
            continue
        c0 = int(c[j])
        # 5.
        if max_cost > 0 and c0 > max_cost:
            continue
        # 6. uniqueness, on integers
        if uniq_pct > 0:
            others = np.r_[c[: max(j - 1, 0)], c[j + 2:]]
            if len(others) and not (c0 * 100 < uniq_pct * int(others.min())):
                continue
        # 7. the parabola through the three costs, float32 operation by operation
        cm, cp = int(c[j - 1]), int(c[j + 1])
        den = cm + cp - 2 * c0
        assert den >= 0
        delta = np.float32(0) if den == 0 else np.float32(cm - cp) / np.float32(2 * den)
        d = dlo + j
        nxt[k, 0] = np.float32(x) - (np.float32(d) + delta)
        status[k], disp[k], cost[k] = 1, d, c0
    return nxt, status, disp, cost


class KittiBfMixin:
    """A scene whose right view and projections default to KITTI's own fx * b."""
    bf = KITTI_BF

    def right(self, t, bf=None):
        return super().right(t, self.bf if bf is None else bf)

    def projections(self, bf=None):
        return super().projections(self.bf if bf is None else bf)


class WideScene(KittiBfMixin, Scene):
    pass


class WideSceneForward(KittiBfMixin, SceneForward):
    def __init__(self, w, h, seed=0, bf=None, **kw):
        super().__init__(w, h, seed=seed, **kw)
        if bf is not None:
            self.bf = bf


class RowsOracleLoop(OracleLoop):
    """The oracle loop with row SAD in findLeftFeaturesInRight's place."""

    def __init__(self, scene, n_features=2000, rows=None, **kw):
        super().__init__(scene, n_features, **kw)
        self.rows = dict(DEFAULTS, **(rows or {}))
        self.trace = {}

    def _keyframe(self, left, right, cand, T, t):
        new = np.ascontiguousarray(cand, np.float32)
        if len(new) == 0:
            self.trace = dict(right=new.reshape(0, 2), status=np.zeros(0, np.uint8), ur=np.zeros(0, np.float32))
            return new.reshape(0, 2), np.zeros((0, 3))
        nr, st, _, _ = match_rows(left, right, new, **self.rows)
        keep = (st == 1) & (np.abs(nr[:, 1] - new[:, 1]) < Y_THRESHOLD)
        newL, newR = new[keep], nr[keep]
        _, xyz = O.triangulate(self.P_left, self.P_right, newL, newR)
        front = xyz[:, 2] > 0
        self.trace = dict(right=nr, status=st, ur=newR[front, 0])
        return newL[front], transform(T, t, xyz[front])
