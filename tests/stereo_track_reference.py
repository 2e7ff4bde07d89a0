"""Stereo columns for tracked features restated in numpy (TEST INFRASTRUCTURE):
the rules of svo_stereo_match_rows_guided, svo_stereo_row_priors and
svo_frontend_set_stereo_tracking (include/svo_gpu.h) on top
of tests/stereo_rows_reference.py, so the device's outputs are compared bit for
bit; and the oracle loops that record the window's right columns per frame."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import oracle as O
from oracle_loop import STEREO, Y_THRESHOLD, OracleLoop, transform
from stereo_rows_reference import (DEFAULTS, RowsOracleLoop, WideScene, WideSceneForward, match_rows,
                                   params_ok)

NO_PRIOR = -(2 ** 31)  # SVO_STEREO_NO_PRIOR
GUIDE_MAX = 15


def guided_range(d_min, d_max, prior, guide):
    """Point's [d_min_i, d_max_i] in Python's unbounded ints (no overflow to speak of)."""
    prior = int(prior)
    if prior == NO_PRIOR:
        return d_min, d_max
    return max(d_min, prior - guide), min(d_max, prior + guide)


def match_rows_guided(left, right, pts, d_prior=None, guide=4, radius=5, d_min=-1, d_max=128, uniq_pct=80,
                      max_cost=0):
    """match_rows applied per point with that point's range -> match_rows' outputs."""
    if not params_ok(radius, d_min, d_max, uniq_pct, max_cost) or not 0 <= guide <= GUIDE_MAX:
        raise ValueError("guided row SAD parameters out of range")
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    if d_prior is None or guide == 0:
        return match_rows(left, right, pts, radius, d_min, d_max, uniq_pct, max_cost)
    d_prior = np.asarray(d_prior).reshape(-1)
    assert len(d_prior) == len(pts)
    n = len(pts)
    nxt, status = pts.copy(), np.zeros(n, np.uint8)
    disp, cost = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for k in range(n):
        lo, hi = guided_range(d_min, d_max, d_prior[k], guide)
        if hi - lo + 1 < 3:  # step 2 finds fewer than 3 candidates whatever the image leaves
            continue
        a, s, d, c = match_rows(left, right, pts[k: k + 1], radius, lo, hi, uniq_pct, max_cost)
        nxt[k], status[k], disp[k], cost[k] = a[0], s[0], d[0], c[0]
    return nxt, status, disp, cost


def row_priors(mid, prev_mid, prev_xy, prev_ur):
    """svo_stereo_row_priors -> (n,) int64 (NO_PRIOR where there is none)."""
    mid = np.asarray(mid, np.int64).reshape(-1)
    prev_mid = np.asarray(prev_mid, np.int64).reshape(-1)
    prev_xy = np.asarray(prev_xy, np.float32).reshape(-1, 2)
    prev_ur = np.asarray(prev_ur, np.float32).reshape(-1)
    out = np.full(len(mid), NO_PRIOR, np.int64)
    if len(prev_mid) == 0:
        return out
    assert np.all(np.diff(prev_mid) > 0)
    j = np.searchsorted(prev_mid, mid)
    for i, q in enumerate(j):
        if q >= len(prev_mid) or prev_mid[q] != mid[i] or not prev_ur[q] >= 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.rint(np.float32(prev_xy[q, 0]) - np.float32(prev_ur[q]))  # float32, half to even
        if np.isfinite(d) and -32767 <= d <= 32767:
            out[i] = int(d)
    return out


class TrackedMixin:
    """An oracle loop that also keeps, per frame, the window's right columns by
    svo_frontend_set_stereo_tracking's rule: `ur` beside pts / mid. The base loop
    supplies new_ur(), the columns of the features the frame created.
    track: the guided match's parameters; guide 0: the full range for every feature."""

    def __init__(self, *a, track=None, guide=4, **kw):
        super().__init__(*a, **kw)
        self.track = dict(DEFAULTS, **(track or {}))
        self.guide = guide

    def init(self, t0=0, left=None, right=None):
        super().init(t0, left, right)
        self.ur = np.asarray(self.new_ur(), np.float32)
        assert len(self.ur) == len(self.pts)
        self.tracked_n, self.matched_n, self.prior_n = 0, 0, 0
        return self

    def step(self, t, left=None, right=None, reclaim=False):
        """reclaim: the front end's keyframe of this step reclaims its map (the window's
        older slots then belong to another epoch: no priors)."""
        B = self.sc.frame(t) if left is None else left
        Br = self.sc.right(t) if right is None else right
        prev = (self.mid.copy(), self.pts.copy(), self.ur.copy())
        stats = super().step(t, B, Br)
        new_ur = np.asarray(self.new_ur(), np.float32)
        n0 = len(self.pts) - len(new_ur)
        assert len(new_ur) == stats["added"]
        prior = None
        if self.guide > 0:
            prior = np.full(n0, NO_PRIOR, np.int64) if reclaim else row_priors(self.mid[:n0], *prev)
        nx, st, _, _ = match_rows_guided(B, Br, self.pts[:n0], prior, self.guide, **self.track)
        self.ur = np.r_[np.where(st == 1, nx[:, 0], np.float32(-1)).astype(np.float32), new_ur].astype(np.float32)
        self.tracked_n, self.matched_n = n0, int(st.sum())
        self.prior_n = 0 if prior is None else int(np.sum(prior != NO_PRIOR))
        self.last_status = st
        return stats


class TrackedStereoLoop(TrackedMixin, RowsOracleLoop):
    """Row SAD at the keyframe (svo_frontend_set_stereo_matcher) and for the tracked features."""

    def new_ur(self):
        return self.trace["ur"]


class _LKColumns(OracleLoop):
    """OracleLoop (stereo LK at the keyframe) that keeps the created features' right columns."""

    def _keyframe(self, left, right, cand, T, t):
        new = np.ascontiguousarray(cand, np.float32)
        self._new_ur = np.zeros(0, np.float32)
        if len(new):
            nr, st, _, _ = O.lk(left, right, new, STEREO["win"], STEREO["max_level"], STEREO["criteria"],
                                STEREO["flags"], acc=self.acc, want_err=False)
            keep = (st == 1) & (np.abs(nr[:, 1] - new[:, 1]) < Y_THRESHOLD)
            newL, newR = new[keep], nr[keep]
            _, xyz = O.triangulate(self.P_left, self.P_right, newL, newR)
            front = xyz[:, 2] > 0
            self._new_ur = newR[front, 0].astype(np.float32)
            return newL[front], transform(T, t, xyz[front])
        return new.reshape(0, 2), np.zeros((0, 3))

    def new_ur(self):
        return self._new_ur


class TrackedStereoLKLoop(TrackedMixin, _LKColumns):
    """The stereo LK at the keyframe, row SAD for the tracked features."""


# ---------------------------------------------------------------- the shared loops
KITTI_BASELINE = 0.537  # metres: fx * 0.537 gives the forward scene 9-66 px of disparity
LOOP_FRAMES = 6


def loop_scene(kind, seed):
    """"wide": WideScene(320, 240) at KITTI's fx * b; "forward": the 640x376 forward
    scene with KITTI's baseline."""
    if kind == "wide":
        return WideScene(320, 240, seed=seed)
    sc = WideSceneForward(640, 376, seed=seed)
    sc.bf = float(sc.K[0, 0]) * KITTI_BASELINE
    return sc


LOOP_FEATURES = {"wide": 400, "forward": 800}


def tracked_trace(kind, seed, guide=4, lk=False):
    return _tracked_trace(kind, seed, guide, lk)


@functools.lru_cache(maxsize=None)
def _tracked_trace(kind, seed, guide, lk):
    """The tracked loop of a scene, run once and shared read-only by the CPU and the
    GPU tests: per frame a namespace with pts, mid, ur (the window's columns), the
    tracked / matched counts, and full_ur: the tracked features' columns by the
    full-range rule on the same points (what guide 0 records: the loop's points do
    not depend on the columns)."""
    cls = TrackedStereoLKLoop if lk else TrackedStereoLoop
    ref = cls(loop_scene(kind, seed), LOOP_FEATURES[kind], guide=guide).init(0)
    out = []

    def snap(t):
        n0 = ref.tracked_n
        full = np.zeros(0, np.float32)
        if t and guide > 0:
            nx, st, _, _ = match_rows(ref.sc.frame(t), ref.sc.right(t), ref.pts[:n0], **ref.track)
            full = np.where(st == 1, nx[:, 0], np.float32(-1)).astype(np.float32)
        elif t:
            full = ref.ur[:n0].copy()
        s = SimpleNamespace(pts=ref.pts.copy(), mid=ref.mid.copy(), ur=ref.ur.copy(), tracked=n0,
                            matched=ref.matched_n, priors=ref.prior_n, full_ur=full)
        for a in (s.pts, s.mid, s.ur, s.full_ur):
            a.setflags(write=False)
        out.append(s)

    snap(0)
    for t in range(1, LOOP_FRAMES):
        ref.step(t)
        snap(t)
    return out
