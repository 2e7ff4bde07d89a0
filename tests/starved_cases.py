"""Starved sequences for the batched front end (TEST INFRASTRUCTURE): 320x240
synthetic stereo sequences that lose their features -- tiny feature sets, frames
replaced by a constant image (a dark or dropped camera frame), a sequence that
never shows a corner -- and their oracle loops (tests/oracle_loop.py), run once
per case and shared, read-only, by the GPU tests (test_frontend_starved_gpu.py)
and their CPU companions (test_starved_oracle_cpu.py)."""
from __future__ import annotations

import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import oracle as O
from extreme_images import binarise
from oracle_loop import OracleLoop
from svo_amd.scene import Scene, SceneForward

W, H = 320, 240

# seed: Scene(W, H, seed); n: n_features; frames: frames 0 .. frames - 1;
# drops: the frames replaced by the constant image, on `side` ("both", "left",
# "right"); every: replace every frame t with t % every == 0 as well (t >= 1);
# blank: every frame constant from frame 0; bucket / acc: OracleLoop's; forward:
# SceneForward (translation, an occluder: RANSAC drops points every frame and the
# keyframes add tens) instead of Scene; strips / strip: on the frames `strips` the
# left `strip` columns of both images are constant (the features there are lost,
# the others live on); binary: both images binarised (extreme_images.binarise: 255
# where the frame is >= 128, else 0 -- the scene's geometry and motion at full contrast)
Case = namedtuple("Case", "seed n frames drops side every blank bucket acc forward strips strip binary",
                  defaults=((), "both", 0, False, (0, 0), O.ACC_EXACT, False, (), W // 2, False))

LADDER = [Case(seed, n, 6) for seed in (2, 5) for n in range(1, 10)]
DROPPED_64 = Case(4, 64, 9, drops=(3, 6))
DROPPED_300 = Case(4, 300, 9, drops=(3, 6))
BLANK = Case(4, 64, 9, blank=True)
# the t % 3 drops of the streamed run: 24 steps, the map outgrows a 4-frame ring's 6 * 64 slots
STREAMED = Case(4, 64, 25, every=3)
# a streamed run whose map fills while features live: five drops and rebuilds, then
# every second frame loses the left 100 columns' features and the next replaces them
RECLAIM = Case(3, 450, 25, drops=(2, 4, 6, 8, 10), strips=tuple(range(12, 24, 2)), strip=100)
# binarised scenes (test_frontend_saturated_gpu.py): the two seeds of one batch
SATURATED_SEEDS = (4, 2)


def saturated(n, forward=False, **kw):
    return [Case(seed, n, 7, binary=True, forward=forward, **kw) for seed in SATURATED_SEEDS]


def blank_image():
    return np.full((H, W), 128, np.uint8)


def scene(case):
    return (SceneForward if case.forward else Scene)(W, H, seed=case.seed)


def is_dropped(case, t):
    return case.blank or t in case.drops or (case.every > 0 and t >= 1 and t % case.every == 0)


@functools.lru_cache(maxsize=None)
def frames(case):
    """[(left, right)] of the case's frames, the dropped ones doctored."""
    sc = scene(case)
    out = []
    for t in range(case.frames):
        L, R = np.ascontiguousarray(sc.frame(t)), np.ascontiguousarray(sc.right(t))
        if is_dropped(case, t):
            if case.side in ("both", "left"):
                L = blank_image()
            if case.side in ("both", "right"):
                R = blank_image()
        elif t in case.strips:
            L, R = L.copy(), R.copy()
            L[:, : case.strip] = 128
            R[:, : case.strip] = 128
        if case.binary:
            L, R = binarise(L), binarise(R)
        L.setflags(write=False)
        R.setflags(write=False)
        out.append((L, R))
    return out


@functools.lru_cache(maxsize=None)
def oracle_trace(case):
    """The oracle loop of the case: one snapshot per frame (frame 0: init) with
    the step's statistics (`stats`, None at init) and the state `_compare_step`
    reads (pts, pose, X)."""
    fr = frames(case)
    ref = OracleLoop(scene(case), case.n, bucket=case.bucket, acc=case.acc).init(0, *fr[0])
    snaps = []

    def snap(stats):
        s = SimpleNamespace(stats=stats, pts=ref.pts.copy(), pose=(ref.pose[0].copy(), ref.pose[1].copy()),
                            X=ref.X.copy(), mid=ref.mid.copy())
        for a in (s.pts, s.X, *s.pose):
            a.setflags(write=False)
        snaps.append(s)

    snap(None)
    for t in range(1, case.frames):
        snap(ref.step(t, *fr[t]))
    return snaps


def tracked_counts(case):
    return [s.stats["tracked"] for s in oracle_trace(case)[1:]]


def is_no_model(stats):
    """calculatePose found no model: all 100 hypotheses tried, every feature dropped."""
    return (stats["tracked"] >= 4 and stats.get("hypotheses") == 100 and stats["inliers"] == 0
            and stats["features"] == 0)


def is_garbage_model(stats):
    """A model accepted from fewer than half of the tracked points."""
    return stats["tracked"] >= 4 and 0 < stats["inliers"] < stats["tracked"] / 2


def is_rebuild(stats):
    """Nothing tracked, and the keyframe rebuilds the set from nothing."""
    return stats["tracked"] == 0 and stats["added"] > 0 and stats["features"] == stats["added"]


def cumulative_added(case):
    """Map points created up to and including each frame (frame 0: init's)."""
    tr = oracle_trace(case)
    out = [len(tr[0].pts)]
    for s in tr[1:]:
        out.append(out[-1] + s.stats["added"])
    return out


def map_occupancy(case, n_frames=4):
    """The front end's map of the case, streamed into a ring of n_frames, replayed on
    the oracle's counts: per step t >= 1 a namespace with map_n before the keyframe,
    the features kept (n), the keyframe's take, whether map_n + take exceeds the
    CAP * (n_frames + 2) slots (the keyframe reclaims the map then: map_n = n), and
    whether the kept features' creation ids are 0 .. n - 1 (at the first reclaim these
    are the map ids: nothing would move)."""
    cap = (case.n + 63) // 64 * 64
    slots = cap * (n_frames + 2)
    tr = oracle_trace(case)
    map_n = len(tr[0].pts)
    out = [None]
    for s in tr[1:]:
        n = s.stats["features"] - s.stats["added"]
        take = s.stats["take"]
        over = map_n + take > slots
        ident = bool(np.array_equal(s.mid[:n], np.arange(n)))
        out.append(SimpleNamespace(map_n=map_n, n=n, take=take, reclaim=over, identity=ident, slots=slots))
        if over:
            map_n = n
        map_n += s.stats["added"]
    return out


def assert_reclaim_moves_live_points(case, n_frames=4, block=256):
    """The oracle-side conditions of a reclaim that has work to do: at the first step
    whose keyframe overflows the ring's map, more than `block` features are kept
    (two chunks of the kernel's block), their map ids are not 0 .. n - 1 (earlier
    features were lost: points really move), and candidates are taken behind them.
    Returns that step."""
    occ = map_occupancy(case, n_frames)
    first = next((t for t in range(1, case.frames) if occ[t].reclaim), None)
    assert first is not None, [(o.map_n, o.n, o.take) for o in occ[1:]]
    o = occ[first]
    assert o.n > block and not o.identity and o.take > 0, vars(o)
    mid = oracle_trace(case)[first].mid[: o.n]
    assert np.all(np.diff(mid) > 0) and mid[-1] >= o.n  # strictly increasing, some point moves down
    return first


def assert_saturated_conditions(cases):
    """The oracle side of the binarised cases: every left frame is 0 / 255 with a
    full-range edge (max |Scharr| = 4080), every step tracks at least 50 features,
    and RANSAC keeps >= 0.9 of them on Scene, >= 0.6 on SceneForward."""
    for case in cases:
        for L, _ in frames(case):
            assert set(np.unique(L)) <= {0, 255}
            assert int(np.abs(O.scharr(L).astype(np.int32)).max()) == 4080
        for s in oracle_trace(case)[1:]:
            st = s.stats
            assert st["tracked"] >= 50, (case, st)
            assert st["inliers"] >= (0.6 if case.forward else 0.9) * st["tracked"], (case, st)
