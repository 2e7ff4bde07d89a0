"""Row SAD on the CPU: the numpy restatement (tests/stereo_rows_reference.py) on
known answers, against the oracle's stereo LK at KITTI's own fx * b, and in the
oracle loop. No GPU."""
import numpy as np
import pytest

import oracle as O
from oracle_loop import STEREO, Y_THRESHOLD
from stereo_rows_reference import KITTI_BF, RowsOracleLoop, WideScene, match_rows, params_ok
from svo_amd.scene import STEREO_BF, Scene


def shifted_pair(d, w=96, h=64, seed=1):
    """R[y][x] = L[y][x + d] on a random image (columns past the edge: fresh noise)."""
    rng = np.random.default_rng(seed)
    wide = rng.integers(0, 256, (h, w + abs(d) + 8), dtype=np.uint8)
    off = max(-d, 0)
    return np.ascontiguousarray(wide[:, off: off + w]), np.ascontiguousarray(wide[:, off + d: off + d + w])


@pytest.mark.parametrize("d", [0, 1, 7, 30, -1])
def test_known_shift_comes_back_exactly(d):
    L, R = shifted_pair(d)
    h, w = L.shape
    # interior: the patch and the right patch inside both images, a bracket on both sides
    xs = np.arange(max(d, 0) + 8, w - 8 - max(-d, 0), 5)
    pts = np.array([(x, y) for y in range(8, h - 8, 7) for x in xs], np.float32)
    nxt, st, disp, cost = match_rows(L, R, pts, d_min=-2, d_max=40)
    assert len(pts) > 50 and st.all()
    assert np.all(disp == d) and np.all(cost == 0)
    # cost 0 at d, random costs beside it: delta = (c- - c+) / (2 (c- + c+)) is not 0 in
    # general; it is where the image repeats the neighbours' costs -- checked below
    assert np.all(np.abs(pts[:, 0] - nxt[:, 0] - d) <= 0.5)
    assert np.array_equal(nxt[:, 1], pts[:, 1])


def test_symmetric_costs_give_delta_zero():
    """A pattern symmetric about the match column: c- == c+, delta == 0, xr = x - d."""
    h, w, d = 32, 96, 6
    rng = np.random.default_rng(5)
    half = rng.integers(0, 256, (h, 24), dtype=np.uint8)
    sym = np.concatenate([half, half[:, -2::-1]], axis=1)  # 47 columns, symmetric about column 23
    L = np.zeros((h, w), np.uint8)
    R = np.zeros((h, w), np.uint8)
    L[:, 30:77] = sym
    R[:, 30 - d:77 - d] = sym
    pts = np.array([[53.0, 16.0]], np.float32)  # the axis of symmetry
    nxt, st, disp, cost = match_rows(L, R, pts, d_min=0, d_max=12, uniq_pct=0)
    assert st[0] == 1 and disp[0] == d and cost[0] == 0
    assert nxt[0, 0] == np.float32(53.0 - d)


def test_tie_takes_the_lowest_disparity_and_den_zero():
    """Period-4 columns: the costs repeat every 4 disparities, the lowest wins."""
    h, w = 32, 96
    col = np.array([10, 200, 90, 40], np.uint8)
    L = np.tile(col, (h, w // 4))
    R = L.copy()
    pts = np.array([[48.0, 16.0]], np.float32)
    nxt, st, disp, cost = match_rows(L, R, pts, d_min=-1, d_max=20, uniq_pct=0)
    assert st[0] == 1 and disp[0] == 0 and cost[0] == 0  # ties at 0, 4, 8, ...: 0
    _, st_u, _, _ = match_rows(L, R, pts, d_min=-1, d_max=20, uniq_pct=80)
    assert st_u[0] == 0  # the runner-up costs 0 as well: 0 * 100 < 80 * 0 fails
    # den == 0 needs c- == c0 == c+, and the tie rule rules it out: c- == c0 would make
    # d* - 1 the smaller minimiser. A constant image: the minimum is the first candidate.
    C = np.full((h, w), 77, np.uint8)
    _, st_c, _, _ = match_rows(C, C, pts, uniq_pct=0)
    assert st_c[0] == 0
    # the nearest case, a flat minimum that starts inside (c- > c0 == c+): delta = 1/2 exactly
    ramp = np.minimum(np.arange(w), 60).astype(np.uint8) * 4
    Lr = np.tile(ramp, (h, 1))  # flat 240 from column 60 on
    Rr = np.full((h, w), 240, np.uint8)
    Rr[:, 86] = 0  # only the window of d = -1 (columns 76..86) sees column 86
    p = np.array([[80.0, 16.0]], np.float32)
    nx, s2, d2, c2 = match_rows(Lr, Rr, p, d_min=-1, d_max=3, uniq_pct=0)
    assert s2[0] == 1 and d2[0] == 0 and c2[0] == 0 and nx[0, 0] == np.float32(79.5)
    Rr[:, 86] = 240  # all costs equal: the first of the equals is d_min, no bracket
    _, s3, d3, _ = match_rows(Lr, Rr, p, d_min=-1, d_max=3, uniq_pct=0)
    assert s3[0] == 0 and d3[0] == 0


def test_half_to_even_rounding():
    L, R = shifted_pair(3)
    for x, xi in ((10.5, 10), (11.5, 12), (40.5, 40), (41.5, 42)):
        p = np.array([[x, 20.5]], np.float32)  # 20.5 -> 20
        q = np.array([[xi, 20.0]], np.float32)
        a = match_rows(L, R, p, d_min=-1, d_max=8)
        b = match_rows(L, R, q, d_min=-1, d_max=8)
        assert a[1][0] == 1 and a[2][0] == b[2][0] == 3 and a[3][0] == b[3][0]
        # the sub-pixel column is taken from the unrounded x
        assert a[0][0, 0] - np.float32(x) == b[0][0, 0] - np.float32(xi)
        assert a[0][0, 1] == np.float32(20.5)


def test_parameter_ranges():
    assert params_ok()
    for bad in (dict(radius=0), dict(radius=8), dict(d_min=-17), dict(d_max=256), dict(d_min=0, d_max=1),
                dict(d_min=-16, d_max=240), dict(uniq_pct=-1), dict(uniq_pct=101), dict(max_cost=-1)):
        assert not params_ok(**bad), bad
    assert params_ok(d_min=-16, d_max=239) and params_ok(d_min=0, d_max=255) and params_ok(d_min=0, d_max=2)


def truth_table(seed, bf):
    sc = Scene(320, 240, seed)
    L, R = sc.frame(0), sc.right(0, bf=bf)
    kp = np.ascontiguousarray(O.fast(L, 20, True)[:, :2], np.float32)
    truth = bf / sc.map_points(kp, 0)[:, 2]
    out = {}
    lk = O.lk(L, R, kp, STEREO["win"], STEREO["max_level"], STEREO["criteria"], STEREO["flags"], want_err=False)
    rows = match_rows(L, R, kp)
    for name, (nr, st) in (("lk", lk[:2]), ("rows", rows[:2])):
        kept = (st == 1) & (np.abs(nr[:, 1] - kp[:, 1]) < Y_THRESHOLD)
        err = np.abs((kp[:, 0] - nr[:, 0]) - truth)
        good = kept & (err <= 1.0)
        out[name] = (int(kept.sum()), int(good.sum()), int((kept & ~good).sum()), err[kept])
    return len(kp), truth, out


@pytest.mark.parametrize("seed", [3, 5, 8])
def test_row_search_beats_the_stereo_lk_at_kitti_disparities(seed):
    n, truth, out = truth_table(seed, KITTI_BF)
    print(f"seed {seed}: {n} corners, disparities {truth.min():.0f}-{truth.max():.0f} px, "
          f"LK kept/good/bad {out['lk'][:3]}, rows kept/good/bad {out['rows'][:3]}")
    assert out["rows"][1] > out["lk"][1], "good matches"
    assert out["rows"][2] < out["lk"][2], "bad matches"


@pytest.mark.parametrize("seed", [3, 5, 8])
def test_every_kept_match_is_good_at_the_default_rig(seed):
    n, truth, out = truth_table(seed, STEREO_BF)
    kept, good, bad, err = out["rows"]
    print(f"seed {seed}: {n} corners, rows kept/good/bad {(kept, good, bad)}, median error {np.median(err):.3f} px")
    assert kept > n // 2 and bad == 0


def test_oracle_loop_with_row_search_follows_the_truth():
    sc = WideScene(320, 240, seed=3)
    ref = RowsOracleLoop(sc, 400).init(0)
    worst = []
    for t in range(1, 6):
        ref.step(t)
        worst.append(np.abs(O.rodrigues(ref.pose[0]) - sc.R(t)).max())
    print("max|R - R_true| per step:", np.array(worst))
    assert max(worst) < 1e-3
