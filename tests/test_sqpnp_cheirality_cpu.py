"""SQPnP's cheirality majority rule (checkSolution: the object-point mean in front
of the camera, or pos >= n - pos points with a positive depth) on the host:
svo_solve_pnp_sqpnp against the oracle's restatement of OpenCV's sqpnp.cpp on
problems whose point mean lies behind the camera, so that the count alone picks
between the pose and its mirror. This pins the reference the device fit is then
compared with (test_sqpnp_fit_gpu.py). Host code only."""
import numpy as np
import pytest

import oracle as O
import svo_amd as S
from sqpnp_stats_reference import KITTI_K, problem

# (nf in front, nb behind, depth scale of the points behind)
CASES = [(100, 0, 40.0), (100, 3, 1000.0), (16, 16, 40.0), (16, 17, 40.0), (50, 50, 40.0), (51, 50, 40.0),
         (50, 51, 40.0), (40, 60, 40.0), (1024, 1024, 40.0), (1025, 1024, 40.0), (1024, 1025, 40.0)]


def oracle_fit(X, uv, K=KITTI_K):
    """O.sqpnp on float object points and float pixels -> (rc, R, t)."""
    q = (uv.astype(np.float64) - [K[0, 2], K[1, 2]]) * [1 / K[0, 0], 1 / K[1, 1]]
    return O.sqpnp(X.astype(np.float64), q)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("nf,nb,zb", CASES)
def test_majority_rule_matches_oracle(nf, nb, zb, seed):
    X, uv, Rt, tt = problem(nf, nb, seed, zb)
    ok, rv, tv = S.solve_pnp_sqpnp(X.astype(np.float64), uv, KITTI_K)
    rc, Ro, to = oracle_fit(X, uv)
    assert ok and rc == 0
    R = O.rodrigues(rv)
    dR = np.abs(R - Ro).max()
    dt = np.abs(tv - to).max()
    dtrue = np.abs(R - Rt).max()
    print(f"nf={nf} nb={nb} seed={seed}: |dR| {dR:.3g} |dt| {dt:.3g} |R - R_true| {dtrue:.3g}")
    assert dR < 1e-9 and dt < 1e-9
    if nb <= nf:  # a tie counts as in front: the true pose
        assert dtrue < 1e-2
    else:  # the majority is behind the true pose's camera: the other solution
        assert dtrue > 1


def test_slow_mirror_solution_departs_from_the_bar():
    """A known departure from the 1e-9 bar, kept so that the figure has a case: the
    generator's (16, 17) problem of seed 3 with its points drawn in shuffled order.
    Both solvers return the mirror pose, 2e-5 apart in R and 7e-5 in t, at costs
    1.3e-7 apart: two SQP runs end near the same minimum within the 1e-10 step
    tolerance, their costs within SQPnP's 1e-6 of each other, and which of the two
    is kept hangs on the runs' last bits. If this test fails because the two now
    agree, assert the bar here instead."""
    rng = np.random.default_rng(3)
    nf, nb, n = 16, 17, 33
    z = np.r_[rng.uniform(6, 30, nf), -rng.uniform(40, 80, nb)]
    X = np.c_[rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), z][rng.permutation(n)]
    Rt = O.rodrigues(rng.normal(0, 0.05, 3))
    t = rng.normal(0, 0.3, 3)
    X = X.astype(np.float32)
    Y = X.astype(np.float64) @ Rt.T + t
    K = KITTI_K
    uv = ((Y[:, :2] / Y[:, 2:]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]] + rng.normal(0, 0.2, (n, 2))).astype(np.float32)
    ok, rv, tv = S.solve_pnp_sqpnp(X.astype(np.float64), uv, K)
    rc, Ro, to = oracle_fit(X, uv)
    assert ok and rc == 0
    R = O.rodrigues(rv)
    dR, dt = np.abs(R - Ro).max(), np.abs(tv - to).max()
    print(f"shuffled (16, 17) seed 3: |dR| {dR:.3g} |dt| {dt:.3g}")
    assert np.abs(R - Rt).max() > 1 and np.abs(Ro - Rt).max() > 1  # the mirror, both
    assert 1e-9 < dR < 1e-4 and 1e-9 < dt < 1e-3
