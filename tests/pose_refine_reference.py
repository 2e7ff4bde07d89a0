"""Independent numpy restatement of the motion-only stereo refinement (CPU only),
as include/svo_gpu.h states it for svo_refine_poses_stereo: the 28 sums of one
pose over constant points, built on ba_stereo_reference.obs_terms with one camera,
and svo_refine_poses' Levenberg-Marquardt control per problem. Every function
takes a dtype, so the same run exists in float64 and in np.longdouble; their
distance is the rounding error the GPU tests derive their bars from."""
import numpy as np

import ba_reference as B
import ba_stereo_reference as R

K = B.K
BASELINE = R.BASELINE
TRIU6 = np.triu_indices(6)


def terms(T, X, xy, ur, baseline, delta, dt=np.float64):
    """obs_terms of one camera at pose T seeing every point once -> (front, stereo, r, w, cost, Jc)."""
    n = len(X)
    X = np.asarray(X, dt).reshape(n, 3)
    front, stereo, r, w, cost, Jc, _ = R.obs_terms(np.asarray(T, dt)[None], X, np.zeros(n, np.int64), np.arange(n),
                                                   np.asarray(xy, np.float32).reshape(n, 2),
                                                   np.asarray(ur, np.float32).reshape(n), baseline, delta, dt)
    return front, stereo, r, w, cost, Jc


def linearize(T, X, xy, ur, baseline=BASELINE, delta=0.0, dt=np.float64):
    """The 28 sums at T: H (upper triangle of sum w J^T J, row-major, 21), g (sum w
    J^T r, 6), cost. A point with Pz <= 0 contributes nothing (w = cost = 0)."""
    _, _, r, w, cost, Jc = terms(T, X, xy, ur, baseline, delta, dt)
    H = np.einsum("n,nai,naj->ij", w, Jc, Jc)
    g = np.einsum("n,nai,na->i", w, Jc, r)
    return np.r_[H[TRIU6], g, cost.sum()].astype(dt)


def left_update(T, xi, dt=np.float64):
    """refine.cpp's se3_left_update: T <- exp(xi^) T, the series below |phi| = 1e-8."""
    T, xi = np.asarray(T, dt), np.asarray(xi, dt)
    rho, ph = xi[:3], xi[3:]
    th2 = ph @ ph
    th = np.sqrt(th2)
    if th < 1e-8:
        a, b, c = 1 - th2 / 6, dt(0.5) - th2 / 24, dt(1) / 6 - th2 / 120
    else:
        a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    W, I = B.hat(ph).astype(dt), np.eye(3, dtype=dt)
    dR, V = I + a * W + b * (W @ W), I + b * W + c * (W @ W)
    return np.r_[(dR @ T[:9].reshape(3, 3)).ravel(), dR @ T[9:] + V @ rho]


def solve(ne, lam, dt=np.float64):
    """refine.cpp's lm_solve: (H + lam diag*(H)) x = -g by Cholesky, None if not
    positive definite; a diagonal entry that is not positive is damped by lam 1e-12."""
    A = np.zeros((6, 6), dt)
    A[TRIU6] = ne[:21]
    A = A + np.triu(A, 1).T
    d = np.diag(A).copy()
    A[np.diag_indices(6)] = d + dt(lam) * np.where(d > 0, d, dt(1e-12))
    return B.chol_solve(A, -np.asarray(ne[21:27], dt))


def lm(T, X, xy, ur, baseline=BASELINE, delta=0.0, max_iterations=20, dt=np.float64, history=None):
    """svo_refine_poses' control for one problem -> (pose, (initial, final cost),
    iterations, the 28 sums at the returned pose). Every iteration that was begun
    counts. history: as ba_reference.lm's (event, retries, c_cur, c_trial, cost)."""
    cur = np.array(T, dt)
    ne = linearize(cur, X, xy, ur, baseline, delta, dt)
    c_first = ne[27]
    lam, it = 1e-4, 0
    log = [] if history is None else history
    for it in range(1, max_iterations + 1):
        retries = 0
        dx = solve(ne, lam, dt)
        while dx is None and lam < 1e16:
            lam *= 10
            retries += 1
            dx = solve(ne, lam, dt)
        c_cur = ne[27]
        if dx is None:
            log.append({"event": "give up", "retries": retries, "c_cur": c_cur, "c_trial": None, "cost": c_cur})
            break
        if np.sqrt(dx @ dx) < 1e-12 * (1 + np.sqrt(cur[9:] @ cur[9:])):
            log.append({"event": "small step", "retries": retries, "c_cur": c_cur, "c_trial": None, "cost": c_cur})
            break
        trial = left_update(cur, dx, dt)
        nt = linearize(trial, X, xy, ur, baseline, delta, dt)
        c1 = nt[27]
        log.append({"event": "accept" if c1 <= c_cur else "reject", "retries": retries, "c_cur": c_cur, "c_trial": c1,
                    "cost": min(c1, c_cur)})
        if c1 <= c_cur:
            cur, ne = trial, nt
            lam = max(lam * 0.1, 1e-12)
            if c_cur - c1 <= 1e-15 * c_cur:
                break
        else:
            lam *= 10
            if lam >= 1e16:
                break
    return cur, (c_first, ne[27]), it, ne


def lm_prefix(T, X, xy, ur, baseline=BASELINE, delta=0.0, max_iterations=14, margin=1e-6):
    """ba_reference.lm_prefix for this LM: K = the longest prefix of iterations in
    which float64 and longdouble decide alike (same event, same lambda retries) and
    every decision is clear, |c_trial - c_cur| > margin c_cur in both. Also the two
    full results -> (K, float64 history, longdouble history, float64 result, longdouble result)."""
    h64, hld = [], []
    r64 = lm(T, X, xy, ur, baseline, delta, max_iterations, np.float64, h64)
    rld = lm(T, X, xy, ur, baseline, delta, max_iterations, np.longdouble, hld)
    k = 0
    for a, b in zip(h64, hld):
        if a["event"] != b["event"] or a["retries"] != b["retries"] or a["event"] not in ("accept", "reject"):
            break
        if not all(abs(h["c_trial"] - h["c_cur"]) > margin * h["c_cur"] for h in (a, b)):
            break
        k += 1
    return k, h64, hld, r64, rld


def stereo_scene(n, seed, noise=0.0, outliers=0.0, mono_fraction=0.5, baseline=BASELINE):
    """test_reproj_gpu.scene with a right column: n points at 5 - 40 m, a pose near
    the identity, float32 pixels (+ N(0, noise), a fraction `outliers` moved by up
    to 60 px) and, for all but a random fraction mono_fraction of the points and
    those whose column would be negative, the right image's column (same noise,
    outliers moved by +-40 px); -1 for the others -> (X, xy, ur, T)."""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(5, 40, n)]
    T = left_update(np.r_[np.eye(3).ravel(), rng.normal(0, 0.3, 3)], np.r_[0, 0, 0, rng.normal(0, 0.05, 3)])
    u, P = B.project(T, X)
    ur = B.FX * (P[:, 0] - baseline) / P[:, 2] + B.CX
    if noise:
        u = u + rng.normal(0, noise, u.shape)
        ur = ur + rng.normal(0, noise, n)
    if outliers:
        m = rng.random(n) < outliers
        u[m] += rng.uniform(-60, 60, (m.sum(), 2))
        m = rng.random(n) < outliers
        ur[m] += rng.choice([-40.0, 40.0], m.sum())
    drop = (rng.random(n) < mono_fraction) | ~(ur >= 0)
    return X, u.astype(np.float32), np.where(drop, -1.0, ur).astype(np.float32), T


def start_pose(T, seed, dpos, drot):
    """T moved by a translation of dpos m and a rotation of drot rad in random directions."""
    rng = np.random.default_rng(seed + 500)
    a, b = rng.normal(size=3), rng.normal(size=3)
    return left_update(T, np.r_[dpos * a / np.linalg.norm(a), drot * b / np.linalg.norm(b)])


# The GPU trajectory scenes: name -> (n, seed, noise, outliers, Huber delta, dpos, drot).
# "far" is 0.5 m / 0.05 rad off; the pose-only LM accepts every step from there
# (seeds 0 .. 39 of every shape), so the "rough" starts, 6 m / 0.6 rad off, are the
# ones whose steps are rejected. Every scene has pixel noise: on exact data the
# cost falls to the float32 rounding of the pixels (1e-8), where float64 and
# longdouble sums differ by 1e-9 of it and no cost bar of 1e-10 can hold; and the
# seeds are those (of 0 .. 79) whose rough trajectory is the same in float64 and
# longdouble to 1e-12 of the cost (test_pose_refine_cpu) -- from 6 m off some are
# not, a point crossing the camera plane at one precision and not at the other.
TRAJECTORY = {"n40-noise-far": (40, 1, 0.5, 0.0, 0.0, 0.5, 0.05),
              "n40-noise-rough": (40, 73, 0.5, 0.0, 0.0, 6.0, 0.6),
              "n40-outliers-huber-rough": (40, 67, 0.5, 0.1, 2.0, 6.0, 0.6),
              "n300-outliers-huber-rough": (300, 2, 0.5, 0.2, 2.0, 6.0, 0.6),
              "n1500-noise-huber-far": (1500, 3, 1.0, 0.1, 2.0, 0.5, 0.05)}
TRAJECTORY_ITERATIONS = 12


def trajectory_case(name):
    """-> (X, xy, ur, true pose, start pose, Huber delta)"""
    n, seed, noise, outliers, delta, dpos, drot = TRAJECTORY[name]
    X, xy, ur, T = stereo_scene(n, seed, noise, outliers)
    return X, xy, ur, T, start_pose(T, seed, dpos, drot), delta
