"""Independent numpy restatement of the windowed bundle adjustment (CPU only):
per-observation residuals and Jacobians, the U / V / W blocks, the Schur
complement, the dense solve and the Levenberg-Marquardt loop, as
include/svo_gpu.h states them for svo_ba_linearize / svo_bundle_adjust. Every
function takes a dtype, so the same computation runs in float64 and in
np.longdouble: their distance on a test's own inputs is the measured rounding
error the GPU tests derive their bars from."""
import numpy as np

K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])
FX, FY, CX, CY = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
TRIU6 = np.triu_indices(6)
TRIU3 = np.triu_indices(3)


def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def se3_exp(xi, dt=np.float64):
    xi = np.asarray(xi, dt)
    rho, ph = xi[:3], xi[3:]
    th = np.linalg.norm(ph)
    W, I = hat(ph), np.eye(3, dtype=dt)
    if th < 1e-10:
        return I + W, rho
    A, B, C = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return I + A * W + B * W @ W, (I + B * W + C * W @ W) @ rho


def left_update(T, xi, dt=np.float64):
    T = np.asarray(T, dt)
    R, t = T[:9].reshape(3, 3), T[9:]
    dR, dd = se3_exp(xi, dt)
    return np.r_[(dR @ R).ravel(), dR @ t + dd]


def project(T, X):
    P = X @ T[:9].reshape(3, 3).T + T[9:]
    return np.c_[FX * P[:, 0] / P[:, 2] + CX, FY * P[:, 1] / P[:, 2] + CY], P


def sort_observations(obs_cam, obs_point, n_cams, n_points):
    """Stable sort by (point, camera) and the index lists of the staged order."""
    obs_cam, obs_point = np.asarray(obs_cam), np.asarray(obs_point)
    order = np.lexsort((obs_cam, obs_point))  # stable; last key is the primary one
    pt_off = np.r_[0, np.cumsum(np.bincount(obs_point, minlength=n_points))]
    cam_off = np.r_[0, np.cumsum(np.bincount(obs_cam, minlength=n_cams))]
    sc = obs_cam[order]
    cam_idx = np.concatenate([np.flatnonzero(sc == j) for j in range(n_cams)]) if n_cams else np.zeros(0, int)
    return order, pt_off, cam_off, cam_idx


def window_scene(C=6, M=300, seed=0, drop=0.3, noise=0.0, outliers=0.0, step=0.8, min_obs=0):
    """C cameras stepping `step` m along z (small rotations), M points at 6 - 40 m,
    a fraction `drop` of the observations missing (every point keeps at least
    min_obs), float32 observations in a random order."""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-8, 8, M), rng.uniform(-3, 3, M), rng.uniform(6, 40, M)]
    poses = []
    for j in range(C):
        R, _ = se3_exp(np.r_[0, 0, 0, rng.normal(0, 0.01, 3)])
        c = np.array([0.05 * np.sin(j), 0.02 * j, step * j])  # camera centre in the world
        poses.append(np.r_[R.ravel(), -R @ c])
    poses = np.array(poses)
    oc, op = np.meshgrid(np.arange(C), np.arange(M), indexing="ij")
    oc, op = oc.ravel(), op.ravel()
    keep = (rng.random(len(oc)) >= drop).reshape(C, M)
    for i in np.flatnonzero(keep.sum(0) < min(min_obs, C)):  # give a starved point its first cameras back
        keep[np.flatnonzero(~keep[:, i])[:min(min_obs, C) - keep[:, i].sum()], i] = True
    keep = keep.ravel()
    oc, op = oc[keep], op[keep]
    perm = rng.permutation(len(oc))  # any order
    oc, op = oc[perm], op[perm]
    xy = np.zeros((len(oc), 2))
    for j in range(C):
        m = oc == j
        xy[m] = project(poses[j], X[op[m]])[0]
    if noise:
        xy += rng.normal(0, noise, xy.shape)
    if outliers:
        m = rng.random(len(oc)) < outliers
        xy[m] += rng.choice([-40.0, 40.0], (m.sum(), 2))
    return {"poses": poses, "points": X, "fixed": np.zeros(C, np.uint8), "obs_cam": oc.astype(np.int32),
            "obs_point": op.astype(np.int32), "obs_xy": xy.astype(np.float32)}


def perturbed(prob, seed, n_fixed=2, dpos=0.05, drot=0.005, depth=0.03):
    """The start of the convergence tests: the first n_fixed cameras fixed at the
    truth, the others moved by N(0, dpos) m and N(0, drot) rad, every point's depth
    (its distance from the first camera) scaled by 1 +- depth."""
    rng = np.random.default_rng(seed)
    q = dict(prob)
    q["poses"] = prob["poses"].copy()
    q["fixed"] = np.zeros(len(q["poses"]), np.uint8)
    q["fixed"][:n_fixed] = 1
    for j in range(n_fixed, len(q["poses"])):
        q["poses"][j] = left_update(prob["poses"][j], np.r_[rng.normal(0, dpos, 3), rng.normal(0, drot, 3)])
    q["points"] = prob["points"] * (1 + rng.uniform(-depth, depth, (len(prob["points"]), 1)))
    return q


PARITY_SHAPES = [(2, 1), (3, 63), (4, 64), (5, 65), (16, 300)]


def parity_case(C, M, seed, outliers=0.0):
    """A linearisation-parity problem: 30 % of the observations dropped, 0.5 px
    noise, the first camera fixed and everything else off the truth; from 63
    points on, point 5 lies behind camera 1, point 10 has no observation and
    point 11 a single one. The cameras step 0.25 m, so that the sixteenth still
    stands 2 m in front of the nearest point: a point a hair from a camera's plane
    has Jacobian entries of 1e6 and more, and no per-entry bar holds there."""
    prob = perturbed(window_scene(C, M, seed, drop=0.3, noise=0.5, outliers=outliers, step=0.25), seed + 1000,
                     n_fixed=1)
    if M >= 63:
        T = prob["poses"][1]
        R, t = T[:9].reshape(3, 3), T[9:]
        prob["points"][5] = R.T @ (np.array([0.3, -0.2, -3.0]) - t)  # 3 m behind camera 1
        oc, op = prob["obs_cam"], prob["obs_point"]
        keep = (op != 10) & ((op != 11) | (np.cumsum(op == 11) == 1))
        if not np.any((oc == 1) & (op == 5)):  # camera 1 must see the point behind it
            k = np.flatnonzero(keep & (op != 5) & (op != 11))[0]
            oc[k], op[k] = 1, 5
        for key in ("obs_cam", "obs_point", "obs_xy"):
            prob[key] = prob[key][keep]
    return prob


def dense_duplicates(seed=0, outliers=0.0, repeat=70):
    """2 cameras (the first fixed), 5 points, every (camera, point) pair observed
    `repeat` times with N(0, 0.5 px) noise, shuffled: 350 observations per camera
    (the camera pass strides twice), 560 among the first four points (the
    elimination's staging strides twice), runs of 70 to sum."""
    rng = np.random.default_rng(seed + 500)
    prob = perturbed(window_scene(C=2, M=5, seed=seed, drop=0, step=0.25), seed + 1000, n_fixed=1)
    perm = rng.permutation(10 * repeat)
    oc, op = np.repeat(prob["obs_cam"], repeat)[perm], np.repeat(prob["obs_point"], repeat)[perm]
    xy = np.repeat(prob["obs_xy"].astype(np.float64), repeat, axis=0)[perm] + rng.normal(0, 0.5, (10 * repeat, 2))
    if outliers:
        m = rng.random(len(oc)) < outliers
        xy[m] += rng.choice([-40.0, 40.0], (m.sum(), 2))
    prob["obs_cam"], prob["obs_point"], prob["obs_xy"] = oc, op, xy.astype(np.float32)
    return prob


def sparse_duplicates(seed=0, outliers=0.0):
    """3 cameras (the first fixed), 20 points, one observation per pair, except:
    point 0 is seen by camera 1 alone, twice, 0.5 px apart (one view: no depth
    constraint, so it is constant); point 1 twice by camera 1 and once by camera 2
    (two views: free)."""
    prob = perturbed(window_scene(C=3, M=20, seed=seed, drop=0, noise=0.5, outliers=outliers, step=0.25), seed + 1000,
                     n_fixed=1)
    oc, op, xy = prob["obs_cam"], prob["obs_point"], prob["obs_xy"]
    at = {(j, i): xy[(oc == j) & (op == i)][0] for j in (1, 2) for i in (0, 1)}
    keep = op > 1
    add = [(1, 0, at[1, 0]), (1, 1, at[1, 1]), (2, 1, at[2, 1]), (1, 0, at[1, 0] + np.float32([0.5, 0])),
           (1, 1, at[1, 1] + np.float32([-0.25, 0.5]))]
    prob["obs_cam"] = np.r_[oc[keep], [a[0] for a in add]].astype(np.int32)
    prob["obs_point"] = np.r_[op[keep], [a[1] for a in add]].astype(np.int32)
    prob["obs_xy"] = np.vstack([xy[keep]] + [a[2][None] for a in add]).astype(np.float32)
    return prob


def wide_camera(seed=0, outliers=0.0):
    """2 cameras (the first fixed), 300 points, nothing dropped: 300 observations
    per camera (the camera pass strides twice) and two blocks of points."""
    return perturbed(window_scene(C=2, M=300, seed=seed, drop=0, noise=0.5, outliers=outliers, step=0.25), seed + 1000,
                     n_fixed=1)


def full_system(seed=0, outliers=0.0):
    """parity_case(16, 40) with no camera fixed: 16 free cameras, the reduced
    system of order 96 with all kMaxNS = 4656 packed entries."""
    prob = parity_case(16, 40, seed, outliers)
    prob["fixed"] = np.zeros(16, np.uint8)
    return prob


def on_axis():
    """One free camera at the identity, one point at (0, 0, 10) on its axis, one
    observation. x = y = 0 exactly, so rows and columns 2 and 5 of U are exactly
    zero at every lambda; the point is seen once, so it is constant and S = U*:
    the third pivot of the Cholesky factorisation is exactly zero."""
    return {"poses": np.r_[np.eye(3).ravel(), 0, 0, 0][None], "points": np.array([[0.0, 0.0, 10.0]]),
            "fixed": np.zeros(1, np.uint8), "obs_cam": np.zeros(1, np.int32), "obs_point": np.zeros(1, np.int32),
            "obs_xy": np.array([[600.0, 180.0]], np.float32)}


# Starts rough enough that LM overshoots and rejects steps: (C, M, seed, dpos,
# Huber delta). Most seeds of this family reject only at convergence, where the
# trial cost differs from the current one in the ninth digit and rounding
# decides; these are the seeds (of 0 .. 39, Huber: 40 .. 249) whose rejections
# are clear in float64 and in longdouble alike (test_bundle_adjust_cpu).
REJECT_SCENES = [(3, 12, 21, 0.5, 0.0), (3, 12, 76, 0.5, 2.0), (4, 40, 12, 1.0, 0.0)]
REJECT_ITERATIONS = 16


def reject_scene(C, M, seed, dpos=0.5):
    """Two fixed cameras, the others off by N(0, dpos m) / N(0, 0.05 rad), depths by 1 +- 30 %."""
    return perturbed(window_scene(C, M, seed, min_obs=2), seed + 1, dpos=dpos, drot=0.05, depth=0.3)


def healthy(k):
    """Problem k of test_batch_equals_one_by_one's batch."""
    return perturbed(window_scene(C=3 + k % 3, M=40 + 9 * k, seed=20 + k, noise=0.3, outliers=0.05), seed=k)


# one value of healthy(2) (5 cameras, two of them fixed) replaced: kind -> Huber delta
POISONED = {"nan observation": 0.0, "nan pose rotation": 0.0, "nan pose depth": 0.0, "nan point": 0.0,
            "inf observation": 2.0}


def poisoned(kind):
    """"nan pose depth" puts the NaN into tz and "nan point" into a point: Pz is NaN
    for every observation of that camera (of that point), the Pz <= 0 rule drops
    them all and the cost stays finite."""
    q = healthy(2)
    q["poses"], q["points"], q["obs_xy"] = q["poses"].copy(), q["points"].copy(), q["obs_xy"].copy()
    k = int(np.flatnonzero(q["obs_cam"] == 3)[0])  # an observation by a free camera
    if kind == "nan observation":
        q["obs_xy"][k, 0] = np.nan
    elif kind == "inf observation":
        q["obs_xy"][k, 1] = np.inf
    elif kind == "nan pose rotation":
        q["poses"][3, 1] = np.nan
    elif kind == "nan pose depth":
        q["poses"][3, 11] = np.nan
    elif kind == "nan point":
        q["points"][q["obs_point"][k], 2] = np.nan
    else:
        raise KeyError(kind)
    return q


def batch(probs):
    """Problems padded to one ragged batch: the arrays and the three count vectors."""
    P = len(probs)
    nc = np.array([len(q["poses"]) for q in probs], np.int32)
    nm = np.array([len(q["points"]) for q in probs], np.int32)
    no = np.array([len(q["obs_cam"]) for q in probs], np.int32)
    poses, fixed = np.zeros((P, nc.max(), 12)), np.zeros((P, nc.max()), np.uint8)
    points = np.zeros((P, nm.max(), 3))
    oc, op = np.zeros((P, max(no.max(), 1)), np.int32), np.zeros((P, max(no.max(), 1)), np.int32)
    oxy = np.zeros((P, max(no.max(), 1), 2), np.float32)
    for p, q in enumerate(probs):
        poses[p, :nc[p]], fixed[p, :nc[p]], points[p, :nm[p]] = q["poses"], q["fixed"], q["points"]
        oc[p, :no[p]], op[p, :no[p]], oxy[p, :no[p]] = q["obs_cam"], q["obs_point"], q["obs_xy"]
    return {"poses": poses, "fixed": fixed, "points": points, "obs_cam": oc, "obs_point": op, "obs_xy": oxy,
            "n_cams": nc, "n_points": nm, "n_obs": no}


def rounding_error(prob, lam, delta):
    """How far the float64 restatement of S, b, dc, dp lies from the same
    computation in np.longdouble, relative to the largest entry of each."""
    a, b = linearize(prob, lam, delta, np.float64), linearize(prob, lam, delta, np.longdouble)
    return {k: float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()) if b[k].size and np.abs(b[k]).max() > 0 else 0.0
            for k in ("S", "b", "dc", "dp")}


def obs_terms(poses, points, oc, op, oxy, delta, dt=np.float64):
    """Per observation: in-front flag, residual r (n, 2), weight w, cost, Jc (n, 2, 6),
    Jp (n, 2, 3); w and cost are zero where the point is not in front."""
    T = np.asarray(poses, dt)[oc]
    R, t = T[:, :9].reshape(-1, 3, 3), T[:, 9:]
    X = np.asarray(points, dt)[op]
    Pc = np.einsum("nij,nj->ni", R, X) + t
    front = Pc[:, 2] > 0
    z = np.where(front, Pc[:, 2], dt(1))
    x, y = Pc[:, 0] / z, Pc[:, 1] / z
    fx, fy, cx, cy = dt(FX), dt(FY), dt(CX), dt(CY)
    u = np.asarray(oxy, np.float32).astype(dt)
    r = np.stack([fx * x + cx - u[:, 0], fy * y + cy - u[:, 1]], 1)
    o = np.zeros_like(z)
    Jc = np.stack([np.stack([fx / z, o, -fx * x / z, -fx * x * y, fx * (1 + x * x), -fx * y], 1),
                   np.stack([o, fy / z, -fy * y / z, -fy * (1 + y * y), fy * x * y, fy * x], 1)], 1)
    Jp = np.einsum("nak,nkc->nac", Jc[:, :, :3], R)
    nr = np.sqrt((r * r).sum(1))
    d = dt(delta)
    rob = (delta > 0) & (nr > d)
    w = np.where(rob, d / np.where(rob, nr, dt(1)), dt(1))
    cost = np.where(rob, d * (nr - dt(0.5) * d), dt(0.5) * nr * nr)
    return front, r, np.where(front, w, dt(0)), np.where(front, cost, dt(0)), Jc, Jp


def inv3_sym(A):
    """Closed-form inverse of symmetric 3x3 blocks (n, 3, 3) and their positive
    definiteness (leading minors)."""
    a, b, c, d, e, f = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * c00 + b * c01 + c * c02
    pd = (a > 0) & (c22 > 0) & (det > 0)
    sd = np.where(pd, det, 1)
    inv = np.stack([np.stack([c00, c01, c02], 1), np.stack([c01, c11, c12], 1), np.stack([c02, c12, c22], 1)], 1)
    return inv / sd[:, None, None], pd


def chol_solve(S, b):
    """Cholesky solve in S's own dtype (np.linalg has no longdouble); None if S is
    not positive definite."""
    n = len(b)
    L = np.zeros_like(S)
    for j in range(n):
        s = S[j:, j] - L[j:, :j] @ L[j, :j]
        if not s[0] > 0:
            return None
        L[j:, j] = s / np.sqrt(s[0])
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def linearize(prob, lam, delta=0.0, dt=np.float64, count_observations=False):
    """What svo_ba_linearize returns, plus the blocks behind it. A point is free
    when at least two distinct cameras see it in front of them (pt_cnt);
    count_observations: the rule this replaced, which counted a camera's second
    observation of a point as a second view (kept to show that a test can tell
    the two apart)."""
    poses, points = prob["poses"], prob["points"]
    oc, op = np.asarray(prob["obs_cam"]), np.asarray(prob["obs_point"])
    C, M = len(poses), len(points)
    front, r, w, cost, Jc, Jp = obs_terms(poses, points, oc, op, prob["obs_xy"], delta, dt)
    U, gc = np.zeros((C, 6, 6), dt), np.zeros((C, 6), dt)
    V, gp = np.zeros((M, 3, 3), dt), np.zeros((M, 3), dt)
    W = np.zeros((C, M, 6, 3), dt)
    np.add.at(U, oc, w[:, None, None] * np.einsum("nai,naj->nij", Jc, Jc))
    np.add.at(gc, oc, w[:, None] * np.einsum("nai,na->ni", Jc, r))
    np.add.at(V, op, w[:, None, None] * np.einsum("nai,naj->nij", Jp, Jp))
    np.add.at(gp, op, w[:, None] * np.einsum("nai,na->ni", Jp, r))
    np.add.at(W, (oc, op), w[:, None, None] * np.einsum("nai,naj->nij", Jc, Jp))
    cam_cnt = np.bincount(oc[front], minlength=C)
    seen = np.zeros((M, C), bool)
    seen[op[front], oc[front]] = True
    pt_cnt = np.bincount(op[front], minlength=M) if count_observations else seen.sum(1)
    lam = dt(lam)
    Vs = V + lam * V * np.eye(3, dtype=dt)
    Vinv, pd = inv3_sym(Vs)
    pt_free = (pt_cnt >= 2) & pd
    Vinv = np.where(pt_free[:, None, None], Vinv, dt(0))
    free = [j for j in range(C) if not prob["fixed"][j] and cam_cnt[j] > 0]
    nf = len(free)
    Wf = W[free] * pt_free[None, :, None, None] if nf else np.zeros((0, M, 6, 3), dt)
    Y = np.einsum("jiab,ibc->jiac", Wf, Vinv)
    S = -np.einsum("jiac,kidc->jakd", Y, Wf).reshape(6 * nf, 6 * nf)
    for a, j in enumerate(free):
        S[6 * a:6 * a + 6, 6 * a:6 * a + 6] += U[j] + lam * U[j] * np.eye(6, dtype=dt)
    gpf = gp * pt_free[:, None]
    b = (np.einsum("jiac,ic->ja", Y, gpf) - gc[free]).reshape(6 * nf) if nf else np.zeros(0, dt)
    x = chol_solve(S, b) if nf else np.zeros(0, dt)
    status = int(x is None)
    dc = np.zeros((C, 6), dt)
    dp = np.zeros((M, 3), dt)
    if not status:
        if nf:
            dc[free] = x.reshape(nf, 6)
        dp = np.einsum("iab,ib->ia", Vinv, -gpf - np.einsum("jiac,ja->ic", Wf, dc[free]))
    return {"U": np.stack([u[TRIU6] for u in U]) if C else np.zeros((0, 21), dt), "gc": gc,
            "V": np.stack([v[TRIU3] for v in V]) if M else np.zeros((0, 6), dt), "gp": gp, "cost": cost.sum(),
            "S": S, "b": b, "dc": dc, "dp": dp, "n_free": nf, "status": status, "free": free, "pt_free": pt_free,
            "U_full": U, "V_full": V, "W": W, "Vs": Vs, "pt_cnt": pt_cnt}


def dense_step(prob, lam, delta=0.0):
    """The same step from the full damped system [[U*, W], [W^T, V*]] d = -[gc; gp]
    over the free cameras and the free points, solved densely (no elimination)."""
    L = linearize(prob, lam, delta)
    free, pf = L["free"], np.flatnonzero(L["pt_free"])
    nc, npt = 6 * len(free), 3 * len(pf)
    H = np.zeros((nc + npt, nc + npt))
    g = np.zeros(nc + npt)
    for a, j in enumerate(free):
        H[6 * a:6 * a + 6, 6 * a:6 * a + 6] = L["U_full"][j] * (1 + lam * np.eye(6))
        g[6 * a:6 * a + 6] = L["gc"][j]
        for q, i in enumerate(pf):
            H[6 * a:6 * a + 6, nc + 3 * q:nc + 3 * q + 3] = L["W"][j, i]
            H[nc + 3 * q:nc + 3 * q + 3, 6 * a:6 * a + 6] = L["W"][j, i].T
    for q, i in enumerate(pf):
        H[nc + 3 * q:nc + 3 * q + 3, nc + 3 * q:nc + 3 * q + 3] = L["Vs"][i]
        g[nc + 3 * q:nc + 3 * q + 3] = L["gp"][i]
    d = np.linalg.solve(H, -g)
    dc = np.zeros((len(prob["poses"]), 6))
    dp = np.zeros((len(prob["points"]), 3))
    dc[free] = d[:nc].reshape(-1, 6)
    dp[pf] = d[nc:].reshape(-1, 3)
    return dc, dp


def total_cost(poses, points, oc, op, oxy, delta=0.0, dt=np.float64):
    return obs_terms(poses, points, oc, op, oxy, delta, dt)[3].sum()


def lm(prob, delta=0.0, max_iterations=50, dt=np.float64, history=None):
    """svo_bundle_adjust's control in numpy -> (poses, points, (initial, final cost), iterations).
    Every iteration that was begun counts, the one that gives up included.
    history: a list that receives one dict per iteration: "event" ("accept",
    "reject", "small step" or "give up"), "retries" (how often lambda was raised
    because the reduced system was not positive definite), "c_cur" (the cost
    before), "c_trial" and "cost" (the cost after; for the last two events no
    trial cost exists and c_trial is None)."""
    cur = dict(prob)
    cur["poses"], cur["points"] = np.array(prob["poses"], dt), np.array(prob["points"], dt)
    oc, op, oxy = prob["obs_cam"], prob["obs_point"], prob["obs_xy"]
    c_first = c_cur = total_cost(cur["poses"], cur["points"], oc, op, oxy, delta, dt)
    lam, it = 1e-4, 0
    log = [] if history is None else history
    for it in range(1, max_iterations + 1):
        retries = 0
        L = linearize(cur, lam, delta, dt)
        while L["status"] and lam < 1e16:
            lam *= 10
            retries += 1
            L = linearize(cur, lam, delta, dt)
        if L["status"]:
            log.append({"event": "give up", "retries": retries, "c_cur": c_cur, "c_trial": None, "cost": c_cur})
            break
        free, pf = L["free"], L["pt_free"]
        step2 = (L["dc"] ** 2).sum() + (L["dp"] ** 2).sum()
        state2 = (cur["poses"][free, 9:] ** 2).sum() + (cur["points"][pf] ** 2).sum()
        if np.sqrt(step2) < 1e-12 * (1 + np.sqrt(state2)):
            log.append({"event": "small step", "retries": retries, "c_cur": c_cur, "c_trial": None, "cost": c_cur})
            break
        tp = np.array([left_update(T, d, dt) if j in free else T
                       for j, (T, d) in enumerate(zip(cur["poses"], L["dc"]))])
        tx = cur["points"] + L["dp"]
        c1 = total_cost(tp, tx, oc, op, oxy, delta, dt)
        log.append({"event": "accept" if c1 <= c_cur else "reject", "retries": retries, "c_cur": c_cur, "c_trial": c1,
                    "cost": min(c1, c_cur)})
        if c1 <= c_cur:
            cur["poses"], cur["points"] = tp, tx
            small = c_cur - c1 <= 1e-15 * c_cur
            c_cur, lam = c1, max(lam * 0.1, 1e-12)
            if small:
                break
        else:
            lam *= 10
            if lam >= 1e16:
                break
    return cur["poses"], cur["points"], (c_first, c_cur), it


def lm_prefix(prob, delta=0.0, max_iterations=14, margin=1e-6):
    """The part of the LM trajectory that rounding cannot change: B.lm in float64
    and in np.longdouble, and K = the longest prefix of iterations in which both
    precisions accept or reject alike (after the same number of lambda retries)
    and every decision is clear, |c_trial - c_cur| > margin * c_cur in both.
    -> (K, float64 history, longdouble history)."""
    h64, hld = [], []
    lm(prob, delta, max_iterations, np.float64, h64)
    lm(prob, delta, max_iterations, np.longdouble, hld)
    K = 0
    for a, b in zip(h64, hld):
        if a["event"] != b["event"] or a["retries"] != b["retries"] or a["event"] not in ("accept", "reject"):
            break
        if not all(abs(h["c_trial"] - h["c_cur"]) > margin * h["c_cur"] for h in (a, b)):
            break
        K += 1
    return K, h64, hld
