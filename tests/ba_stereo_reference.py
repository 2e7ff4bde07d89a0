"""Independent numpy restatement of the bundle adjustment with stereo
observations (CPU only), as include/svo_gpu.h states it for
svo_ba_linearize_stereo / svo_bundle_adjust_stereo: an observation may carry the
right image's column ur of a rectified pair (right camera centre at +baseline on
the left camera's x axis); ur < 0 marks a monocular observation. ba_reference's
helpers that do not know about observations (SE(3), the 3x3 inverse, Cholesky,
the scenes) are imported; everything that evaluates an observation is restated
here with the third row. Every function takes a dtype, as in ba_reference."""
import numpy as np

import ba_reference as B

BASELINE = 0.54  # m


def obs_terms(poses, points, oc, op, oxy, our, baseline, delta, dt=np.float64):
    """Per observation: in-front flag, stereo flag, residual r (n, 3), weight w,
    cost, Jc (n, 3, 6), Jp (n, 3, 3). The third row is zero for a monocular
    observation; w and cost are zero where the point is not in front."""
    T = np.asarray(poses, dt)[oc]
    R, t = T[:, :9].reshape(-1, 3, 3), T[:, 9:]
    X = np.asarray(points, dt)[op]
    Pc = np.einsum("nij,nj->ni", R, X) + t
    front = Pc[:, 2] > 0
    z = np.where(front, Pc[:, 2], dt(1))
    x, y = Pc[:, 0] / z, Pc[:, 1] / z
    fx, fy, cx, cy = dt(B.FX), dt(B.FY), dt(B.CX), dt(B.CY)
    u = np.asarray(oxy, np.float32).astype(dt)
    ur32 = np.asarray(our, np.float32)
    stereo = ur32 >= 0
    ur = ur32.astype(dt)
    xr = (Pc[:, 0] - dt(baseline)) / z
    o = np.zeros_like(z)
    s = stereo.astype(dt)
    r = np.stack([fx * x + cx - u[:, 0], fy * y + cy - u[:, 1], np.where(stereo, fx * xr + cx - ur, o)], 1)
    Jc = np.stack([np.stack([fx / z, o, -fx * x / z, -fx * x * y, fx * (1 + x * x), -fx * y], 1),
                   np.stack([o, fy / z, -fy * y / z, -fy * (1 + y * y), fy * x * y, fy * x], 1),
                   np.stack([fx / z, o, -fx * xr / z, -fx * xr * y, fx * (1 + xr * x), -fx * y], 1) * s[:, None]], 1)
    Jp = np.einsum("nak,nkc->nac", Jc[:, :, :3], R)
    nr = np.sqrt((r * r).sum(1))
    d = dt(delta)
    rob = (delta > 0) & (nr > d)
    w = np.where(rob, d / np.where(rob, nr, dt(1)), dt(1))
    cost = np.where(rob, d * (nr - dt(0.5) * d), dt(0.5) * nr * nr)
    return front, stereo, r, np.where(front, w, dt(0)), np.where(front, cost, dt(0)), Jc, Jp


def predict(T, X, baseline):
    """(u, v, ur) of one point: the function the Jacobian rows differentiate."""
    T, X = np.asarray(T, np.float64), np.asarray(X, np.float64)
    P = T[:9].reshape(3, 3) @ X + T[9:]
    return np.array([B.FX * P[0] / P[2] + B.CX, B.FY * P[1] / P[2] + B.CY, B.FX * (P[0] - baseline) / P[2] + B.CX])


def view_counts(oc, op, front, stereo, C, M):
    """Views per point: per distinct camera in front of which the point lies one,
    plus one more if any of that camera's observations of the point is stereo."""
    seen = np.zeros((M, C), bool)
    two = np.zeros((M, C), bool)
    seen[op[front], oc[front]] = True
    two[op[front & stereo], oc[front & stereo]] = True
    return seen.sum(1) + two.sum(1)


def linearize(prob, lam, delta=0.0, dt=np.float64):
    """What svo_ba_linearize_stereo returns, plus the blocks behind it."""
    poses, points = prob["poses"], prob["points"]
    oc, op = np.asarray(prob["obs_cam"]), np.asarray(prob["obs_point"])
    C, M = len(poses), len(points)
    front, stereo, r, w, cost, Jc, Jp = obs_terms(poses, points, oc, op, prob["obs_xy"], prob["obs_ur"],
                                                  prob["baseline"], delta, dt)
    U, gc = np.zeros((C, 6, 6), dt), np.zeros((C, 6), dt)
    V, gp = np.zeros((M, 3, 3), dt), np.zeros((M, 3), dt)
    W = np.zeros((C, M, 6, 3), dt)
    np.add.at(U, oc, w[:, None, None] * np.einsum("nai,naj->nij", Jc, Jc))
    np.add.at(gc, oc, w[:, None] * np.einsum("nai,na->ni", Jc, r))
    np.add.at(V, op, w[:, None, None] * np.einsum("nai,naj->nij", Jp, Jp))
    np.add.at(gp, op, w[:, None] * np.einsum("nai,na->ni", Jp, r))
    np.add.at(W, (oc, op), w[:, None, None] * np.einsum("nai,naj->nij", Jc, Jp))
    cam_cnt = np.bincount(oc[front], minlength=C)
    pt_cnt = view_counts(oc, op, front, stereo, C, M)
    lam = dt(lam)
    Vs = V + lam * V * np.eye(3, dtype=dt)
    Vinv, pd = B.inv3_sym(Vs)
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
    x = B.chol_solve(S, b) if nf else np.zeros(0, dt)
    status = int(x is None)
    dc = np.zeros((C, 6), dt)
    dp = np.zeros((M, 3), dt)
    if not status:
        if nf:
            dc[free] = x.reshape(nf, 6)
        dp = np.einsum("iab,ib->ia", Vinv, -gpf - np.einsum("jiac,ja->ic", Wf, dc[free]))
    return {"U": np.stack([u[B.TRIU6] for u in U]) if C else np.zeros((0, 21), dt), "gc": gc,
            "V": np.stack([v[B.TRIU3] for v in V]) if M else np.zeros((0, 6), dt), "gp": gp, "cost": cost.sum(),
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


def rounding_error(prob, lam, delta):
    """How far the float64 restatement of S, b, dc, dp lies from the same
    computation in np.longdouble, relative to the largest entry of each."""
    a, b = linearize(prob, lam, delta, np.float64), linearize(prob, lam, delta, np.longdouble)
    return {k: float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()) if b[k].size and np.abs(b[k]).max() > 0 else 0.0
            for k in ("S", "b", "dc", "dp")}


def total_cost(prob, poses, points, delta=0.0, dt=np.float64):
    return obs_terms(poses, points, prob["obs_cam"], prob["obs_point"], prob["obs_xy"], prob["obs_ur"],
                     prob["baseline"], delta, dt)[4].sum()


def lm(prob, delta=0.0, max_iterations=50, dt=np.float64):
    """svo_bundle_adjust_stereo's control in numpy (svo_bundle_adjust's, on the
    stereo linearisation and cost) -> (poses, points, (initial, final cost), iterations)."""
    cur = dict(prob)
    cur["poses"], cur["points"] = np.array(prob["poses"], dt), np.array(prob["points"], dt)
    c_first = c_cur = total_cost(prob, cur["poses"], cur["points"], delta, dt)
    lam, it = 1e-4, 0
    for it in range(1, max_iterations + 1):
        L = linearize(cur, lam, delta, dt)
        while L["status"] and lam < 1e16:
            lam *= 10
            L = linearize(cur, lam, delta, dt)
        if L["status"]:
            break
        free, pf = L["free"], L["pt_free"]
        step2 = (L["dc"] ** 2).sum() + (L["dp"] ** 2).sum()
        state2 = (cur["poses"][free, 9:] ** 2).sum() + (cur["points"][pf] ** 2).sum()
        if np.sqrt(step2) < 1e-12 * (1 + np.sqrt(state2)):
            break
        tp = np.array([B.left_update(T, d, dt) if j in free else T
                       for j, (T, d) in enumerate(zip(cur["poses"], L["dc"]))])
        tx = cur["points"] + L["dp"]
        c1 = total_cost(prob, tp, tx, delta, dt)
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


def batch(probs):
    """B.batch with obs_ur (P, O) beside obs_xy (-1 behind each problem's count) and the baseline."""
    q = B.batch(probs)
    q["obs_ur"] = np.full(q["obs_cam"].shape, -1.0, np.float32)
    for p, prob in enumerate(probs):
        q["obs_ur"][p, :len(prob["obs_ur"])] = prob["obs_ur"]
    q["baseline"] = probs[0]["baseline"]
    return q


def mono(prob):
    """The problem without its stereo keys: ba_reference's and the monocular entries' input."""
    return {k: v for k, v in prob.items() if k not in ("obs_ur", "baseline")}


def with_right(prob, poses, points, seed, mono_fraction=0.5, noise=0.0, outliers=0.0, baseline=BASELINE):
    """prob with a right camera: obs_ur (float32) = the projection of `points` from
    `poses` into the right image (+ N(0, noise) px, a fraction `outliers` moved by
    +-40 px), and -1 for a random fraction mono_fraction of the observations and
    for every column that would be negative (left of the right image)."""
    rng = np.random.default_rng(seed + 7000)
    q = dict(prob)
    oc, op = np.asarray(prob["obs_cam"]), np.asarray(prob["obs_point"])
    T = np.asarray(poses)[oc]
    Pc = np.einsum("nij,nj->ni", T[:, :9].reshape(-1, 3, 3), np.asarray(points)[op]) + T[:, 9:]
    ur = B.FX * (Pc[:, 0] - baseline) / Pc[:, 2] + B.CX
    if noise:
        ur = ur + rng.normal(0, noise, len(ur))
    if outliers:
        m = rng.random(len(ur)) < outliers
        ur[m] += rng.choice([-40.0, 40.0], m.sum())
    drop = (rng.random(len(ur)) < mono_fraction) | ~(ur >= 0) | ~(Pc[:, 2] > 0)
    q["obs_ur"] = np.where(drop, -1.0, ur).astype(np.float32)
    q["baseline"] = baseline
    return q


def stereo_window_scene(C=6, M=300, seed=0, mono_fraction=0.5, noise=0.0, **kw):
    """B.window_scene with a right camera (the truth; perturb it with B.perturbed,
    which carries obs_ur and baseline along)."""
    truth = B.window_scene(C, M, seed, noise=noise, **kw)
    return with_right(truth, truth["poses"], truth["points"], seed, mono_fraction, noise)


def parity_case(Cn, M, seed, outliers=0.0):
    """B.parity_case with right columns for about half of its observations,
    predicted from the (perturbed) state with 0.5 px noise and the same share of
    outliers as the left pixels."""
    q = B.parity_case(Cn, M, seed, outliers)
    return with_right(q, q["poses"], q["points"], seed, 0.5, 0.5, outliers)


def single_stereo():
    """1 fixed camera at the identity, 1 point, 1 stereo observation 1.5 px off:
    structure only, and the smallest problem in which the point is free."""
    X = np.array([[1.0, -0.5, 12.0]])
    T = np.r_[np.eye(3).ravel(), 0, 0, 0]
    uvr = predict(T, X[0], BASELINE)
    return {"poses": T[None], "points": X, "fixed": np.ones(1, np.uint8), "obs_cam": np.zeros(1, np.int32),
            "obs_point": np.zeros(1, np.int32), "obs_xy": (uvr[:2] + [0.75, -0.5])[None].astype(np.float32),
            "obs_ur": np.array([uvr[2] + 1.5], np.float32), "baseline": BASELINE}


def counting_cases():
    """name -> (problem, is point 0 free?): 2 cameras (the first fixed) and 4 points;
    points 1 - 3 are seen by both cameras, point 0 as the case says (by camera 1)."""
    base = B.perturbed(B.window_scene(C=2, M=4, seed=3, drop=0, noise=0.3, step=0.25), seed=4, n_fixed=1)
    oc, op, xy = base["obs_cam"], base["obs_point"], base["obs_xy"]
    rest = op != 0
    k1 = int(np.flatnonzero((oc == 1) & (op == 0))[0])
    T1, X0 = base["poses"][1], base["points"][0]
    ur = np.float32(predict(T1, X0, BASELINE)[2] + 0.4)
    R1, t1 = T1[:9].reshape(3, 3), T1[9:]
    behind = R1.T @ (np.array([0.3, -0.2, -3.0]) - t1)

    def make(obs, point0=None):
        q = dict(base)
        q["points"] = base["points"].copy()
        if point0 is not None:
            q["points"][0] = point0
        q["obs_cam"] = np.r_[oc[rest], [1] * len(obs)].astype(np.int32)
        q["obs_point"] = np.r_[op[rest], [0] * len(obs)].astype(np.int32)
        q["obs_xy"] = np.vstack([xy[rest]] + [(xy[k1] + np.float32(d))[None] for d, _ in obs]).astype(np.float32)
        q["obs_ur"] = np.r_[np.full(rest.sum(), -1.0), [u for _, u in obs]].astype(np.float32)
        q["baseline"] = BASELINE
        return q

    return {"one stereo observation": (make([((0, 0), ur)]), True),
            "one monocular observation": (make([((0, 0), -1.0)]), False),
            "monocular + stereo duplicates by one camera": (make([((0, 0), -1.0), ((0.5, 0.25), ur)]), True),
            "stereo + monocular duplicates by one camera": (make([((0.5, 0.25), ur), ((0, 0), -1.0)]), True),
            "stereo observation behind the camera": (make([((0, 0), ur)], behind), False)}


def boundary_duplicates(seed=0):
    """2 cameras (the first fixed), 9 points, every pair observed once, except that
    camera 1 sees each of points 3, 4 (either side of the elimination's 4-point
    staging boundary) and 7, 8 three times: monocular, stereo, monocular, and
    camera 0 sees none of them, so those four are free through the run's stereo
    observation alone."""
    prob = B.perturbed(B.window_scene(C=2, M=9, seed=seed, drop=0, noise=0.3, step=0.25), seed + 1000, n_fixed=1)
    q = with_right(prob, prob["poses"], prob["points"], seed, 0.5, 0.3)
    oc, op, xy, ur = q["obs_cam"], q["obs_point"], q["obs_xy"], q["obs_ur"]
    special = np.isin(op, (3, 4, 7, 8))
    keep = ~special
    add_c, add_p, add_xy, add_ur = [], [], [], []
    for i in (3, 4, 7, 8):
        k = int(np.flatnonzero((oc == 1) & (op == i))[0])
        u = np.float32(predict(prob["poses"][1], prob["points"][i], BASELINE)[2] - 0.3)
        for d, r in (((0.0, 0.0), -1.0), ((0.4, -0.2), u), ((-0.3, 0.1), -1.0)):
            add_c.append(1), add_p.append(i), add_xy.append(xy[k] + np.float32(d)), add_ur.append(r)
    q["obs_cam"] = np.r_[oc[keep], add_c].astype(np.int32)
    q["obs_point"] = np.r_[op[keep], add_p].astype(np.int32)
    q["obs_xy"] = np.vstack([xy[keep], np.array(add_xy)]).astype(np.float32)
    q["obs_ur"] = np.r_[ur[keep], add_ur].astype(np.float32)
    return q


def newest_keyframe_scene(seed=0, noise=0.0, C=5, M_old=60, M_new=40, depth=0.05):
    """What the feature is for. C cameras stepping 0.8 m along z, the first two
    fixed; M_old points seen by every camera, monocular except in the camera that
    created them (camera i % (C - 1): one stereo observation there, where its
    column lies in the right image); of the M_new last points those whose column
    lies in the last camera's right image are created there: one stereo
    observation each, nothing else (the others have no observation at all). The
    start: free poses off by N(0, 0.05 m) / N(0, 0.005 rad), every depth by 1 +-
    `depth`. -> (truth, start, indices of the points created at the last camera)."""
    M = M_old + M_new
    truth = B.window_scene(C, M, seed, drop=0, noise=noise)
    oc, op = truth["obs_cam"], truth["obs_point"]
    keep = (op < M_old) | (oc == C - 1)
    for k in ("obs_cam", "obs_point", "obs_xy"):
        truth[k] = truth[k][keep]
    truth = with_right(truth, truth["poses"], truth["points"], seed, 0.0, noise)
    oc, op = truth["obs_cam"], truth["obs_point"]
    keep = (op < M_old) | (truth["obs_ur"] >= 0)
    for k in ("obs_cam", "obs_point", "obs_xy", "obs_ur"):
        truth[k] = truth[k][keep]
    oc, op = truth["obs_cam"], truth["obs_point"]
    creator = np.where(op >= M_old, C - 1, op % (C - 1))
    truth["obs_ur"] = np.where(oc == creator, truth["obs_ur"], np.float32(-1)).astype(np.float32)
    new = np.unique(op[op >= M_old])
    return truth, B.perturbed(truth, seed + 1, depth=depth), new
