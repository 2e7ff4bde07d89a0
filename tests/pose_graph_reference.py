"""Independent numpy restatement of the pose-graph optimisation (CPU only), as
include/svo_gpu.h states it for svo_pose_graph_optimize: the edge's error and
Jacobians, the robust cost, the node sums in the stated order, the block-Jacobi
preconditioned conjugate gradients and svo_refine_poses' Levenberg-Marquardt
control. Every function takes a dtype, so the same run exists in float64 and in
np.longdouble; their distance is the rounding error the tests derive their bars
from. Also the scenes: a camera on a circle, one node per metre."""
import numpy as np

import ba_reference as B
import pose_refine_reference as Q

TRIU6 = np.triu_indices(6)
SMALL_ANGLE = 1e-4
CG_TOL = 1e-8


def mat(T, dt=np.float64):
    T = np.asarray(T, dt)
    return T[:9].reshape(3, 3), T[9:]


def vec(R, t):
    return np.r_[R.ravel(), t]


def relative(Ti, Tj, dt=np.float64):
    """Z = T_j T_i^-1"""
    Ri, ti = mat(Ti, dt)
    Rj, tj = mat(Tj, dt)
    R = Rj @ Ri.T
    return vec(R, tj - R @ ti)


def compose(Z, Ti, dt=np.float64):
    """T_j = Z T_i"""
    Rz, tz = mat(Z, dt)
    Ri, ti = mat(Ti, dt)
    return vec(Rz @ Ri, Rz @ ti + tz)


def info_matrix(info, dt=np.float64):
    Om = np.zeros((6, 6), dt)
    Om[TRIU6] = np.asarray(info, dt)
    return Om + np.triu(Om, 1).T


def info_diag(sigma_t, sigma_r):
    return np.diag(np.r_[[sigma_t ** -2.0] * 3, [sigma_r ** -2.0] * 3])[TRIU6]


def hat(v, dt):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dt)


def log_factors(th, dt=np.float64, series=None):
    """f = th / sin th and k = 1/th^2 - (1 + cos th)/(2 th sin th); their series
    below SMALL_ANGLE (series: force one form or the other)."""
    if (th < SMALL_ANGLE) if series is None else series:
        return 1 + th * th / 6, dt(1) / 12
    return th / np.sin(th), 1 / (th * th) - (1 + np.cos(th)) / (2 * th * np.sin(th))


def edge(Ti, Tj, Z, info, delta=0.0, dt=np.float64, series=None):
    """-> e (6), J_i, J_j (6, 6), w, cost"""
    A = relative(Ti, Tj, dt)
    Ra, ta = mat(A, dt)
    Re, te = mat(relative(Z, A, dt), dt)
    c = min(max((np.trace(Re) - 1) / 2, dt(-1)), dt(1))
    th = np.arccos(c)
    f, k = log_factors(th, dt, series)
    phi = f * (dt(0.5) * np.array([Re[2, 1] - Re[1, 2], Re[0, 2] - Re[2, 0], Re[1, 0] - Re[0, 1]], dt))
    e = np.r_[te, phi]
    Px = hat(phi, dt)
    Jl = np.eye(3, dtype=dt) - dt(0.5) * Px + k * (Px @ Px)
    D = np.zeros((6, 6), dt)
    D[:3, :3], D[:3, 3:], D[3:, 3:] = np.eye(3, dtype=dt), -hat(te, dt), Jl
    Ad = np.zeros((6, 6), dt)
    Ad[:3, :3], Ad[:3, 3:], Ad[3:, 3:] = Ra, hat(ta, dt) @ Ra, Ra
    q = e @ info_matrix(info, dt) @ e
    if q < 0:
        return e, -D @ Ad, D, dt(0), dt(0)
    s = np.sqrt(q)
    if delta > 0 and s > delta:
        return e, -D @ Ad, D, dt(delta) / s, dt(delta) * (s - dt(0.5) * dt(delta))
    return e, -D @ Ad, D, dt(1), dt(0.5) * q


def error_of(Ti, Tj, Z, dt=np.longdouble):
    return edge(Ti, Tj, Z, np.zeros(21), 0.0, dt)[0]


def linearize(poses, ij, Z, info, delta=0.0, dt=np.float64):
    """-> dict: cost, per edge e / w / Ji / Jj / Hij (Ji' W Jj), per node the 21 + 6
    sums over its incident edges in ascending edge index, whichever end it is."""
    poses = np.asarray(poses, dt).reshape(-1, 12)
    N, E = len(poses), len(ij)
    out = {"e": np.zeros((E, 6), dt), "w": np.zeros(E, dt), "Ji": np.zeros((E, 6, 6), dt),
           "Jj": np.zeros((E, 6, 6), dt), "Hij": np.zeros((E, 6, 6), dt), "node": np.zeros((N, 27), dt),
           "cost": dt(0)}
    for k in range(E):
        i, j = int(ij[k][0]), int(ij[k][1])
        e, Ji, Jj, w, cost = edge(poses[i], poses[j], Z[k], info[k], delta, dt)
        W = w * info_matrix(info[k], dt)
        out["e"][k], out["w"][k], out["Ji"][k], out["Jj"][k] = e, w, Ji, Jj
        out["Hij"][k] = Ji.T @ W @ Jj
        out["node"][i] += np.r_[(Ji.T @ W @ Ji)[TRIU6], Ji.T @ W @ e]
        out["node"][j] += np.r_[(Jj.T @ W @ Jj)[TRIU6], Jj.T @ W @ e]
        out["cost"] = out["cost"] + cost
    return out


def cost_of(poses, ij, Z, info, delta=0.0, dt=np.float64):
    poses = np.asarray(poses, dt).reshape(-1, 12)
    c = dt(0)
    for k in range(len(ij)):
        c = c + edge(poses[int(ij[k][0])], poses[int(ij[k][1])], Z[k], info[k], delta, dt)[4]
    return c


def chol6(A):
    """lower factor in A's dtype, None if A is not positive definite"""
    L = np.zeros_like(A)
    for j in range(6):
        s = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not s[0] > 0:
            return None
        L[j:, j] = s / np.sqrt(s[0])
    return L


def solve_step(lin, ij, fixed, lam, max_cg, dt=np.float64):
    """The damped system over the free nodes by PCG from x = 0 -> (x (N, 6),
    iterations) or (None, iterations) when a block or p'Ap is not positive."""
    N = len(lin["node"])
    free = [n for n in range(N) if not fixed[n]]
    at = {n: a for a, n in enumerate(free)}
    m = 6 * len(free)
    A, Minv, b = np.zeros((m, m), dt), np.zeros((m, m), dt), np.zeros(m, dt)
    for n in free:
        H = np.zeros((6, 6), dt)
        H[TRIU6] = lin["node"][n, :21]
        H = H + np.triu(H, 1).T
        d = np.diag(H).copy()
        H[np.diag_indices(6)] = d + dt(lam) * np.where(d > 0, d, dt(1e-12))
        L = chol6(H)
        if L is None:
            return None, 0
        Li = np.zeros((6, 6), dt)
        for c in range(6):  # L^-1 by forward substitution
            for r in range(6):
                Li[r, c] = ((r == c) - L[r, :r] @ Li[:r, c]) / L[r, r]
        s = slice(6 * at[n], 6 * at[n] + 6)
        A[s, s], Minv[s, s], b[s] = H, Li.T @ Li, -lin["node"][n, 21:]
    for k in range(len(ij)):
        i, j = int(ij[k][0]), int(ij[k][1])
        if i in at and j in at:
            si, sj = slice(6 * at[i], 6 * at[i] + 6), slice(6 * at[j], 6 * at[j] + 6)
            A[si, sj] += lin["Hij"][k]
            A[sj, si] += lin["Hij"][k].T
    x, r = np.zeros(m, dt), b.copy()
    z = Minv @ r
    p, rz = z.copy(), r @ z
    rz0, its = rz, 0
    while its < max_cg and not rz <= dt(CG_TOL) * dt(CG_TOL) * rz0:
        Ap = A @ p
        pAp = p @ Ap
        its += 1
        if not (pAp > 0 and np.isfinite(pAp)):
            return None, its
        alpha = rz / pAp
        x, r = x + alpha * p, r - alpha * Ap
        z = Minv @ r
        rzn = r @ z
        p, rz = z + (rzn / rz) * p, rzn
    full = np.zeros((N, 6), dt)
    for n in free:
        full[n] = x[6 * at[n]:6 * at[n] + 6]
    return full, its


def lm(poses, fixed, ij, Z, info, delta=0.0, max_iterations=20, max_cg=1024, dt=np.float64, history=None):
    """-> (poses (N, 12), (first, final cost), iterations, cg iterations). history
    gets one dict per iteration: event, retries, c_cur, c_trial, cost, cg."""
    cur = np.array(poses, dt).reshape(-1, 12)
    lin = linearize(cur, ij, Z, info, delta, dt)
    c_first = c0 = lin["cost"]
    lam, it, cgs = 1e-4, 0, 0
    log = [] if history is None else history
    if not (np.all(np.isfinite(cur)) and np.isfinite(c_first)):
        return cur, (np.nan, np.nan), 0, 0
    for it in range(1, max_iterations + 1):
        retries, dx = 0, None
        while lam < 1e16:
            dx, n_cg = solve_step(lin, ij, fixed, lam, max_cg, dt)
            cgs += n_cg
            if dx is not None:
                break
            lam *= 10
            retries += 1
        if dx is None:
            log.append({"event": "give up", "retries": retries, "c_cur": c0, "c_trial": None, "cost": c0, "cg": 0})
            break
        if np.sqrt((dx * dx).sum()) < 1e-12 * (1 + np.sqrt((cur[:, 9:] ** 2).sum())):
            log.append({"event": "small step", "retries": retries, "c_cur": c0, "c_trial": None, "cost": c0, "cg": n_cg})
            break
        trial = np.array([cur[n] if fixed[n] else Q.left_update(cur[n], dx[n], dt) for n in range(len(cur))])
        c1 = cost_of(trial, ij, Z, info, delta, dt)
        log.append({"event": "accept" if c1 <= c0 else "reject", "retries": retries, "c_cur": c0, "c_trial": c1,
                    "cost": min(c1, c0), "cg": n_cg})
        if c1 <= c0:
            stop = c0 - c1 <= 1e-15 * c0
            cur, c0 = trial, c1
            lin = linearize(cur, ij, Z, info, delta, dt)
            lam = max(lam * 0.1, 1e-12)
            if stop:
                break
        else:
            lam *= 10
            if lam >= 1e16:
                break
    return cur, (c_first, c0), it, cgs


def lm_prefix(poses, fixed, ij, Z, info, delta=0.0, max_iterations=10, max_cg=1024, margin=1e-6):
    """pose_refine_reference.lm_prefix for this LM: K = the longest prefix of
    iterations in which float64 and longdouble decide alike and clearly."""
    h64, hld = [], []
    r64 = lm(poses, fixed, ij, Z, info, delta, max_iterations, max_cg, np.float64, h64)
    rld = lm(poses, fixed, ij, Z, info, delta, max_iterations, max_cg, np.longdouble, hld)
    k = 0
    for a, b in zip(h64, hld):
        if a["event"] != b["event"] or a["retries"] != b["retries"] or a["event"] not in ("accept", "reject"):
            break
        if not all(abs(h["c_trial"] - h["c_cur"]) > margin * h["c_cur"] for h in (a, b)):
            break
        k += 1
    return k, h64, hld, r64, rld


# ---------------------------------------------------------------- scenes
def circle_truth(n):
    """n world -> camera poses on a circle of circumference n metres, one per metre,
    each camera looking along the tangent."""
    rad = n / (2 * np.pi)
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        centre = np.array([rad * np.cos(a), 0.0, rad * np.sin(a)])
        fwd = np.array([-np.sin(a), 0.0, np.cos(a)])
        down = np.array([0.0, 1.0, 0.0])
        R = np.stack([np.cross(down, fwd), down, fwd])  # rows: the camera's axes in the world
        out.append(vec(R, -R @ centre))
    return np.array(out)


def circle_scene(n, loops, seed=0, sigma_t=0.02, sigma_r=0.002, start_noise=0.0):
    """-> dict: truth (n, 12), poses: the chained odometry from node 0 (+ a left
    perturbation of start_noise m / rad per node), fixed (node 0), ij, Z, info.
    Odometry edges k -> k + 1 carry noise N(0, sigma_t) m and N(0, sigma_r) rad;
    the loop edges (i, j) are exact. info = diag(sigma^-2)."""
    rng = np.random.default_rng(seed)
    truth = circle_truth(n)
    ij, Z = [], []
    for k in range(n - 1):
        z = relative(truth[k], truth[k + 1])
        ij.append((k, k + 1))
        Z.append(Q.left_update(z, np.r_[rng.normal(0, sigma_t, 3), rng.normal(0, sigma_r, 3)]))
    poses = [truth[0]]
    for k in range(n - 1):
        poses.append(compose(Z[k], poses[k]))
    for i, j in loops:
        ij.append((i, j))
        Z.append(relative(truth[i], truth[j]))
    poses = np.array(poses)
    if start_noise:
        for k in range(1, n):
            poses[k] = Q.left_update(poses[k], rng.normal(0, start_noise, 6))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    info = np.tile(info_diag(sigma_t, sigma_r), (len(ij), 1))
    return {"truth": truth, "poses": poses, "fixed": fixed, "ij": np.array(ij, np.int32), "Z": np.array(Z),
            "info": info}


def position_error(poses, truth):
    """max distance between the camera centres"""
    def centre(T):
        R, t = mat(T)
        return -R.T @ t
    return max(np.linalg.norm(centre(a) - centre(b)) for a, b in zip(poses, truth))


LOOPS64 = [(0, 63), (5, 40), (20, 58)]
