"""svo_match_projected's rules (include/svo_gpu.h) restated
in numpy (TEST INFRASTRUCTURE): what the device must return bit for bit. Nothing
here touches the GPU, and nothing here has a search structure: every point looks
at every keypoint.

  project          rule 1: the f64 projection, its f32 pixel, visibility
  match_projected  rules 2 and 3: candidates in the square f32 window, the two
                   smallest (distance, keypoint index)
  pairs            rule 4: the bids, each keypoint to the smallest (distance, point
                   index), (keypoint, point) in ascending keypoint
  widen            the second look of Context.relocalize_guided and
                   svo_frontend_places_widen: the map under a first pose, then the
                   oracle's solvePnPRansac on the widened pairs
"""
import numpy as np

import orb_describe_reference as R

NO_IDX, NO_DIST = -1, 257
DEFAULTS = dict(radius=4.0, max_dist=64, ratio_pct=80)


def k4_of(K):
    K = np.asarray(K, np.float64).reshape(-1)
    return K if len(K) == 4 else K.reshape(9)[[0, 4, 2, 5]]


def project(xyz, T, K, size):
    """-> (proj (n, 2) f32, visible (n,) bool). T: 12 doubles [R row-major | t]."""
    X = np.asarray(xyz, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(12)
    fx, fy, cx, cy = (np.float64(v) for v in k4_of(K))
    w, h = np.float32(size[0]), np.float32(size[1])
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        px = ((T[0] * x + T[1] * y) + T[2] * z) + T[9]
        py = ((T[3] * x + T[4] * y) + T[5] * z) + T[10]
        pz = ((T[6] * x + T[7] * y) + T[8] * z) + T[11]
        iz = 1.0 / pz
        u = fx * (px * iz) + cx
        v = fy * (py * iz) + cy
        uf, vf = u.astype(np.float32), v.astype(np.float32)
        front = pz > 0
        visible = front & (uf >= 0) & (uf < w) & (vf >= 0) & (vf < h)
    proj = np.where(front[:, None], np.stack([uf, vf], axis=1), np.float32(-1)).astype(np.float32)
    return proj, visible


def usable(kxy, size):
    k = np.asarray(kxy, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        return (k[:, 0] >= 0) & (k[:, 0] < np.float32(size[0])) & (k[:, 1] >= 0) & (k[:, 1] < np.float32(size[1]))


def match_projected(xyz, pdesc, kxy, kdesc, T, K, size, radius=4.0):
    """-> (idx (n, 2) i32, dist (n, 2) i32, proj (n, 2) f32, candidates (n,) per point)."""
    pdesc = np.asarray(pdesc, np.uint8).reshape(-1, R.DESC_BYTES)
    kdesc = np.asarray(kdesc, np.uint8).reshape(-1, R.DESC_BYTES)
    k = np.asarray(kxy, np.float32).reshape(-1, 2)
    proj, visible = project(xyz, T, K, size)
    n = len(proj)
    idx = np.full((n, 2), NO_IDX, np.int32)
    dist = np.full((n, 2), NO_DIST, np.int32)
    ncand = np.zeros(n, np.int32)
    use = usable(k, size)
    r = np.float32(radius)
    d_all = R.hamming(pdesc, kdesc) if n and len(k) else np.zeros((n, len(k)), np.int32)
    for i in np.nonzero(visible)[0]:
        with np.errstate(invalid="ignore"):
            cand = use & (np.abs(k[:, 0] - proj[i, 0]) <= r) & (np.abs(k[:, 1] - proj[i, 1]) <= r)  # f32 throughout
        js = np.nonzero(cand)[0]
        ncand[i] = len(js)
        keys = sorted((int(d_all[i, j]), int(j)) for j in js)[:2]
        for q, (d, j) in enumerate(keys):
            idx[i, q], dist[i, q] = j, d
    return idx, dist, proj, ncand


def bids(idx, dist, max_dist=64, ratio_pct=80):
    """The points that bid (rule 4), as a bool array."""
    idx = np.asarray(idx).reshape(-1, 2)
    dist = np.asarray(dist).reshape(-1, 2)
    out = np.zeros(len(idx), bool)
    for i in range(len(idx)):
        j, d1, d2 = int(idx[i, 0]), int(dist[i, 0]), int(dist[i, 1])
        out[i] = j >= 0 and d1 <= max_dist and (ratio_pct == 0 or idx[i, 1] < 0 or d1 * 100 < ratio_pct * d2)
    return out


def pairs(idx, dist, max_dist=64, ratio_pct=80):
    """-> (m, 2) i32 of (keypoint, point) in ascending keypoint."""
    won = {}
    for i in np.nonzero(bids(idx, dist, max_dist, ratio_pct))[0]:
        j, key = int(idx[i, 0]), (int(dist[i, 0]), int(i))
        if j not in won or key < won[j]:
            won[j] = key
    return np.array([(j, won[j][1]) for j in sorted(won)], np.int32).reshape(-1, 2)


def pose12(rvec, tvec):
    import oracle as O
    return np.r_[O.rodrigues(np.asarray(rvec, np.float64)).ravel(), np.asarray(tvec, np.float64).reshape(3)]


def widen(map_xyz, map_desc, kxy, kdesc, rvec, tvec, K, size, radius=4.0, max_dist=64, ratio_pct=80, iterations=100,
          reproj=8.0, confidence=0.999):
    """The map under [R(rvec) | tvec], matched, then solvePnPRansac on the pairs in
    ascending frame index -> dict of pairs (frame, map), ok, rvec, tvec, inliers
    (indices into pairs), and the counts visible / with a candidate."""
    import oracle as O
    map_xyz = np.asarray(map_xyz, np.float64).reshape(-1, 3)
    kxy = np.asarray(kxy, np.float32).reshape(-1, 2)
    idx, dist, proj, ncand = match_projected(map_xyz, map_desc, kxy, kdesc, pose12(rvec, tvec), K, size, radius)
    p = pairs(idx, dist, max_dist, ratio_pct)
    out = dict(pairs=p, ok=False, rvec=np.zeros(3), tvec=np.zeros(3), inliers=np.zeros(0, np.int32),
               visible=int(project(map_xyz, pose12(rvec, tvec), K, size)[1].sum()), with_candidate=int((ncand > 0).sum()))
    if len(p) < 4:
        return out
    rc, rv, tv, inl, _ = O.solve_pnp_ransac(map_xyz[p[:, 1]], kxy[p[:, 0]], np.asarray(K, np.float64).reshape(9),
                                            iterations, reproj, confidence)
    if rc == 1:
        out.update(ok=True, rvec=rv, tvec=tv, inliers=inl)
    return out
