"""The place memory's rules restated on the CPU (TEST
INFRASTRUCTURE): what svo_frontend_place and svo_frontend_places_query must
return. Built on the descriptor and matcher restatement
(tests/orb_describe_reference.py) and the oracle's solvePnPRansac; nothing here
touches the GPU.

A record of a frame: every feature (x, y) of the frame's list described at octave 0
of the frame's own level-0 left image -- R.compute with one level, lscale 1, moments
on the frame, samples on its blur -- and the valid ones kept in list order with
their pixels and their map points. A query: the frame's list described and
compacted the same way, matched against every record of a frame range in both
directions, filtered; the record with the most pairs (ties: the oldest frame) gives
the pairs solvePnPRansac runs on, in ascending query index.
"""
import numpy as np

import oracle as O
import orb_describe_reference as R


def describe(img, xy, patch_size=31, pattern=None):
    """(desc (n, 32) u8, valid (n,) u8) of the list xy on img, octave 0."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    img = np.ascontiguousarray(img, np.uint8)
    desc, _, valid = R.compute([img], [R.blur(img)], [1.0], xy, np.zeros(len(xy), np.int32), patch_size, pattern)
    return desc, valid


def record(img, xy, xyz=None, patch_size=31, pattern=None):
    """The record of a frame (xyz given), or its query set (xyz None): the valid
    entries in list order."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    desc, valid = describe(img, xy, patch_size, pattern)
    keep = valid == 1
    out = dict(desc=desc[keep], xy=xy[keep])
    if xyz is not None:
        out["xyz"] = np.asarray(xyz, np.float64).reshape(-1, 3)[keep]
    return out


def match_pairs(qset, rec, ratio_pct=80, cross_check=True):
    """svo_match_hamming both ways + svo_match_filter: (m, 2) (query index, record index)."""
    iqt, dqt = R.knn2(qset["desc"], rec["desc"])
    itq = R.knn2(rec["desc"], qset["desc"])[0] if cross_check else None
    return R.match_filter(iqt, dqt, itq, ratio_pct)


def query(qset, records, t_lo, t_hi, K, ratio_pct=80, cross_check=True, min_pairs=4, iterations=100, reproj=8.0,
          confidence=0.999):
    """records: {frame: record}. -> dict of counts {frame: pairs} over the searched
    frames, frame_t (-1: no result), n_pairs (the best record's, 0 with nothing
    searched), pairs, ok, rvec, tvec, inliers (indices into pairs)."""
    searched = sorted(f for f in records if t_lo <= f <= t_hi)
    pairs = {f: match_pairs(qset, records[f], ratio_pct, cross_check) for f in searched}
    out = dict(counts={f: len(pairs[f]) for f in searched}, frame_t=-1, n_pairs=0, pairs=np.zeros((0, 2), np.int32),
               ok=False, rvec=np.zeros(3), tvec=np.zeros(3), inliers=np.zeros(0, np.int32))
    if not searched:
        return out
    best = max(searched, key=lambda f: (len(pairs[f]), -f))  # the most pairs, ties to the oldest frame
    out["n_pairs"] = len(pairs[best])
    if len(pairs[best]) < max(min_pairs, 4):
        return out
    p = pairs[best]
    rc, rv, tv, inl, _ = O.solve_pnp_ransac(records[best]["xyz"][p[:, 1]], qset["xy"][p[:, 0]], K, iterations, reproj,
                                            confidence)
    out.update(frame_t=best, pairs=p, ok=rc == 1)
    if rc == 1:
        out.update(rvec=rv, tvec=tv, inliers=inl)
    return out
