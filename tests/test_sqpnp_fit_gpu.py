"""The device's final SQPnP fits by themselves (svo_sqpnp_fit device = 1 ->
launch_sqpnp_fit: sqpnp_eig_kernel, sqpnp_sqp_kernel, sqpnp_select_kernel) against
the code the front end's host pool runs from the same statistics (device = 0:
RansacSeq::fit, then Frame::pose()), bit for bit, and against the oracle's SQPnP.
The problems put the object-point mean behind the camera, so the pose or its
mirror is chosen by the positive-depth count alone: on both sides of the majority
rule, of the 2,048-inlier LDS staging limit and of a bit word's end.

pose12: the fit's Frame::pose() takes sin and cos from trig_pa.hpp (the same
operations on host and device), svo_pose_from_rvec from the maths library, so
pose12 is compared with a longdouble restatement of la::rodrigues and of -(R^T t)
within 8 * 2^-53 * (1 + sum |t|); its translation also bit for bit with its own
rotation times t summed left to right in float64 (the code's order)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import svo_amd as S
from sqpnp_stats_reference import KITTI_K as K, pack_bits, problem
from test_sqpnp_cheirality_cpu import CASES, oracle_fit

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


def _bits_eq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


class Seq:
    """One sequence of a launch: the fitted points X / uv (in order), laid out either
    as the whole sequence or as a subset picked by bits out of more slots, the rest
    NaN; every bit of the last word above the count set; a RANSAC model of its own."""

    def __init__(self, X, uv, Rt, tt, subset, seed, label=""):
        rng = np.random.default_rng(seed)
        n_in = len(X)
        self.X, self.uv, self.Rt, self.label = X, uv, Rt, label
        self.count = n_in + n_in // 2 + 5 if subset else n_in
        self.pos = np.sort(rng.choice(self.count, n_in, replace=False)) if subset else np.arange(n_in)
        self.mode = 1
        self.refused = False  # SQPnP asserts on these points: no oracle pose
        self.R = O.rodrigues(O.rodrigues_inv(Rt) + rng.normal(0, 0.01, 3)).ravel()  # not the truth, not trivial
        self.t = tt + rng.normal(0, 0.05, 3)
        self.rv = rng.normal(0, 0.1, 3)

    def place(self, obj, img, words_cap):
        obj[self.pos], img[self.pos] = self.X, self.uv
        m = np.zeros(32 * words_cap, bool)
        m[self.pos] = True
        if self.count % 32:
            m[self.count: 32 * (self.count // 32 + 1)] = True
        return pack_bits(m, words_cap)


def layout(ctx, seqs):
    """seqs placed in one batch and their statistics (one launch of svo_sqpnp_stats)
    -> obj, counts, bits, stats."""
    cap = max(q.count for q in seqs) + 3
    words_cap = (cap + 31) // 32 + 1
    obj = np.full((len(seqs), cap, 3), np.nan, np.float32)
    img = np.full((len(seqs), cap, 2), np.nan, np.float32)
    bits = np.stack([q.place(obj[s], img[s], words_cap) for s, q in enumerate(seqs)])
    counts = [q.count for q in seqs]
    return obj, counts, bits, ctx.sqpnp_stats(obj, img, counts, bits, K)


def run(ctx, seqs, device):
    """One launch of svo_sqpnp_stats and one of svo_sqpnp_fit over seqs -> pose6, pose12."""
    obj, counts, bits, stats = layout(ctx, seqs)
    return ctx.sqpnp_fit(stats, [q.mode for q in seqs], [q.R for q in seqs], [q.t for q in seqs],
                         [q.rv for q in seqs], obj, counts, bits, device=device)


def check_pose12(p6, p12):
    bound = 8 * U * (1 + np.abs(p6[3:]).sum())
    rv, t = p6[:3].astype(np.longdouble), p6[3:]
    th = np.sqrt((rv * rv).sum())
    R = np.eye(3, dtype=np.longdouble)
    if th >= 2.220446049250313e-16:  # la::rodrigues' formula, in longdouble
        k = rv / th
        kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], np.longdouble)
        R = np.cos(th) * R + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * kx
    assert float(np.abs(p12[:9].astype(np.longdouble) - R.T.ravel()).max()) <= bound
    Rt = p12[:9].reshape(3, 3)
    same_order = np.array([-((Rt[i, 0] * t[0] + Rt[i, 1] * t[1]) + Rt[i, 2] * t[2]) for i in range(3)])
    assert _bits_eq(p12[9:], same_order)
    ld = -(R.T @ t.astype(np.longdouble))
    assert float(np.abs(p12[9:].astype(np.longdouble) - ld).max()) <= bound


def _ulps(a, b):
    return (np.ascontiguousarray(a).view(np.int64) - np.ascontiguousarray(b).view(np.int64)).tolist()


def compare(ctx, seqs, oracle=True):
    """Device against host bit for bit, pose12 against pose6, and (oracle) pose6
    against O.sqpnp + rodrigues_inv on the same points within 1e-9 -> the device's
    pose6 and the largest difference from the oracle."""
    d6, d12 = run(ctx, seqs, True)
    h6, h12 = run(ctx, seqs, False)
    worst = 0.0
    for s, q in enumerate(seqs):
        assert _bits_eq(d6[s], h6[s]) and _bits_eq(d12[s], h12[s]), \
            (f"slot {s} of {len(seqs)} ({q.label}, |rvec| {np.linalg.norm(h6[s, :3]):.4f}): device - host in ulps, "
             f"pose6 {_ulps(d6[s], h6[s])} pose12 {_ulps(d12[s], h12[s])}")
        check_pose12(d6[s], d12[s])
        if oracle and q.mode == 1 and not q.refused:
            rc, Ro, to = oracle_fit(q.X, q.uv)
            assert rc == 0
            diff = max(np.abs(d6[s, :3] - O.rodrigues_inv(Ro)).max(), np.abs(d6[s, 3:] - to).max())
            worst = max(worst, diff)
            assert diff < 1e-9, f"{q.label}: {diff} from the oracle"
    return d6, worst


def majority(q, p6):
    """The discriminating property: the true pose, or (more points behind) the other one."""
    d = np.abs(O.rodrigues(p6[:3]) - q.Rt).max()
    assert (d < 1e-2) if q.nb <= q.nf else (d > 1), f"{q.label}: |R - R_true| = {d}"


def _seq(nf, nb, seed, subset, zb=40.0):
    X, uv, Rt, tt = problem(nf, nb, seed, zb)
    q = Seq(X, uv, Rt, tt, subset, 1000 * seed + nf + 3 * nb, f"nf={nf} nb={nb} seed={seed}")
    q.nf, q.nb = nf, nb
    return q


@pytest.mark.parametrize("subset", [False, True], ids=["all points", "subset of a larger cap"])
def test_device_fit_is_the_host_fit_and_the_oracles(ctx, subset):
    """Every case of test_sqpnp_cheirality_cpu.py, seeds 1-3, in shuffled order in
    launches of 1, 3 and 6 sequences. (1024, 1024) fits 2,048 points, the last size
    staged through LDS; (1025, 1024) and (1024, 1025) fit 2,049, the first unstaged.

    nf = 1024, nb = 1025, seed 2 (the mirror pose at |rvec| = 3.0179 rad) is the case
    that showed the two maths libraries' acos a double apart: rvec 1 ulp off in every
    entry with the rotation matrix and tvec equal. The fit's acos, sin and cos are
    since stated in plain arithmetic for both sides (trig_pa.hpp)."""
    seqs = [_seq(nf, nb, seed, subset, zb) for nf, nb, zb in CASES for seed in (1, 2, 3)]
    order = np.random.default_rng(5 + subset).permutation(len(seqs))
    worst, k, sizes = 0.0, 0, [1, 3, 6]
    at = 0
    while at < len(order):
        batch = [seqs[i] for i in order[at: at + sizes[k % 3]]]
        p6, w = compare(ctx, batch)
        for q, p in zip(batch, p6):
            majority(q, p)
        worst = max(worst, w)
        at += len(batch)
        k += 1
    print(f"device fit against the oracle ({'subset' if subset else 'all points'}): largest difference {worst:.3g}")


@pytest.mark.parametrize("subset", [False, True], ids=["all points", "subset of a larger cap"])
def test_fit_sizes_around_a_word_and_a_wave(ctx, subset):
    """31 .. 65 fitted points, half of them behind the camera or one more than half
    (the tail-word mask of the count, the ballot prefix of the compaction): one
    miscounted point flips the answer. And the smallest sets, 3 and 4 points."""
    seqs = [_seq(n - (n + 1) // 2, (n + 1) // 2, seed, subset) for n in (31, 32, 33, 63, 64, 65) for seed in (1, 2)]
    for at in range(0, len(seqs), 6):
        p6, _ = compare(ctx, seqs[at: at + 6])
        for q, p in zip(seqs[at: at + 6], p6):
            majority(q, p)
    # 3 and 4 points: device against host only. The front end never fits such sets (RANSAC keeps a
    # model of more than 4 inliers, and n <= 5 is solved by EPnP directly), and they are no test of
    # the 1e-9 bar: three points leave several poses of zero cost, of which host and oracle can
    # return different ones (seed 3: 21 apart), and four points are conditioned badly enough that
    # the statistics' summation order shows (seed 3: 5e-9 from the oracle, 2.7e-12 with serial sums).
    compare(ctx, [_seq(n, 0, seed, subset) for n in (3, 4) for seed in (1, 2, 3)], oracle=False)


def test_modes_mixed_in_one_launch(ctx):
    fit_a, fit_b = _seq(50, 51, 1, True), _seq(1024, 1025, 1, False)
    none, given, flat, tiny = (_seq(40, 10, 10 + k, k % 2 == 0) for k in range(4))
    none.mode, given.mode = 0, 2
    flat.uv = np.repeat(flat.uv[:1], len(flat.uv), axis=0)  # every pixel equal: SQPnP's variance assert
    # test_sqpnp_rank_assert_near_threshold's scaled-down points, on the assert side (Omega's largest
    # eigenvalue below 1e-7): the host solver and the oracle both refuse them
    tiny.X = (tiny.X.astype(np.float64) * 1e-7).astype(np.float32)
    for q in (flat, tiny):
        q.refused = True
        assert not S.solve_pnp_sqpnp(q.X.astype(np.float64), q.uv, K)[0] and oracle_fit(q.X, q.uv)[0] != 0
    assert S.solve_pnp_sqpnp(tiny.X.astype(np.float64) * 1e4, tiny.uv, K)[0]  # (the points, not the pixels)
    # which fallback each takes, from the statistics the fit gets (sqpnp_assemble / sq_null_count):
    # flat fails the point-variance test (c.ok false); tiny passes it, and Omega's largest
    # eigenvalue, at most the trace of its un-reduced form, is below 1e-7 (nn < 0)
    st = layout(ctx, [flat, tiny])[3]
    var = [(n * (n * ssq - sy * sy - sx * sx)) / n ** 3 for n, sx, sy, ssq in st[:, :4]]
    assert var[0] < 1e-5 <= var[1]
    assert 2 * st[1, [16, 19, 21]].sum() + st[1, [34, 37, 39]].sum() < 1e-7
    seqs = [fit_a, none, given, flat, tiny, fit_b]
    p6, _ = compare(ctx, seqs)
    d6, d12 = run(ctx, seqs, True)
    assert _bits_eq(p6, d6)  # a repeat gives the same bits
    assert (d6[1] == 0).all() and np.array_equal(d12[1], np.r_[np.eye(3).ravel(), 0, 0, 0])
    assert _bits_eq(d6[2], np.r_[given.rv, given.t])
    for s in (3, 4):  # the RANSAC model, as the host keeps it
        q = seqs[s]
        assert _bits_eq(d6[s, 3:], q.t) and np.abs(d6[s, :3] - O.rodrigues_inv(q.R)).max() < 1e-12
    # the ordinary fits on either side are what they are alone
    for s in (0, 5):
        alone, _ = run(ctx, [seqs[s]], True)
        assert _bits_eq(alone[0], d6[s])
        majority(seqs[s], d6[s])


def test_refused_arguments_write_nothing_and_no_sequences_is_valid(ctx):
    q = _seq(40, 10, 3, False)
    cap, words_cap = 64, 3
    obj = np.full((1, cap, 3), np.nan, np.float32)
    img = np.full((1, cap, 2), np.nan, np.float32)
    bits = q.place(obj[0], img[0], words_cap)[None]
    stats = ctx.sqpnp_stats(obj, img, [q.count], bits, K)
    f32p, f64p, i32p, u32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int, C.c_uint32))
    R, t, rv = (np.ascontiguousarray(a, np.float64) for a in (q.R, q.t, q.rv))

    def call(**kw):
        p6, p12 = np.full((1, 6), -7.0), np.full((1, 12), -7.0)
        a = dict(ctx=ctx.handle, stats=stats.ctypes.data_as(f64p), mode=[1], R=R.ctypes.data_as(f64p),
                 t=t.ctypes.data_as(f64p), rv=rv.ctypes.data_as(f64p), obj=obj.ctypes.data_as(f32p), counts=[q.count],
                 S=1, cap=cap, bits=bits.ctypes.data_as(u32p), words_cap=words_cap, device=1,
                 pose6=p6.ctypes.data_as(f64p), pose12=p12.ctypes.data_as(f64p))
        a.update(kw)
        ints = {k: None if a[k] is None else np.ascontiguousarray(a[k], np.int32) for k in ("mode", "counts")}
        ip = {k: None if v is None else v.ctypes.data_as(i32p) for k, v in ints.items()}
        rc = S.lib().svo_sqpnp_fit(a["ctx"], a["stats"], ip["mode"], a["R"], a["t"], a["rv"], a["obj"], ip["counts"],
                                   a["S"], a["cap"], a["bits"], a["words_cap"], a["device"], a["pose6"], a["pose12"])
        if rc != 0 or a["S"] == 0:
            assert (p6 == -7.0).all() and (p12 == -7.0).all()
        return rc

    assert call() == 0 and call(device=0) == 0 and call(device=0, ctx=None) == 0
    assert call(counts=[-1]) == -1 and call(counts=[cap + 1]) == -1 and call(words_cap=1) == -1
    assert call(mode=[3]) == -1 and call(mode=[-1]) == -1 and call(device=2) == -1 and call(S=-1) == -1
    for name in ("ctx", "stats", "mode", "R", "t", "rv", "obj", "counts", "bits", "pose6", "pose12"):
        assert call(**{name: None}) == -1, name
        if name != "ctx":
            assert call(device=0, **{name: None}) == -1, name
    assert call(S=0) == 0 and call(S=0, device=0) == 0
