"""The reprojection model and the LM rules (svo_amd/csrc/reproj_model.hpp) on the
host, under ASan + UBSan: tools/reproj_model_check.cpp built with the line at its
top, fed commands written here, its %a output compared with the numpy
restatements (tests/pose_refine_reference.py, ba_stereo_reference.py). No GPU, and
no part of the library: the header includes nothing of HIP."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ba_stereo_reference as R
import pose_refine_reference as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = np.r_[0.05, -0.02, 0.1, 0.003, -0.002, 0.001]


@pytest.fixture(scope="module")
def check():
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"  # (the library's host compiler)
    os.makedirs(os.path.join(ROOT, "tools", "bin"), exist_ok=True)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-Isvo_amd/csrc", "tools/reproj_model_check.cpp", "-o", "tools/bin/reproj_model_check"],
                          cwd=ROOT)

    def run(commands):
        """commands: lists of words and floats -> the output's lines as (tag, [floats])"""
        text = "\n".join(" ".join(w if isinstance(w, str) else float(w).hex() for w in c) for c in commands) + "\n"
        env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        out = subprocess.run([os.path.join(ROOT, "tools", "bin", "reproj_model_check")], input=text, cwd=ROOT,
                             env=env, capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "reproj_model_check: ok"
        return [(ln.split()[0], [float.fromhex(w) for w in ln.split()[1:]]) for ln in lines[:-1]]

    return run


def lin(check, stereo, T, X, xy, ur, delta):
    """-> kinds (n), r w cost (n, 5), J (n, 3, 6), the 28 sums"""
    n = len(X)
    out = check([["lin", float(stereo), delta, Q.BASELINE, float(n)], list(T)] +
                [list(X[i]) + list(xy[i]) + [ur[i]] for i in range(n)])
    assert [t for t, _ in out] == ["obs", "J"] * n + ["sums"]
    obs = np.array([v for t, v in out if t == "obs"])
    J = np.array([v for t, v in out if t == "J"]).reshape(n, 3, 6)
    return obs[:, 0].astype(int), obs[:, 1:], J, np.array(out[-1][1])


def scene(seed):
    """65 noisy observations with outliers, started NEAR off the truth: point 3 is
    behind the camera, point 7 on the optical axis, observation 11 monocular and 12 stereo."""
    X, xy, ur, T = Q.stereo_scene(65, seed, noise=0.5, outliers=0.2)
    T0 = Q.left_update(T, NEAR)
    Rm, t = T0[:9].reshape(3, 3), T0[9:]
    X[3] = Rm.T @ (np.array([0.3, -0.2, -3.0]) - t)
    X[7] = np.linalg.solve(Rm, np.array([0.0, 0.0, 10.0]) - t)
    ur[11], ur[12] = -1.0, max(ur[12], 100.0)
    return X, xy, ur, T0


@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_observation_rows_and_sums_match_the_restatement(check, delta):
    """test_reproj_gpu's bars: rows at rtol 1e-12 / atol 1e-9, the 28 sums (added in
    index order) at rtol 1e-10 / atol 1e-6."""
    X, xy, ur, T0 = scene(20)
    kind, o, J, sums = lin(check, True, T0, X, xy, ur, delta)
    front, stereo, r, w, cost, Jc = Q.terms(T0, X, xy, ur, Q.BASELINE, delta)
    assert not front[3] and front.sum() == 64 and 10 < stereo.sum() < 60 and not stereo[11] and stereo[12]
    P7 = T0[:9].reshape(3, 3) @ X[7] + T0[9:]
    assert np.abs(P7[:2]).max() < 1e-14  # on the axis
    assert np.array_equal(kind, np.where(front, 1 + stereo, 0))
    rows = np.c_[front, front, front & stereo]  # the rows an observation has
    assert np.allclose(o[:, :3][rows], r[rows], rtol=1e-12, atol=1e-9)
    assert np.allclose(J[rows], Jc[rows], rtol=1e-12, atol=1e-9)
    assert np.allclose(o[front, 3], w[front], rtol=1e-12, atol=0) and np.allclose(o[front, 4], cost[front], rtol=1e-12)
    if delta:
        assert (w[front] < 1).sum() > 5  # Huber at work
    ref = Q.linearize(T0, X, xy, ur, delta=delta)
    assert np.allclose(sums, ref, rtol=1e-10, atol=1e-6), np.abs(sums - ref).max()


@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_all_monocular_is_the_monocular_instantiation_bit_for_bit(check, delta):
    X, xy, _, T0 = scene(21)
    mono = np.full(65, -1.0, np.float32)
    k2, o2, J2, s2 = lin(check, False, T0, X, xy, mono, delta)
    k3, o3, J3, s3 = lin(check, True, T0, X, xy, mono, delta)
    assert np.array_equal(k2, k3) and set(k2) == {0, 1}
    assert np.array_equal(s2.view(np.uint64), s3.view(np.uint64))
    for a, b in ((o2[:, [0, 1, 3, 4]], o3[:, [0, 1, 3, 4]]), (J2[:, :2], J3[:, :2])):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    assert np.allclose(s2, Q.linearize(T0, X, xy, mono, delta=delta), rtol=1e-10, atol=1e-6)


def bar(f64, ld):
    """test_pose_refine_gpu's rule: 100 x the float64-to-longdouble distance of the
    restatement on the same inputs (floor 1e-12)"""
    return max(100 * float(np.abs(np.asarray(f64, np.longdouble) - ld).max()), 1e-12)


@pytest.mark.parametrize("mag", [0.0, 1e-9, 0.3])
def test_left_update_matches_the_restatement(check, mag):
    T = Q.stereo_scene(5, 22)[3]
    xi = np.r_[0.05, -0.02, 0.1, mag * np.array([2.0, -1.0, 2.0]) / 3.0]
    (tag, got), = check([["upd"] + list(xi) + list(T)])
    want, wantld = Q.left_update(T, xi), Q.left_update(T, xi, np.longdouble)
    d = np.abs(np.array(got) - want).max()
    print(f"|phi| = {mag}: distance {d:.3e}, bar {bar(want, wantld):.3e}")
    assert tag == "upd" and d <= bar(want, wantld)
    Rn = np.array(got[:9]).reshape(3, 3)
    assert np.allclose(Rn @ Rn.T, np.eye(3), atol=1e-14)


@pytest.mark.parametrize("lam", [1e-4, 1e3])
def test_solve_matches_the_restatement(check, lam):
    X, xy, ur, T0 = scene(23)
    ne = Q.linearize(T0, X, xy, ur, delta=2.0)
    (tag, got), = check([["solve", lam] + list(ne)])
    want, wantld = Q.solve(ne, lam), Q.solve(ne.astype(np.longdouble), lam, np.longdouble)
    assert tag == "solve" and got[0] == 1
    d = np.abs(np.array(got[1:]) - want).max()
    print(f"lambda = {lam}: distance {d:.3e}, bar {bar(want, wantld):.3e}")
    assert d <= bar(want, wantld)


def test_solve_refuses_an_indefinite_system(check):
    X, xy, ur, T0 = scene(23)
    ne = Q.linearize(T0, X, xy, ur)
    for k in (0, 11, 20):  # H[0][0], H[2][2], H[5][5]
        bad = ne.copy()
        bad[k] = -bad[k]
        assert Q.solve(bad, 1e-4) is None
        assert check([["solve", 1e-4] + list(bad)])[0][1][0] == 0
    assert check([["solve", 1e-4] + [float("nan")] * 28])[0][1][0] == 0


# include/svo_gpu.h, svo_refine_poses: a trial is accepted on c1 <= c0; accepted,
# lambda <- max(0.1 lambda, 1e-12) and the solver stops once c0 - c1 <= 1e-15 c0;
# rejected, lambda <- 10 lambda and the solver stops at lambda >= 1e16.
NAN = float("nan")
VERDICTS = [  # c0, c1, lambda -> accept, stop, lambda
    ((10.0, 5.0, 1e-4), (1, 0, 1e-4 * 0.1)),            # a clear accept
    ((5.0, 10.0, 1e-4), (0, 0, 1e-4 * 10)),             # a clear reject
    ((7.0, 7.0, 1e-4), (1, 1, 1e-4 * 0.1)),             # the tie: accepted, and nothing left to gain
    ((10.0, 5.0, 1e-12), (1, 0, 1e-12)),                # lambda at the floor stays there
    ((10.0, 5.0, 5e-12), (1, 0, 1e-12)),                # and does not pass below it
    ((5.0, 10.0, 1e15), (0, 1, 1e16)),                  # a reject that reaches the ceiling
    ((5.0, 10.0, 1e14), (0, 0, 1e15)),
    ((5.0, NAN, 1e-4), (0, 0, 1e-4 * 10)),              # a NaN cost is a reject
    ((1.0, 1.0 - 2.0 ** -53, 1e-3), (1, 1, 1e-3 * 0.1)),  # a fall of 1.1e-16 c0: accepted, stop
    ((1.0, 1.0 - 1e-14, 1e-3), (1, 0, 1e-3 * 0.1)),     # a fall of 1e-14 c0: go on
    ((0.0, 0.0, 1e-3), (1, 1, 1e-3 * 0.1)),             # nothing to see: cost 0 both times
]
S12 = 1e-12
SMALL = [  # |dx|^2, |t|^2 -> small: |dx| < 1e-12 (1 + |t|)
    ((S12 * S12, 0.0), 0),                               # exactly at the threshold: not small (the rule is <)
    (((S12 * (1 - 1e-9)) ** 2, 0.0), 1),
    (((S12 * (1 + 1e-9)) ** 2, 0.0), 0),
    (((4 * S12) * (4 * S12), 9.0), 0),                   # the threshold with |t| = 3
    (((3.9 * S12) ** 2, 9.0), 1),
    ((0.0, 0.0), 1),
    ((1e-6, 100.0), 0),
    ((NAN, 1.0), 0),
]


def test_lm_verdict_and_step_rule_follow_the_stated_rule(check):
    assert np.sqrt(S12 * S12) == S12 and np.sqrt((4 * S12) * (4 * S12)) == 4 * S12  # the threshold cases sit on it
    out = check([["verdict"] + list(a) for a, _ in VERDICTS] + [["small"] + list(a) for a, _ in SMALL])
    for (args, want), (tag, got) in zip(VERDICTS, out):
        assert tag == "verdict" and tuple(got) == want, (args, got, want)
    for (args, want), (tag, got) in zip(SMALL, out[len(VERDICTS):]):
        assert tag == "small" and got == [want], (args, got, want)
