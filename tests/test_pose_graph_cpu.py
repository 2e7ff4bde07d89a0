"""The pose-graph rule (svo_amd/csrc/pose_graph_model.hpp) on the host, under ASan +
UBSan: tools/pose_graph_model_check.cpp built with the line at its top, fed
commands written here, its %a output compared with the numpy restatement
(tests/pose_graph_reference.py). No GPU. Also the parts of the C ABI that need no
device: the refusals on a null handle, svo_pose_graph_edge, the symbols."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_graph_reference as R
import pose_refine_reference as Q
import svo_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def build_check():
    """-> run(commands): the check program's output lines as (tag, [words])"""
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"  # (the library's host compiler)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # trig_pa.hpp includes the HIP runtime's header
    os.makedirs(os.path.join(ROOT, "tools", "bin"), exist_ok=True)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-Isvo_amd/csrc",
                           "tools/pose_graph_model_check.cpp", "-o", "tools/bin/pose_graph_model_check"], cwd=ROOT)

    def run(commands):
        text = "\n".join(" ".join(w if isinstance(w, str) else float(w).hex() for w in c) for c in commands) + "\n"
        env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        out = subprocess.run([os.path.join(ROOT, "tools", "bin", "pose_graph_model_check")], input=text, cwd=ROOT,
                             env=env, capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
        lines = out.stdout.splitlines()
        assert lines[-1] == "pose_graph_model_check: ok"
        return [(ln.split()[0], ln.split()[1:]) for ln in lines[:-1]]

    return run


@pytest.fixture(scope="module")
def check():
    return build_check()


def floats(words):
    return np.array([float.fromhex(w) for w in words])


def graph_commands(poses, fixed, ij, Z, info, delta=0.0, max_iterations=0, max_cg=1024):
    poses = np.asarray(poses).reshape(-1, 12)
    return ([["graph", delta, float(max_iterations), float(max_cg), float(len(poses)), float(len(ij))]] +
            [list(poses[n]) + [float(fixed[n])] for n in range(len(poses))] +
            [[float(ij[k][0]), float(ij[k][1])] + list(Z[k]) + list(info[k]) for k in range(len(ij))])


def parse_graph(out, N, E):
    """the `graph` command's output -> dict (e, w, cost_e, Ji, Jj (E, ...), node (N, 27), cost, its: the
    iteration lines, costs, poses)"""
    g = {"e": np.zeros((E, 6)), "w": np.zeros(E), "cost_e": np.zeros(E), "Ji": np.zeros((E, 6, 6)),
         "Jj": np.zeros((E, 6, 6)), "node": np.zeros((N, 27)), "its": [], "poses": []}
    assert [t for t, _ in out[:3 * E]] == ["e", "Ji", "Jj"] * E
    for k in range(E):
        o = floats(out[3 * k][1])
        g["e"][k], g["w"][k], g["cost_e"][k] = o[:6], o[6], o[7]
        g["Ji"][k], g["Jj"][k] = floats(out[3 * k + 1][1]).reshape(6, 6), floats(out[3 * k + 2][1]).reshape(6, 6)
    rest = out[3 * E:]
    assert [t for t, _ in rest[:N + 1]] == ["node"] * N + ["cost"]
    for n in range(N):
        g["node"][n] = floats(rest[n][1])
    g["cost"] = floats(rest[N][1])[0]
    for tag, w in rest[N + 1:]:
        if tag == "it":
            g["its"].append({"event": w[0], "retries": int(w[1]), "c_cur": float.fromhex(w[2]),
                             "c_trial": float.fromhex(w[3]), "cg": int(w[4])})
        elif tag == "costs":
            g["costs"] = (float.fromhex(w[0]), float.fromhex(w[1]), int(w[2]), int(w[3]))
        else:
            assert tag == "pose"
            g["poses"].append(floats(w))
    return g


def inverse(T, dt=LD):
    return R.relative(T, np.r_[np.eye(3).ravel(), 0, 0, 0].astype(dt), dt)


def edge_with_error(seed, theta, te, dt=LD):
    """Ti, Tj at random and the Z for which E = A Z^-1 is a rotation by theta about a
    random axis with the translation te: Z = E^-1 A, formed in longdouble."""
    rng = np.random.default_rng(seed)
    Ti = Q.left_update(np.r_[np.eye(3).ravel(), rng.normal(0, 2, 3)], np.r_[0, 0, 0, rng.normal(0, 0.7, 3)])
    Tj = Q.left_update(Ti, np.r_[rng.normal(0, 1, 3), rng.normal(0, 0.3, 3)])
    ax = rng.normal(size=3)
    Ew = Q.left_update(np.r_[np.eye(3).ravel(), 0, 0, 0].astype(dt), np.r_[0, 0, 0, dt(theta) * ax / np.linalg.norm(ax)], dt)
    Ew[9:] = np.asarray(te, dt)
    Z = R.compose(inverse(Ew), R.relative(Ti, Tj, dt), dt)
    return Ti, Tj, np.asarray(Z, np.float64)


INFO = R.info_diag(0.02, 0.002)
DENSE = (lambda a: (a @ a.T + 6 * np.eye(6))[R.TRIU6])(np.random.default_rng(5).normal(size=(6, 6)))
THETAS = [1e-10, 1e-6, 0.9e-4, 1.1e-4, 1e-2, 0.39, 1.0, 2.5]


def close(got, ref, scale=1.0):
    """rtol 1e-10, and 1e-12 of the entries' scale for those that cancel to nothing"""
    return np.allclose(got, np.asarray(ref, np.float64), rtol=1e-10, atol=1e-12 * scale)


def run_edge(check, Ti, Tj, Z, info, delta):
    out = check([["edge", delta] + list(Ti) + list(Tj) + list(Z) + list(info)])
    assert [t for t, _ in out] == ["e", "Ji", "Jj"]
    o = floats(out[0][1])
    return o[:6], floats(out[1][1]).reshape(6, 6), floats(out[2][1]).reshape(6, 6), o[6], o[7]


@pytest.mark.parametrize("theta", THETAS)
def test_single_edges_match_the_restatement(check, theta):
    for seed, te, info in ((1, (0.3, -0.2, 0.1), INFO), (2, (0.0, 0.0, 0.0), DENSE)):
        Ti, Tj, Z = edge_with_error(seed, theta, te)
        e, Ji, Jj, w, cost = run_edge(check, Ti, Tj, Z, info, 0.0)
        re, rJi, rJj, rw, rcost = R.edge(Ti, Tj, Z, info, 0.0)
        scale = max(1.0, np.abs(rJi).max())
        assert np.isclose(np.linalg.norm(re[3:]), theta, rtol=1e-6, atol=1e-15)
        assert close(e, re) and close(Ji, rJi, scale) and close(Jj, rJj, scale), theta
        # (the cost's absolute bar is e's, 1e-12 per entry, through d cost = (Omega e)' de)
        assert w == 1 and np.isclose(cost, rcost, rtol=1e-10, atol=1e-12 * np.abs(R.info_matrix(info) @ re).sum())
        ld = R.edge(Ti, Tj, Z, info, 0.0, LD, series=False)  # the closed form throughout
        assert close(e, ld[0]) and close(Ji, ld[1], scale) and close(Jj, ld[2], scale), theta


def test_the_series_joins_the_closed_form_at_the_threshold():
    for th in (R.SMALL_ANGLE * (1 - 1e-9), R.SMALL_ANGLE, R.SMALL_ANGLE * (1 + 1e-9)):
        fs, ks = R.log_factors(LD(th), LD, series=True)
        fc, kc = R.log_factors(LD(th), LD, series=False)
        assert abs(fs - fc) < 1e-17 and abs(ks - kc) * th * th < 1e-18  # (k multiplies [phi]x^2)


def test_edges_on_each_side_of_the_switch_agree_with_the_closed_form(check):
    for theta in (R.SMALL_ANGLE * 0.99, R.SMALL_ANGLE * 1.01):
        Ti, Tj, Z = edge_with_error(3, theta, (0.1, 0.2, -0.3))
        e, Ji, Jj, _, _ = run_edge(check, Ti, Tj, Z, INFO, 0.0)
        ld = R.edge(Ti, Tj, Z, INFO, 0.0, LD, series=False)
        for got, ref in ((e, ld[0]), (Ji, ld[1]), (Jj, ld[2])):
            assert np.abs(got - np.asarray(ref, np.float64)).max() < 1e-14 * max(1.0, np.abs(ld[1]).max())


def test_an_edge_on_each_side_of_delta(check):
    Ti, Tj, Z = edge_with_error(4, 0.05, (0.04, -0.02, 0.01))
    s = float(np.sqrt(2 * R.edge(Ti, Tj, Z, INFO, 0.0)[4]))
    assert s > 5
    for delta, robust in ((s * 1.01, False), (s * 0.99, True), (3.0, True)):
        e, Ji, Jj, w, cost = run_edge(check, Ti, Tj, Z, INFO, delta)
        _, _, _, rw, rcost = R.edge(Ti, Tj, Z, INFO, delta)
        assert (w < 1) == robust and np.isclose(w, rw, rtol=1e-12) and np.isclose(cost, rcost, rtol=1e-12)
    assert np.isclose(w, 3.0 / s, rtol=1e-12) and np.isclose(cost, 3.0 * (s - 1.5), rtol=1e-12)


def test_an_indefinite_information_adds_nothing(check):
    Ti, Tj, Z = edge_with_error(6, 0.2, (0.3, 0.1, 0.2))
    e, Ji, Jj, w, cost = run_edge(check, Ti, Tj, Z, -INFO, 2.0)
    assert w == 0 and cost == 0 and np.all(np.isfinite(Ji)) and np.all(np.isfinite(Jj))
    assert R.edge(Ti, Tj, Z, -INFO, 2.0)[3:] == (0, 0)


def test_a_half_turn_stays_finite(check):
    """th = pi, beyond the rule: an exact half turn gives log R = 0 and finite rows."""
    I = np.r_[np.eye(3).ravel(), 0, 0, 0]
    Z = np.r_[np.diag([1.0, -1.0, -1.0]).ravel(), 0.5, 0.0, 0.0]
    e, Ji, Jj, w, cost = run_edge(check, I, I, Z, INFO, 0.0)
    assert np.all(e[3:] == 0) and np.all(np.isfinite(np.r_[e, Ji.ravel(), Jj.ravel(), cost])) and w == 1
    assert np.allclose(Jj[3:, 3:], np.eye(3))


@pytest.mark.parametrize("theta", [1e-3, 0.39, 2.0])
def test_jacobians_against_central_differences(check, theta):
    """The restatement's error in longdouble, h = 1e-6: truncation ~ h^2 = 1e-12,
    rounding ~ 1e-19 / h. The bar is 1e-9 of the rows' scale."""
    Ti, Tj, Z = edge_with_error(7, theta, (0.3, -0.2, 0.1))
    _, Ji, Jj, _, _ = run_edge(check, Ti, Tj, Z, INFO, 0.0)
    h = LD(1e-6)
    num_i, num_j = np.zeros((6, 6)), np.zeros((6, 6))
    for a in range(6):
        d = np.zeros(6, LD)
        d[a] = h
        num_i[:, a] = (R.error_of(Q.left_update(Ti, d, LD), Tj, Z) - R.error_of(Q.left_update(Ti, -d, LD), Tj, Z)) / (2 * h)
        num_j[:, a] = (R.error_of(Ti, Q.left_update(Tj, d, LD), Z) - R.error_of(Ti, Q.left_update(Tj, -d, LD), Z)) / (2 * h)
    scale = max(1.0, np.abs(num_i).max())
    di, dj = np.abs(Ji - num_i).max(), np.abs(Jj - num_j).max()
    print(f"theta {theta}: |Ji - fd| {di:.2e}, |Jj - fd| {dj:.2e}, scale {scale:.2f}")
    assert di < 1e-9 * scale and dj < 1e-9 * scale


def five_nodes():
    """5 nodes, 7 edges in no particular order: node 2 is an i and a j, node 4 has one edge."""
    sc = R.circle_scene(5, [(0, 4)], seed=11, start_noise=0.05)
    ij = np.array([(3, 2), (0, 1), (2, 0), (1, 2), (4, 3), (1, 3), (0, 2)], np.int32)
    rng = np.random.default_rng(12)
    Z = np.array([Q.left_update(R.relative(sc["truth"][i], sc["truth"][j]), np.r_[rng.normal(0, 0.02, 3), rng.normal(0, 0.01, 3)])
                  for i, j in ij])
    info = np.tile(INFO, (7, 1))
    info[3] = DENSE
    return sc["poses"], sc["fixed"], ij, Z, info


@pytest.mark.parametrize("delta", [0.0, 3.0])
def test_node_sums_match_in_the_stated_order(check, delta):
    poses, fixed, ij, Z, info = five_nodes()
    g = parse_graph(check(graph_commands(poses, fixed, ij, Z, info, delta)), 5, 7)
    ref = R.linearize(poses, ij, Z, info, delta)
    if delta:
        assert 0 < (ref["w"] < 1).sum() < 7
    assert close(g["e"], ref["e"]) and close(g["w"], ref["w"])
    assert close(g["Ji"], ref["Ji"], np.abs(ref["Ji"]).max()) and close(g["Jj"], ref["Jj"], np.abs(ref["Jj"]).max())
    assert np.isclose(g["cost"], ref["cost"], rtol=1e-10)
    # (a sum's entries cancel: the absolute bar is 1e-10 of the node's largest entry)
    for n in range(5):
        assert np.allclose(g["node"][n], ref["node"][n], rtol=1e-10, atol=1e-10 * np.abs(ref["node"][n]).max()), n
    # the order: edges 0, 2, 3, 6 at node 2, whichever end -- a serial float64 sum of the restatement's terms
    s = np.zeros(27)
    for k in (0, 2, 3, 6):
        J = ref["Ji"][k] if ij[k][0] == 2 else ref["Jj"][k]
        W = ref["w"][k] * R.info_matrix(info[k])
        s = s + np.r_[(J.T @ W @ J)[R.TRIU6], J.T @ W @ ref["e"][k]]
    assert np.allclose(g["node"][2], s, rtol=1e-10, atol=1e-10 * np.abs(s).max())


def bar(f64, ld, ref):
    """100 x the restatement's own float64-to-longdouble distance, floored at 1e-10 of the value"""
    return max(100 * float(abs(LD(f64) - ld)), 1e-10 * abs(float(ref)))


def test_one_whole_lm_of_an_8_node_loop(check):
    sc = R.circle_scene(8, [(0, 7)], seed=3)
    args = (sc["poses"], sc["fixed"], sc["ij"], sc["Z"], sc["info"])
    Kp, h64, hld, r64, rld = R.lm_prefix(*args, max_iterations=10)
    assert Kp >= 2
    g = parse_graph(check(graph_commands(*args, max_iterations=10)), 8, len(sc["ij"]))
    events = "".join(h["event"][0] for h in h64)
    got = "".join(h["event"] for h in g["its"])
    print(f"restatement {events}, host {got}, prefix {Kp}, costs {g['costs']}, restatement {r64[1]}, cg {r64[3]}")
    assert got[:Kp] == events[:Kp]
    for k in range(Kp):
        assert g["its"][k]["retries"] == h64[k]["retries"]
        b = bar(h64[k]["c_trial"], hld[k]["c_trial"], h64[k]["c_trial"])
        assert abs(g["its"][k]["c_trial"] - float(h64[k]["c_trial"])) <= b, (k, b)
    assert abs(g["costs"][0] - float(r64[1][0])) <= bar(r64[1][0], rld[1][0], r64[1][0])
    assert abs(g["costs"][1] - float(r64[1][1])) <= bar(r64[1][1], rld[1][1], r64[1][1])
    assert g["costs"][1] < 0.2 * g["costs"][0]
    if Kp == len(h64):
        assert got == events and g["costs"][2] == r64[2]


def test_the_helper_builds_a_consistent_edge(check):
    rng = np.random.default_rng(8)
    Ti = Q.left_update(np.r_[np.eye(3).ravel(), 1.0, 2.0, 3.0], rng.normal(0, 0.5, 6))
    Tj = Q.left_update(Ti, rng.normal(0, 0.5, 6))
    Z = S.Context.pose_graph_edge(Ti, Tj)
    (tag, w), = check([["rel"] + list(Ti) + list(Tj)])
    assert tag == "rel" and np.array_equal(floats(w).view(np.uint64), Z.view(np.uint64))
    assert np.allclose(Z, R.relative(Ti, Tj), rtol=1e-13, atol=1e-14)
    e = run_edge(check, Ti, Tj, Z, INFO, 0.0)[0]
    assert np.abs(e).max() < 1e-14


def test_refusals_that_need_no_device():
    """A null handle is refused before anything else, whatever the other arguments
    are: the valid call, bad counts, an index out of range, i == j. Nothing is written."""
    L = S.lib()
    f64p, i32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    poses = np.tile(np.r_[np.eye(3).ravel(), 0.0, 0.0, 0.0], (3, 1))
    fixed = np.array([1, 0, 0], np.uint8)
    Z, info = np.tile(poses[0], (2, 1)), np.tile(INFO, (2, 1))
    for ij, nn, ne in (([(0, 1), (1, 2)], 3, 2), ([(0, 1), (1, 2)], 4, 2), ([(0, 1), (1, 2)], 3, -1),
                       ([(0, 1), (1, 3)], 3, 2), ([(0, 1), (2, 2)], 3, 2)):
        ij = np.array(ij, np.int32)
        out, costs = np.full((3, 12), 7.0), np.full(2, 7.0)
        its = np.full(2, 7, np.int32)
        n_nodes, n_edges = np.array([nn], np.int32), np.array([ne], np.int32)
        rc = L.svo_pose_graph_optimize(None, 1, 3, 2, n_nodes.ctypes.data_as(i32p), n_edges.ctypes.data_as(i32p),
                                       poses.ctypes.data_as(f64p), fixed.ctypes.data_as(u8p), ij.ctypes.data_as(i32p),
                                       Z.ctypes.data_as(f64p), info.ctypes.data_as(f64p), 0.0, 5, 10,
                                       out.ctypes.data_as(f64p), costs.ctypes.data_as(f64p), its[:1].ctypes.data_as(i32p),
                                       its[1:].ctypes.data_as(i32p))
        assert rc == -1 and np.all(out == 7) and np.all(costs == 7) and np.all(its == 7)
    assert L.svo_pose_graph_linearize(None, 0, 0, 0, None, None, None, None, None, None, None, 0.0, None, None, None,
                                      None, None, None) == -1
    assert L.svo_pose_graph_time(None, 0, 0, 0, None, None, None, None, None, None, None, 0.0, 1, 1, 1, None, None,
                                 None) == -1
    assert L.svo_pose_graph_edge(None, poses.ctypes.data_as(f64p), out.ctypes.data_as(f64p)) == -1
    assert L.svo_pose_graph_edge(poses.ctypes.data_as(f64p), poses.ctypes.data_as(f64p), None) == -1


def test_symbols_are_present():
    L = S.lib()
    for name in ("svo_pose_graph_optimize", "svo_pose_graph_linearize", "svo_pose_graph_time", "svo_pose_graph_edge"):
        assert hasattr(L, name), name
    names = [s[0] for s in S._SIGS]
    assert all(n in names for n in ("svo_pose_graph_optimize", "svo_pose_graph_linearize", "svo_pose_graph_time",
                                    "svo_pose_graph_edge"))
