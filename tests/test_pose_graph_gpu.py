"""svo_pose_graph_optimize: the whole Levenberg-Marquardt of a pose graph in one
launch. The linearisation against the numpy restatement
(tests/pose_graph_reference.py) and, bit for bit, against the host check program
over the same header; determinism and independence of the batch; the LM
trajectory against the restatement over the prefix in which float64 and
longdouble decide alike; what it is for (a loop closed, a wrong loop edge under
Huber, two worlds joined); the paths and the refusals."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_reference as R
import pose_refine_reference as Q
import svo_amd as S
from test_pose_graph_cpu import build_check, graph_commands, parse_graph

pytestmark = pytest.mark.gpu

IDENTITY = np.r_[np.eye(3).ravel(), 0.0, 0.0, 0.0]
INFO = R.info_diag(0.02, 0.002)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture(scope="module")
def check():
    return build_check()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def problem(sc):
    return sc["poses"], sc["fixed"], sc["ij"], sc["Z"], sc["info"]


def batch(probs, max_nodes=None, max_edges=None, fill=0.0):
    """[(poses, fixed, ij, Z, info)] -> padded arrays and the two count arrays"""
    nn = np.array([len(p[0]) for p in probs], np.int32)
    ne = np.array([len(p[2]) for p in probs], np.int32)
    N, E, P = max(int(max_nodes or nn.max()), 1), max(int(max_edges or ne.max()), 1), len(probs)
    poses, fixed = np.full((P, N, 12), fill), np.zeros((P, N), np.uint8)
    ij, Z, info = np.zeros((P, E, 2), np.int32), np.full((P, E, 12), fill), np.full((P, E, 21), fill)
    for p, (a, f, e, z, w) in enumerate(probs):
        poses[p, :len(a)], fixed[p, :len(a)] = a, f
        if len(e):
            ij[p, :len(e)], Z[p, :len(e)], info[p, :len(e)] = e, z, w
    return poses, fixed, ij, Z, info, nn, ne


def run(ctx, probs, delta=0.0, iters=20, max_cg=1024, **kw):
    poses, fixed, ij, Z, info, nn, ne = batch(probs, **kw)
    return ctx.pose_graph_optimize(poses, fixed, ij, Z, info, n_nodes=nn, n_edges=ne, huber_delta=delta,
                                   max_iterations=iters, max_cg=max_cg)


def same(a, b, p=None, q=0, n=None):
    """problem q of result a and problem p of result b (or both whole), bit for bit;
    the poses of the first n nodes (default: as many as both arrays hold)"""
    if p is None:
        return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
    n = n or min(a[0].shape[1], b[0].shape[1])
    return (np.array_equal(bits(a[0][q, :n]), bits(b[0][p, :n])) and np.array_equal(bits(a[1][q]), bits(b[1][p])) and
            a[2][q] == b[2][p] and a[3][q] == b[3][p])


def random_graph(N, E, seed, rot=0.3):
    """N poses around the origin, E edges between random distinct pairs (in no order,
    pairs repeat), measured with noise; the start is the truth perturbed; node 0 fixed."""
    rng = np.random.default_rng(seed)
    truth = np.array([Q.left_update(np.r_[np.eye(3).ravel(), rng.normal(0, 3, 3)], np.r_[0, 0, 0, rng.normal(0, rot, 3)])
                      for _ in range(N)])
    i = rng.integers(0, N, E)
    j = (i + rng.integers(1, N, E)) % N
    ij = np.c_[i, j].astype(np.int32)
    Z = np.array([Q.left_update(R.relative(truth[a], truth[b]), np.r_[rng.normal(0, 0.02, 3), rng.normal(0, 0.004, 3)])
                  for a, b in ij])
    poses = np.array([Q.left_update(T, np.r_[rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)]) for T in truth])
    info = np.tile(INFO, (E, 1))
    for k in range(0, E, 5):  # every fifth edge a dense information matrix
        a = rng.normal(size=(6, 6))
        info[k] = (a @ a.T * 50 + 100 * np.eye(6))[R.TRIU6]
    fixed = np.zeros(N, np.uint8)
    fixed[0] = 1
    return poses, fixed, ij, Z, info


# ---------------------------------------------------------------- 1. linearisation
SHAPES = [(2, 1), (3, 63), (64, 64), (65, 65), (64, 255), (257, 256), (257, 257)]  # (nodes, edges)


@pytest.fixture(scope="module")
def ragged():
    return [random_graph(N, E, 100 + k) for k, (N, E) in enumerate(SHAPES)]


@pytest.mark.parametrize("delta", [0.0, 4.0])
def test_linearisation_matches_the_restatement_and_the_host_bits(ctx, check, ragged, delta):
    """One ragged batch over the edge counts 1, 63 .. 65, 255 .. 257 and the node
    counts 2, 3, 64, 65, 257. Against numpy at rtol 1e-10 (and, for entries that
    cancel, 1e-12 of the rows' scale; the node sums 1e-10 of the node's largest
    entry); per edge e, w and both Jacobians and per node the 27 sums against the
    host program over the same header, bit for bit."""
    poses, fixed, ij, Z, info, nn, ne = batch(ragged)
    got = ctx.pose_graph_linearize(poses, fixed, ij, Z, info, n_nodes=nn, n_edges=ne, huber_delta=delta)
    robust = 0
    for p, (a, f, e, z, w) in enumerate(ragged):
        N, E = SHAPES[p]
        ref = R.linearize(a, e, z, w, delta)
        robust += int((ref["w"] < 1).sum())
        sj = max(1.0, np.abs(ref["Ji"]).max())
        assert np.allclose(got["e"][p, :E], ref["e"], rtol=1e-10, atol=1e-12), SHAPES[p]
        assert np.allclose(got["w"][p, :E], ref["w"], rtol=1e-10, atol=0), SHAPES[p]
        assert np.allclose(got["Ji"][p, :E], ref["Ji"], rtol=1e-10, atol=1e-12 * sj), SHAPES[p]
        assert np.allclose(got["Jj"][p, :E], ref["Jj"], rtol=1e-10, atol=1e-12 * sj), SHAPES[p]
        assert np.isclose(got["cost"][p], ref["cost"], rtol=1e-10), SHAPES[p]
        for n in range(N):
            assert np.allclose(got["node"][p, n], ref["node"][n], rtol=1e-10,
                               atol=1e-10 * np.abs(ref["node"][n]).max()), (SHAPES[p], n)
        host = parse_graph(check(graph_commands(a, f, e, z, w, delta)), N, E)
        for key in ("e", "w", "Ji", "Jj", "node"):
            assert np.array_equal(bits(got[key][p, :len(host[key])]), bits(host[key])), (SHAPES[p], key)
        # beyond the counts nothing is written
        assert np.all(got["e"][p, E:] == 0) and np.all(got["node"][p, N:] == 0)
    assert (robust > 50) == (delta > 0)


# ---------------------------------------------------------------- 2. determinism, independence
def star(n_leaves, seed):
    """node 0 in the middle of n_leaves edges, alternately as i and as j: an incidence
    list longer than a block"""
    poses, fixed, _, _, _ = random_graph(n_leaves + 1, 1, seed)
    rng = np.random.default_rng(seed + 1)
    ij = np.array([(0, k) if k % 2 else (k, 0) for k in range(1, n_leaves + 1)], np.int32)
    Z = np.array([Q.left_update(R.relative(poses[a], poses[b]), np.r_[rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)])
                  for a, b in ij])
    fixed[:] = 0
    fixed[1] = 1
    return poses, fixed, ij, Z, np.tile(INFO, (n_leaves, 1))


def test_results_do_not_depend_on_the_batch(ctx, check, ragged):
    solo = problem(R.circle_scene(40, [(0, 39), (4, 30)], seed=21))
    others = [ragged[2], ragged[4], star(300, 22), ragged[1]]
    a = run(ctx, [solo], delta=3.0, iters=4)
    assert a[2][0] > 1 and a[1][0, 1] < a[1][0, 0] and a[3][0] > 40
    assert same(a, run(ctx, [solo], delta=3.0, iters=4))  # two runs
    b = run(ctx, others[:3] + [solo] + others[3:], delta=3.0, iters=4)  # problem 3 of 5
    assert same(a, b, 3)
    assert same(a, run(ctx, [solo], delta=3.0, iters=4, max_nodes=100, max_edges=333), 0)  # padded
    # the star: 300 edges at one node
    s = star(300, 22)
    assert same(b, run(ctx, [s], delta=3.0, iters=4), 0, 2) and b[1][2, 1] < b[1][2, 0]
    lin = ctx.pose_graph_linearize(*s, huber_delta=3.0)
    host = parse_graph(check(graph_commands(*s, 3.0)), 301, 300)
    assert np.array_equal(bits(lin["node"]), bits(host["node"]))
    ref = R.linearize(s[0], s[2], s[3], s[4], 3.0)
    assert np.allclose(lin["node"][0], ref["node"][0], rtol=1e-10, atol=1e-10 * np.abs(ref["node"][0]).max())


# ---------------------------------------------------------------- 3. trajectory
def rough_scene():
    """24 nodes started 2 m / 2 rad off: iterations 3 - 5 of the restatement are rejected"""
    return R.circle_scene(24, [(0, 23)], seed=3, start_noise=2.0)


TRAJECTORY = {"8-nodes-1-loop": (lambda: R.circle_scene(8, [(0, 7)], seed=3), 0.0, 6),
              "64-nodes-3-loops": (lambda: R.circle_scene(64, R.LOOPS64, seed=0), 0.0, 5),
              "24-nodes-rough": (rough_scene, 0.0, 8)}


def bar(f64, ld):
    """100 x the restatement's own float64-to-longdouble distance, floored at rtol 1e-10"""
    return max(100 * float(abs(np.longdouble(f64) - ld)), 1e-10 * abs(float(f64)))


@pytest.mark.parametrize("name", list(TRAJECTORY))
def test_trajectory_follows_the_restatement(ctx, name):
    """The device keeps lambda and its verdicts to itself, so the trajectory is read
    by running from the same start with max_iterations = 1 .. K, K from R.lm_prefix.
    After k iterations a step was rejected exactly when the restatement rejected it,
    and the cost is the restatement's float64 cost within 100 x its distance to the
    longdouble run (floor rtol 1e-10): a margin for a different summation tree."""
    make, delta, iters = TRAJECTORY[name]
    sc = make()
    Kp, h64, hld, r64, rld = R.lm_prefix(*problem(sc), delta=delta, max_iterations=iters)
    assert Kp >= 2
    if name == "24-nodes-rough":
        assert "reject" in [h["event"] for h in h64[:Kp]]
    prev, pattern = None, ""
    for k in range(1, Kp + 1):
        poses, costs, its, cgs = run(ctx, [problem(sc)], delta=delta, iters=k)
        if prev is None:
            prev = costs[0, 0]
            assert abs(costs[0, 0] - float(h64[0]["c_cur"])) <= bar(h64[0]["c_cur"], hld[0]["c_cur"])
        rejected = bits(costs[0, 1]) == bits(prev)
        prev = costs[0, 1]
        pattern += "r" if rejected else "a"
        ref, b = float(h64[k - 1]["cost"]), bar(h64[k - 1]["cost"], hld[k - 1]["cost"])
        print(f"{name} k={k} {h64[k - 1]['event']}: cost {costs[0, 1]:.12e} ref {ref:.12e} diff "
              f"{abs(costs[0, 1] - ref):.3e} bar {b:.3e} (f64-ld {float(abs(h64[k - 1]['cost'] - hld[k - 1]['cost'])):.3e}) "
              f"cg {cgs[0]} ref cg {sum(h['cg'] for h in h64[:k])}")
        assert rejected == (h64[k - 1]["event"] == "reject"), (k, pattern)
        assert abs(costs[0, 1] - ref) <= b, (k, costs[0, 1], ref, b)
        assert its[0] == k


# ---------------------------------------------------------------- 4. what it is for
def test_loops_pull_the_drift_in_and_huber_holds_a_wrong_loop(ctx):
    sc = R.circle_scene(64, R.LOOPS64, seed=0)
    before = R.position_error(sc["poses"], sc["truth"])
    wrong = dict(sc)
    wrong["Z"] = sc["Z"].copy()
    k = len(sc["ij"]) - 2  # the loop edge (5, 40)
    wrong["Z"][k] = Q.left_update(sc["Z"][k], np.r_[3.0, 0.0, 1.0, 0.3 * np.array([0.0, 1.0, 0.0])])
    poses, costs, its, cgs = run(ctx, [problem(sc), problem(wrong)], iters=20)
    hub, hcosts, _, _ = run(ctx, [problem(wrong)], delta=3.0, iters=20)
    after, plain, robust = (R.position_error(p, sc["truth"]) for p in (poses[0], poses[1], hub[0]))
    print(f"max position error: odometry {before:.3f} m, optimised {after:.3f} m; with a wrong loop edge "
          f"{plain:.3f} m, under Huber 3 {robust:.3f} m; costs {costs.tolist()} {hcosts.tolist()}, cg {cgs.tolist()}")
    assert after < before and costs[0, 1] < costs[0, 0]
    assert robust < plain


# ---------------------------------------------------------------- 5. two worlds
def test_two_worlds_are_joined_by_one_loop_edge(ctx):
    """16 nodes, the chain cut between 7 and 8, nodes 8 .. 15 started from the
    identity, one loop edge 3 -> 9: a tree, so the optimum is every measurement met
    exactly -- cost 0, every node the pose composed along the edges from node 0."""
    sc = R.circle_scene(16, [], seed=31)
    ij = [tuple(e) for e in sc["ij"] if tuple(e) != (7, 8)] + [(3, 9)]
    Z = [z for e, z in zip(sc["ij"], sc["Z"]) if tuple(e) != (7, 8)] + [R.relative(sc["truth"][3], sc["truth"][9])]
    start = sc["poses"].copy()
    start[8:] = IDENTITY
    poses, costs, its, cgs = run(ctx, [(start, sc["fixed"], np.array(ij, np.int32), np.array(Z), np.tile(INFO, (15, 1)))],
                                 iters=60, max_cg=2048)
    print(f"two worlds: cost {costs[0, 0]:.3e} -> {costs[0, 1]:.3e} in {its[0]} iterations, {cgs[0]} products")
    assert costs[0, 1] < 1e-18 * costs[0, 0]
    want = {0: start[0]}
    edges = dict(zip(ij, Z))
    for k in range(1, 8):
        want[k] = R.compose(edges[(k - 1, k)], want[k - 1], np.longdouble)
    want[9] = R.compose(edges[(3, 9)], want[3], np.longdouble)
    want[8] = R.compose(R.relative(edges[(8, 9)], IDENTITY, np.longdouble), want[9], np.longdouble)  # Z_89^-1 T_9
    for k in range(10, 16):
        want[k] = R.compose(edges[(k - 1, k)], want[k - 1], np.longdouble)
    for k in range(16):
        assert np.abs(poses[0, k] - np.asarray(want[k], np.float64)).max() < 1e-8, k


# ---------------------------------------------------------------- 6. paths
def test_no_edges_one_node_and_all_fixed(ctx):
    sc = R.circle_scene(10, [(0, 9)], seed=41, start_noise=0.1)
    p, f, ij, Z, info = problem(sc)
    none = (p, f, ij[:0], Z[:0], info[:0])
    one = (p[:1], f[:1], ij[:0], Z[:0], info[:0])
    held = (p, np.ones(10, np.uint8), ij, Z, info)
    poses, costs, its, cgs = run(ctx, [none, one, held, problem(sc)], iters=10)
    for q, n in ((0, 10), (1, 1), (2, 10)):
        assert np.array_equal(bits(poses[q, :n]), bits(p[:n])), q
        assert its[q] == 1 and cgs[q] == 0 and bits(costs[q, 0]) == bits(costs[q, 1])
    assert np.all(costs[:2] == 0) and costs[2, 0] > 0
    assert costs[3, 1] < costs[3, 0] and its[3] > 1
    # max_nodes == 0 and max_edges == 0: every problem is the empty one
    p0, c0, i0, g0 = ctx.pose_graph_optimize(np.zeros((2, 0, 12)), np.zeros((2, 0), np.uint8), np.zeros((2, 0, 2), np.int32),
                                             np.zeros((2, 0, 12)), np.zeros((2, 0, 21)), max_iterations=3)
    assert p0.shape == (2, 0, 12) and np.all(c0 == 0) and list(i0) == [1, 1]
    # no problem at all
    p0, c0, i0, g0 = ctx.pose_graph_optimize(np.zeros((0, 4, 12)), np.zeros((0, 4), np.uint8), np.zeros((0, 3, 2), np.int32),
                                             np.zeros((0, 3, 12)), np.zeros((0, 3, 21)))
    assert p0.shape == (0, 4, 12) and c0.shape == (0, 2) and len(i0) == 0


def test_no_fixed_node_runs_and_the_cost_does_not_rise(ctx):
    sc = R.circle_scene(12, [(0, 11)], seed=42)
    p, f, ij, Z, info = problem(sc)
    poses, costs, its, cgs = run(ctx, [(p, np.zeros(12, np.uint8), ij, Z, info)], iters=10)
    assert costs[0, 1] <= costs[0, 0] and costs[0, 1] < 0.5 * costs[0, 0] and its[0] > 1
    assert np.all(np.isfinite(poses)) and not np.array_equal(bits(poses[0, 0]), bits(p[0]))


def test_zero_iterations_and_one_product(ctx):
    sc = R.circle_scene(12, [(0, 11)], seed=43)
    poses, costs, its, cgs = run(ctx, [problem(sc)], iters=0)
    assert np.array_equal(bits(poses[0]), bits(sc["poses"])) and bits(costs[0, 0]) == bits(costs[0, 1])
    assert its[0] == 0 and cgs[0] == 0
    assert np.isclose(costs[0, 0], R.cost_of(sc["poses"], sc["ij"], sc["Z"], sc["info"]), rtol=1e-10)
    poses, costs, its, cgs = run(ctx, [problem(sc)], iters=5, max_cg=1)  # the capped step is used as it stands
    assert its[0] >= 1 and cgs[0] <= 5 + 1 and costs[0, 1] <= costs[0, 0] and np.all(np.isfinite(poses))
    single = ctx.pose_graph_optimize(*problem(sc), max_iterations=5, max_cg=1)  # one problem without the leading axis
    assert single[0].shape == (12, 12) and np.array_equal(bits(single[0]), bits(poses[0])) and single[2] == its[0]


@pytest.mark.parametrize("where", ["pose", "Z", "info", "inf pose"])
def test_values_that_are_not_finite_stay_in_their_problem(ctx, ragged, where):
    good = [ragged[2], problem(R.circle_scene(20, [(0, 19)], seed=44))]
    p, f, ij, Z, info = [a.copy() for a in ragged[3]]
    if where == "pose":
        p[64, 10] = np.nan
    elif where == "inf pose":
        p[0, 0] = np.inf
    elif where == "Z":
        Z[64, 3] = np.nan
    else:
        info[7, 20] = np.nan
    res = run(ctx, [good[0], (p, f, ij, Z, info), good[1]], delta=3.0, iters=6)
    poses, costs, its, cgs = res
    assert np.array_equal(bits(poses[1, :65]), bits(p)) and np.all(np.isnan(costs[1])) and its[1] == 0 and cgs[1] == 0
    for q, g in ((0, good[0]), (2, good[1])):
        assert same(run(ctx, [g], delta=3.0, iters=6), res, q), q
        assert its[q] > 1 and np.all(np.isfinite(costs[q]))


def test_garbage_beyond_the_counts_is_ignored(ctx, ragged):
    g = ragged[2]
    a = run(ctx, [g], delta=3.0, iters=4, max_nodes=70, max_edges=80)
    b = run(ctx, [g], delta=3.0, iters=4, max_nodes=70, max_edges=80, fill=np.nan)
    poses, fixed, ij, Z, info, nn, ne = batch([g], 70, 80, fill=1e300)
    ij[0, 64:] = -5  # (indices beyond the count are not looked at)
    c = ctx.pose_graph_optimize(poses, fixed, ij, Z, info, n_nodes=nn, n_edges=ne, huber_delta=3.0, max_iterations=4)
    assert same(a, b, 0, n=64) and same(a, c, 0, n=64) and np.all(np.isfinite(a[1])) and a[2][0] > 1
    assert np.all(np.isnan(b[0][0, 64:]))  # the padding comes back as it came


def test_an_indefinite_information_matrix(ctx):
    """One edge with -Omega adds nothing to the cost and no weight: the result is that
    of the graph without it, to the bit where the sums see only +0 more."""
    sc = R.circle_scene(12, [(0, 11)], seed=45)
    p, f, ij, Z, info = problem(sc)
    bad = info.copy()
    bad[11] = -bad[11]  # the loop edge
    lin = ctx.pose_graph_linearize(p, f, ij, Z, bad)
    assert lin["w"][11] == 0 and np.isclose(lin["cost"], R.cost_of(p, ij[:11], Z[:11], info[:11]), rtol=1e-10)
    poses, costs, its, cgs = run(ctx, [(p, f, ij, Z, bad)], iters=10)
    want = run(ctx, [(p, f, ij[:11], Z[:11], info[:11])], iters=10)
    assert np.all(np.isfinite(poses)) and costs[0, 1] <= costs[0, 0]
    assert np.allclose(poses[0], want[0][0], rtol=0, atol=1e-9) and np.isclose(costs[0, 1], want[1][0, 1], rtol=1e-9, atol=1e-12)


def test_refused_arguments_launch_nothing(ctx):
    sc = R.circle_scene(6, [(0, 5)], seed=46)
    p, f, ij, Z, info = problem(sc)
    L = S.lib()
    f64p, i32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint8)

    def call(N=6, E=6, nn=6, ne=6, ij=ij, iters=5, cg=10, poses=p, out=True):
        ijc = np.ascontiguousarray(ij, np.int32)
        res = np.full((6, 12), 7.0), np.full(2, 7.0), np.full(2, 7, np.int32)
        n_nodes, n_edges = np.array([nn], np.int32), np.array([ne], np.int32)
        rc = L.svo_pose_graph_optimize(
            ctx.handle, 1, N, E, n_nodes.ctypes.data_as(i32p), n_edges.ctypes.data_as(i32p),
            poses.ctypes.data_as(f64p) if poses is not None else None, f.ctypes.data_as(u8p), ijc.ctypes.data_as(i32p),
            Z.ctypes.data_as(f64p), info.ctypes.data_as(f64p), 0.0, iters, cg,
            res[0].ctypes.data_as(f64p) if out else None, res[1].ctypes.data_as(f64p), res[2][:1].ctypes.data_as(i32p),
            res[2][1:].ctypes.data_as(i32p))
        return rc, L.svo_last_error(ctx.handle).decode(), res

    rc, _, res = call()
    assert rc == 0 and res[2][0] >= 1 and not np.any(res[0] == 7)
    far, loop = ij.copy(), ij.copy()
    far[5] = (0, 6)
    loop[2] = (3, 3)
    neg = ij.copy()
    neg[0] = (-1, 2)
    for kw in ({"N": 513}, {"E": 2049}, {"N": -1}, {"nn": 7}, {"nn": -1}, {"ne": 7}, {"ne": -2}, {"iters": -1},
               {"iters": 201}, {"cg": 0}, {"cg": 4097}, {"ij": far}, {"ij": loop}, {"ij": neg}, {"nn": 5},
               {"poses": None}, {"out": False}):
        rc, err, res = call(**kw)
        assert rc == -1 and err.startswith("svo_pose_graph_optimize"), (kw, err)
        assert np.all(res[0] == 7) and np.all(res[1] == 7) and np.all(res[2] == 7), kw
    with pytest.raises(S.SvoError):
        ctx.pose_graph_optimize(p, f, far, Z, info)
    with pytest.raises(S.SvoError):
        ctx.pose_graph_linearize(p, f, loop, Z, info)
    with pytest.raises(S.SvoError):
        ctx.pose_graph_time(p, f, ij, Z, info, reps=0)
    t = ctx.pose_graph_time(p, f, ij, Z, info, max_iterations=3, reps=2)
    assert t["ms"] > 0 and t["iterations"][0] >= 1
