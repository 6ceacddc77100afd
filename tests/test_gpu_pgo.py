"""GPU tests of mulls_pgo_optimize / mulls_pgo_optimize_batch through mulls_amd/lib.py against the numpy restatement of the library's definition
(tests/pgo_restated.py): read from tests/golden/pgo_cases.npz (tests/test_pgo.py keeps the fixture equal to the restatement) and, for the small graphs,
computed again here.

Every comparison is equality of bits: poses_out, iterations, successful_steps, termination, both costs, edge_wrong and the counts.  Nothing is left to
a tolerance: every operation of the definition is + - * / sqrt in double in a stated order, and the library is built without contraction.

Ceres is not available where these tests run: nothing here was compared with Ceres itself."""
import ctypes as C
import threading

import numpy as np
import pytest

import pgo_restated as R
from mulls_amd import abi, lib
from test_pgo import bits, expected, fixture_case, golden

pytestmark = pytest.mark.gpu

INT_FIELDS = ["status", "termination", "iterations", "successful_steps", "n_free", "n_boxed", "n_fixed", "n_edges_used", "wrong_edges", "correct_reg_edges", "edges_ok"]


def c_params(p):
    return abi.pgo_params(**p)


def run(ctx, name):
    poses, fixed, stable, edges, p = fixture_case(name)
    return ctx.pgo_optimize(poses, fixed, stable, edges, c_params(p))


def check(got, want_poses, want_ints, want_costs, want_wrong, what):
    res, poses, wrong = got
    for k in INT_FIELDS:
        assert getattr(res, k) == want_ints[k], (what, k, getattr(res, k), want_ints[k])
    assert (bits([res.initial_cost, res.final_cost]) == bits(want_costs)).all(), (what, res.initial_cost, res.final_cost, list(want_costs))
    assert poses.shape == want_poses.shape
    assert (bits(poses) == bits(want_poses)).all(), (what, np.abs(poses - want_poses).max())
    assert (wrong == want_wrong).all(), what


def check_golden(ctx, name, live=False):
    got = run(ctx, name)
    poses, ints, costs, wrong, _ = expected(name)
    check(got, poses, ints, costs, wrong, name)
    if live:
        r = R.solve(*fixture_case(name))
        check(got, r["poses"], {k: r[k] for k in INT_FIELDS}, [r["initial_cost"], r["final_cost"]], r["edge_wrong"], name + " (restated here)")
    return got


def same(a, b, what):
    check(a, b[1], {k: getattr(b[0], k) for k in INT_FIELDS}, [b[0].initial_cost, b[0].final_cost], b[2], what)


@pytest.mark.parametrize("name", ["two_nodes", "chain3", "all_fixed", "one_node"])
def test_smallest_graphs(ctx_auto, name):
    res, poses, _ = check_golden(ctx_auto, name, live=True)
    if name == "two_nodes":
        # the answer is T_0 T, cost 0, as far as the step stop lets the solver go: it stops when no component of the step exceeds 1e-8, and on a
        # zero-residual problem the step not taken is the distance left (the damping at radius >= 1e4 shortens it by 1e-4 at most); 2e-8 allows for
        # the rotation's lever on the matrix entries.  The cost is then at most 0.5 lambda_max(W) |e|^2 <= 0.5 * 4e4 * 6 * (2e-8)^2 < 1e-10.
        p0, _, _, edges, _ = fixture_case(name)
        assert res.termination == abi.PGO_TERM_STEP
        assert np.abs(poses[1] - p0[0] @ edges[0][3]).max() < 2e-8 and res.final_cost < 1e-10 and res.n_fixed == 1
    if name == "all_fixed":
        assert res.iterations == 0 and res.termination == abi.PGO_TERM_NO_FREE and res.n_fixed == 4
    if name == "one_node":
        assert res.iterations == 0 and res.n_edges_used == 0


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_chains_at_the_lane_edges(ctx_auto, n):
    """both ends fixed, zero info on one edge"""
    name = "chain%d" % n
    assert not golden()[name + ".info"][n // 3].any()
    res, _, _ = check_golden(ctx_auto, name, live=n <= 65)
    assert res.n_fixed == 2 and res.n_boxed == n - 2 and res.successful_steps > 0


def test_skyline_fill(ctx_auto):
    """nested and crossing loop edges, two edges between one pair, one edge with a > b"""
    ab = golden()["loops14.ab"][:, :2].tolist()
    assert [2, 9] in ab and [3, 12] in ab and ab.count([4, 7]) == 2 and [11, 5] in ab
    check_golden(ctx_auto, "loops14", live=True)


def test_square_of_forty_submaps(ctx_auto):
    res, poses, _ = check_golden(ctx_auto, "square40")
    g = golden()
    gt, init = g["square40.gt"], g["square40.poses"]
    before = np.mean(np.linalg.norm(init[:, :3, 3] - gt[:, :3, 3], axis=1))
    after = np.mean(np.linalg.norm(poses[:, :3, 3] - gt[:, :3, 3], axis=1))
    assert after < before, (before, after)
    assert res.correct_reg_edges == 1 and res.edges_ok == 1


@pytest.mark.parametrize("name", ["w_equal", "w_diag", "loops14", "huber", "only_translation", "free_all", "skipped_edges", "consistent", "chain151"])
def test_options(ctx_auto, name):
    res, _, _ = check_golden(ctx_auto, name, live=name in ("huber", "free_all"))
    if name == "free_all":
        assert res.n_boxed == 0 and res.n_free == 13


def test_active_box(ctx_auto):
    """a closing edge 10 m off against boxes of 0.1 m per step: every boxed node's t within its box with <=, the final cost not above the initial.
    (The clamped quaternion before the last normalisation is inside its box in the restatement, tests/test_pgo.py; the device returns the restatement's bits.)"""
    res, poses, wrong = check_golden(ctx_auto, "active_box")
    init, fixed, stable, edges, p = fixture_case("active_box")
    _, _, cls, lim = R.classify(fixed, stable, edges, p)
    assert (cls[1:] == 1).all() and cls[0] == 0
    d = np.abs(poses[:, :3, 3] - init[:, :3, 3])
    assert (d <= lim[:, :1]).all()
    assert (d == lim[:, :1]).any()  # the box is active
    assert res.final_cost <= res.initial_cost
    # the closing edge, the only REGISTRATION edge, is the wrong one: no correct registration edge is left
    assert wrong.sum() == res.wrong_edges == 1 and wrong[-1] == 1 and res.correct_reg_edges == 0 and res.edges_ok == 0


@pytest.mark.parametrize("name", ["iter0", "iter1"])
def test_iteration_stops(ctx_auto, name):
    res, poses, _ = check_golden(ctx_auto, name, live=True)
    assert res.termination == abi.PGO_TERM_MAX_ITERATIONS and res.iterations == int(name[-1])
    if name == "iter0":
        assert res.final_cost == res.initial_cost


def batch_problems():
    return [fixture_case(n)[:4] for n in ("two_nodes", "chain3", "chain65", "chain151", "loops14", "early_return")]


def test_batch_equals_single_calls(ctx_auto):
    """sizes 2, 3, 65, 151, the 14-node loop graph and an early-return problem in one call: each equals its single call, also in reversed order, in
    three sub-batches (a 300 KB limit holds the first three problems; the 151-node chain needs more and runs alone; the rest follow), and with a limit
    below any problem's need"""
    probs = batch_problems()
    p = abi.pgo_params()
    singles = [ctx_auto.pgo_optimize(*q, p) for q in probs]
    assert [s[0].status for s in singles] == [1, 1, 1, 1, 1, -1]
    for what, order, limit in (("batch", range(6), 0), ("reversed", range(5, -1, -1), 0), ("three sub-batches", range(6), 300 << 10), ("one by one", range(6), 1)):
        order = list(order)
        got = ctx_auto.pgo_optimize_batch([probs[i] for i in order], p, scratch_limit=limit)
        for k, i in enumerate(order):
            same(got[k], singles[i], "%s, problem %d" % (what, i))
    assert ctx_auto.pgo_optimize_batch([], p) == []


def test_batch_of_copies(ctx_auto):
    q = fixture_case("loops14")
    got = ctx_auto.pgo_optimize_batch([q[:4]] * 64, c_params(q[4]))
    poses, ints, costs, wrong, _ = expected("loops14")
    for k in range(64):
        check(got[k], poses, ints, costs, wrong, "copy %d" % k)


def test_refusals(ctx_auto):
    poses, fixed, stable, edges, _ = fixture_case("loops14")
    p = abi.pgo_params()

    def refused(code, text, *a):
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.pgo_optimize(*a)
        assert e.value.args[1] == code and text in str(e.value), str(e.value)

    bad = poses.copy()
    bad[3, 1, 2] = np.nan
    refused(abi.MULLS_E_INVALID, "pose_init of node 3", bad, fixed, stable, edges, p)
    refused(abi.MULLS_E_INVALID, "edge 2 names a node outside", poses, fixed, stable, edges[:2] + [(1, 14, 1, np.eye(4), np.eye(6))] + edges[3:], p)
    refused(abi.MULLS_E_INVALID, "edge 0 joins a node to itself", poses, fixed, stable, [(4, 4, 1, np.eye(4), np.eye(6))] + edges[1:], p)
    inf_info = np.eye(6)
    inf_info[2, 2] = np.inf
    refused(abi.MULLS_E_INVALID, "T or info of edge 1", poses, fixed, stable, edges[:1] + [(1, 2, 1, np.eye(4), inf_info)] + edges[2:], p)
    refused(abi.MULLS_E_INVALID, "edge 3 has an unknown type", poses, fixed, stable, edges[:3] + [(3, 4, 5, np.eye(4), np.eye(6))] + edges[4:], p)
    refused(abi.MULLS_E_INVALID, "edge 0 has an unknown type", poses, fixed, stable, [(0, 1, -1, np.eye(4), np.eye(6))] + edges[1:], p)
    refused(abi.MULLS_E_INVALID, "num_iterations", poses, fixed, stable, edges, abi.pgo_params(num_iterations=1001))
    refused(abi.MULLS_E_INVALID, "negative", poses, fixed, stable, edges, abi.pgo_params(t_limit=-1.0))
    n = abi.PGO_MAX_NODES + 1
    refused(abi.MULLS_E_UNSUPPORTED, "more than 4096 nodes", np.tile(np.eye(4), (n, 1, 1)), np.ones(n), np.zeros(n), [], p)
    # a bad problem in the middle of a batch is named, and nothing is written for any problem
    nodes = [abi.pgo_nodes(q, fixed, stable) for q in (poses, bad, poses)]
    earr = abi.pgo_edges(edges)
    outs = [np.full((14, 16), 7.0) for _ in range(3)]
    arr, res = (abi.PgoProblem * 3)(), (abi.PgoResult * 3)()
    C.memset(res, 0x5A, C.sizeof(res))
    for b in range(3):
        arr[b].nodes, arr[b].n_nodes, arr[b].edges, arr[b].n_edges = C.addressof(nodes[b]), 14, C.addressof(earr), len(edges)
        arr[b].poses_out, arr[b].edge_wrong = outs[b].ctypes.data, None
    rc = ctx_auto.lib.mulls_pgo_optimize_batch(ctx_auto.h, arr, 3, C.byref(p), 0, res)
    assert rc == abi.MULLS_E_INVALID
    assert "mulls_pgo_optimize_batch: problem 1: pose_init of node 3" in ctx_auto.lib.mulls_last_error(ctx_auto.h).decode()
    assert bytes(res) == b"\x5a" * C.sizeof(res) and all((o == 7.0).all() for o in outs)
    # NULL checks come first and leave the result untouched
    r1 = abi.PgoResult()
    C.memset(C.byref(r1), 0x5A, C.sizeof(r1))
    assert ctx_auto.lib.mulls_pgo_optimize(ctx_auto.h, C.addressof(nodes[0]), 14, C.addressof(earr), len(edges), None, outs[0].ctypes.data, None, C.byref(r1)) == abi.MULLS_E_INVALID
    assert ctx_auto.lib.mulls_pgo_optimize(ctx_auto.h, C.addressof(nodes[0]), 14, C.addressof(earr), len(edges), C.byref(p), None, None, C.byref(r1)) == abi.MULLS_E_INVALID
    assert bytes(r1) == b"\x5a" * C.sizeof(r1)
    # after the refusals the context still works
    check_golden(ctx_auto, "chain3")


def test_two_contexts_on_two_threads(ctx_auto):
    """two contexts on two host threads solve different batches at once (twice each, the second time in three sub-batches: the arena regrows), with the
    bits each problem gets alone"""
    names = (["loops14", "chain65", "skipped_edges", "two_nodes", "early_return"], ["square40", "chain3", "chain64", "all_fixed", "consistent", "one_node"])
    got, errors = [None, None], []
    start = threading.Barrier(2)

    def work(k):
        try:
            c = lib.Context(0)
            try:
                probs = [fixture_case(n)[:4] for n in names[k]]
                start.wait(timeout=60)
                got[k] = [c.pgo_optimize_batch(probs, abi.pgo_params(), scratch_limit=limit) for limit in (0, 100 << 10)]
            finally:
                c.close()
        except Exception as e:  # noqa: BLE001
            start.abort()
            errors.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for k in range(2):
        for n, g0, g1 in zip(names[k], got[k][0], got[k][1]):
            poses, ints, costs, wrong, _ = expected(n)  # (these cases were generated under the default parameters)
            check(g0, poses, ints, costs, wrong, n)
            check(g1, poses, ints, costs, wrong, n + " (sub-batches)")


NODE_DTYPE = np.dtype([("pose_init", np.float64, 16), ("fixed", np.uint8), ("stable", np.uint8), ("reserved", np.uint8, 6)])
EDGE_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("type", np.int32), ("reserved", np.int32), ("T", np.float64, 16), ("info", np.float64, 36)])


def raw_call(ctx, nodes, edges, p, n_edges=None):
    """mulls_pgo_optimize on numpy records laid out as the C structs (the large graphs: no Python loop over the edges)"""
    assert NODE_DTYPE.itemsize == C.sizeof(abi.PgoNode) and EDGE_DTYPE.itemsize == C.sizeof(abi.PgoEdge)
    out, res = np.full((len(nodes), 16), 7.0), abi.PgoResult()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))
    rc = ctx.lib.mulls_pgo_optimize(ctx.h, nodes.ctypes.data, len(nodes), edges.ctypes.data, len(edges) if n_edges is None else n_edges, C.byref(p),
                                    out.ctypes.data, None, C.byref(res))
    return rc, res, out, ctx.lib.mulls_last_error(ctx.h).decode()


def chain_records(n):
    """n nodes one metre apart along x, node 0 fixed, the n - 1 chain edges, all consistent"""
    nodes, edges = np.zeros(n, NODE_DTYPE), np.zeros(n - 1, EDGE_DTYPE)
    nodes["pose_init"] = np.eye(4).reshape(-1)
    nodes["pose_init"][:, 12] = np.arange(n)
    nodes["fixed"][0] = 1
    edges["a"], edges["b"], edges["type"] = np.arange(n - 1), np.arange(1, n), abi.PGO_ADJACENT
    edges["T"] = np.eye(4).reshape(-1)
    edges["T"][:, 12] = 1.0
    edges["info"] = np.eye(6).reshape(-1)
    return nodes, edges


def long_edges(pairs):
    e = np.zeros(len(pairs), EDGE_DTYPE)
    for k, (a, b) in enumerate(pairs):
        e[k]["a"], e[k]["b"], e[k]["type"] = a, b, abi.PGO_SMOOTH
        T = np.eye(4)
        T[0, 3] = b - a
        e[k]["T"], e[k]["info"] = T.T.reshape(-1), np.eye(6).reshape(-1)
    return e


def test_capacity_edges(ctx_auto):
    """one past each limit is refused with nothing written; at the limits the problem is taken.  The skyline of a 4096-node chain with node 0 fixed has
    1 + 2 * 4094 = 8189 blocks; an edge (1, j) widens block row j - 1 from 2 blocks to j, an edge (a, j) to j - a + 1."""
    p0 = abi.pgo_params(num_iterations=0)  # the problem is checked, planned, uploaded and its cost taken; nothing is factored
    n = abi.PGO_MAX_NODES
    nodes, chain = chain_records(n)
    pairs, blocks, j = [], 8189, n - 1
    while blocks + (j - 2) <= abi.PGO_MAX_BLOCKS:
        pairs.append((1, j))
        blocks += j - 2
        j -= 1
    rest = abi.PGO_MAX_BLOCKS - blocks
    assert 0 < rest < j - 2
    pairs.append((j - 1 - rest, j))  # widens row j - 1 by exactly what is left
    assert blocks + (j - (j - 1 - rest) + 1 - 2) == abi.PGO_MAX_BLOCKS
    at_limit = np.concatenate([chain, long_edges(pairs)])
    rc, res, out, _ = raw_call(ctx_auto, nodes, at_limit, p0)
    assert rc == 0 and res.status == 1 and res.termination == abi.PGO_TERM_MAX_ITERATIONS and res.n_edges_used == len(at_limit) and res.n_fixed == 1
    assert res.initial_cost == 0.0 and (out.reshape(n, 4, 4).transpose(0, 2, 1)[:, 0, 3] == np.arange(n)).all()
    over = np.concatenate([at_limit, long_edges([(j - 3, j - 1)])])  # one block more
    rc, res, out, err = raw_call(ctx_auto, nodes, over, p0)
    assert rc == abi.MULLS_E_UNSUPPORTED and "more than 262144 blocks" in err
    assert bytes(res) == b"\x5a" * C.sizeof(res) and (out == 7.0).all()
    # edges: the count alone decides, before any edge is read
    many = np.zeros(abi.PGO_MAX_EDGES + 1, EDGE_DTYPE)
    rc, res, out, err = raw_call(ctx_auto, nodes, many, p0)
    assert rc == abi.MULLS_E_UNSUPPORTED and "more than 131072 edges" in err and bytes(res) == b"\x5a" * C.sizeof(res)
    # nodes at the limit were taken above; one more is refused in test_refusals


def test_full_graph_of_512_nodes(ctx_auto):
    """the 512-node graph with every edge, 130 816 of them and a full skyline of 131 328 blocks, which the stated capacity covers: edges from
    ground-truth poses, the start 1 cm / 0.1 degree off.  One Levenberg-Marquardt iteration on a zero-residual problem leaves what is of second order in
    the perturbation — about (2e-3 rad)^2 * 20 m against 2e-3 rad * 20 m, a cost ratio near 1e-6 — so the cost falls below a hundredth of the initial."""
    rng = np.random.default_rng(512)
    n = 512

    def small_rot(scale, m):
        w = rng.normal(size=(m, 3)) * scale
        q = np.concatenate([0.5 * w, np.ones((m, 1))], axis=1)
        return R.qrot(R.qnormalise(q))

    gt = np.tile(np.eye(4), (n, 1, 1))
    gt[:, :3, :3] = small_rot(0.3, n)
    gt[:, :3, 3] = rng.uniform(-10, 10, (n, 3))
    init = gt.copy()
    init[1:, :3, :3] = gt[1:, :3, :3] @ small_rot(1e-3, n - 1)
    init[1:, :3, 3] += rng.uniform(-0.01, 0.01, (n - 1, 3))
    a, b = np.triu_indices(n, 1)
    inv = gt.copy()
    inv[:, :3, :3] = gt[:, :3, :3].transpose(0, 2, 1)
    inv[:, :3, 3] = -np.einsum("nij,nj->ni", inv[:, :3, :3], gt[:, :3, 3])
    T = np.einsum("eij,ejk->eik", inv[a], gt[b])
    nodes, edges = np.zeros(n, NODE_DTYPE), np.zeros(len(a), EDGE_DTYPE)
    nodes["pose_init"] = init.transpose(0, 2, 1).reshape(n, 16)
    nodes["fixed"][0] = 1
    edges["a"], edges["b"], edges["type"] = a, b, abi.PGO_SMOOTH
    edges["T"] = T.transpose(0, 2, 1).reshape(-1, 16)
    edges["info"] = np.diag([1.0, 1.0, 1.0, 100.0, 100.0, 100.0]).reshape(-1)
    assert len(edges) == 130816 <= abi.PGO_MAX_EDGES
    rc, res, out, err = raw_call(ctx_auto, nodes, edges, abi.pgo_params(num_iterations=1))
    assert rc == 0, err
    print("512-node full graph: cost %.6e -> %.6e" % (res.initial_cost, res.final_cost))
    assert res.status == 1 and res.iterations == 1 and res.successful_steps == 1 and res.n_edges_used == 130816 and res.n_boxed == 511
    assert res.initial_cost > 0 and res.final_cost < 1e-2 * res.initial_cost
    poses = out.reshape(n, 4, 4).transpose(0, 2, 1)
    assert np.abs(poses - gt).max() < np.abs(init - gt).max()
