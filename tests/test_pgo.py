"""CPU tests of the pose graph optimisation's definition (include/mulls_hip.h, "pose graph optimisation"): the numpy restatement tests/pgo_restated.py
on its own, the fixture tests/golden/pgo_cases.npz against it, the ctypes mirrors, the defaults, and the bridge's syntax against the reference's types.
The device is compared with the restatement bit for bit in tests/test_gpu_pgo.py.

Ceres is not available where these tests run: nothing here was compared with Ceres itself."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pgo_restated as R
from mulls_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pgo_cases.npz")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case_names():
    return [str(n) for n in golden()["names"]]


def fixture_case(name):
    """-> poses, fixed, stable, edges, params (a dict as pgo_restated.params gives)"""
    g = golden()
    ab, T, info = g[name + ".ab"], g[name + ".T"], g[name + ".info"]
    edges = [(int(ab[k, 0]), int(ab[k, 1]), int(ab[k, 2]), T[k], info[k]) for k in range(len(ab))]
    p = {str(k): v for k, v in zip(g["param_keys"], g[name + ".params"])}
    for k in p:
        if isinstance(R.DEFAULTS[k], int):
            p[k] = int(p[k])
    return g[name + ".poses"], g[name + ".fixed"], g[name + ".stable"], edges, p


def expected(name):
    g = golden()
    ints = {str(k): int(v) for k, v in zip(g["int_keys"], g[name + ".out_ints"])}
    return g[name + ".out_poses"], ints, g[name + ".out_costs"], g[name + ".out_wrong"], g[name + ".out_extra"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def restated(name):
    return R.solve(*fixture_case(name), check_systems=True)


@pytest.mark.parametrize("name", case_names())
def test_fixture_is_the_restatement(name):
    """the golden's outputs are what the restatement computes now, bit for bit; no case sits on an accept / reject edge"""
    r = restated(name)
    poses, ints, costs, wrong, extra = expected(name)
    assert (bits(r["poses"]) == bits(poses)).all()
    for k, v in ints.items():
        assert r[k] == v, k
    assert (bits([r["initial_cost"], r["final_cost"]]) == bits(costs)).all()
    assert (r["edge_wrong"] == wrong).all()
    assert r["min_ratio_distance"] > 1e-6
    # the figures the generator printed and stored are the ones a run gives now
    gt, p0 = golden()[name + ".gt"], fixture_case(name)[0]
    err0 = float(np.mean(np.linalg.norm(p0[:, :3, 3] - gt[:, :3, 3], axis=1)))
    err1 = float(np.mean(np.linalg.norm(r["poses"][:, :3, 3] - gt[:, :3, 3], axis=1)))
    assert (bits([r["min_ratio_distance"], r["max_box_excess"], err0, err1]) == bits(extra[:4])).all()


def random_state(rng):
    q = rng.normal(size=4)
    return np.concatenate([rng.normal(size=3), q / np.linalg.norm(q)])


def test_analytic_jacobians_against_central_differences():
    """h = 1e-5: truncation and rounding are both near 1e-10 for O(1) poses; the bound 1e-6 (relative to the Jacobian's largest entry) catches a wrong
    sign or factor and not noise"""
    rng = np.random.default_rng(5)
    h = 1e-5
    for _ in range(20):
        xa, xb, xe = random_state(rng), random_state(rng), random_state(rng)
        th, qh = xe[None, :3], xe[None, 3:]
        e, Rm, v, P, Q = R.residual(xa[None], xb[None], th, qh)
        Ja, Jb = R.jacobians(Rm, v, P, Q, qh)

        def moved(x, d):
            return R.step_node(x, d, x, False, 0.0, 0.0, False)[0]

        for which, J in ((0, Ja[0]), (1, Jb[0])):
            num = np.zeros((6, 6))
            for c in range(6):
                d = np.zeros(6)
                d[c] = h
                xs = [(moved(xa, s * d) if which == 0 else xa, moved(xb, s * d) if which == 1 else xb) for s in (1.0, -1.0)]
                ep = R.residual(xs[0][0][None], xs[0][1][None], th, qh)[0][0]
                em = R.residual(xs[1][0][None], xs[1][1][None], th, qh)[0][0]
                num[:, c] = (ep - em) / (2 * h)
            assert np.abs(num - J).max() <= 1e-6 * max(np.abs(J).max(), 1.0), (which, np.abs(num - J).max())


@pytest.mark.parametrize("name", case_names())
def test_restated_solve_residual(name):
    """|(H + D) delta + g| <= 1e-10 (|H + D| |delta| + |g|) for every linear system that every case solves, the later, more heavily damped and
    nearly converged ones included: Cholesky's backward error at <= 1600 unknowns is near 1e-13"""
    r = restated(name)
    res = r["solve_residuals"]
    assert len(res) <= r["iterations"] and (len(res) > 0) == (r["iterations"] > 0)
    assert all(x <= 1e-10 for x in res), max(res)


def test_consistent_graph_returns_the_ground_truth():
    """edges from ground-truth poses, the start perturbed by 0.5 m / 3 degrees.  The generator printed the error reached, 5.7e-12 m and 3.1e-13 in the
    rotation entries; they are stored, and 10 times the stored values is allowed: the values are the restatement's own rounding floor"""
    g = golden()
    r, extra = restated("consistent"), expected("consistent")[4]
    gt = g["consistent.gt"]
    terr = np.mean(np.linalg.norm(r["poses"][:, :3, 3] - gt[:, :3, 3], axis=1))
    rerr = np.abs(r["poses"][:, :3, :3] - gt[:, :3, :3]).max()
    print("translation error %.3e (stored %.3e), rotation entry error %.3e (stored %.3e), before %.3e" % (terr, extra[3], rerr, extra[4], extra[2]))
    assert extra[2] > 0.1
    assert terr <= 10 * extra[3] and rerr <= 10 * extra[4]
    assert extra[3] < 1e-9 and extra[4] < 1e-9 and r["final_cost"] < 1e-15


def I4(n):
    return np.tile(np.eye(4), (n, 1, 1))


def E(a, b, typ):
    return (a, b, typ, np.eye(4), np.eye(6))


def test_limit_rule_on_flag_patterns():
    p = R.params(t_limit=2.0, r_limit=0.05)
    # a registration edge fixes nodes 0 .. m (m = the smallest a among them) and starts stable_index at m
    edges = [E(i, i + 1, R.ADJACENT) for i in range(5)] + [E(3, 5, R.REGISTRATION), E(2, 5, R.REGISTRATION)]
    used, early, cls, lim = R.classify([0] * 6, [0] * 6, edges, p)
    assert not early and list(cls) == [0, 0, 0, 1, 1, 1]
    assert np.array_equal(lim[:, 0], [0, 0, 0, 2.0, 4.0, 6.0]) and np.array_equal(lim[:, 1], [0, 0, 0, 0.05, 2 * 0.05, 3 * 0.05])
    # stable nodes take the plain box and move stable_index
    edges = [E(i, i + 1, R.ADJACENT) for i in range(5)]
    used, early, cls, lim = R.classify([1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 1], edges, p)
    assert list(cls) == [0, 1, 1, 1, 1, 1]
    assert np.array_equal(lim[:, 0], [0, 2.0, 2.0, 2.0, 4.0, 2.0])
    # the fixed flag wins over the stable flag; a fixed node does not move stable_index
    used, early, cls, lim = R.classify([1, 0, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0], edges, p)
    assert list(cls) == [0, 1, 0, 1, 1, 1] and np.array_equal(lim[:, 0], [0, 2.0, 0, 6.0, 8.0, 10.0])
    # free_all_nodes: no box, and stable nodes do not move stable_index (nothing reads it then)
    used, early, cls, lim = R.classify([1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], edges, R.params(free_all_nodes=1))
    assert list(cls) == [0, 2, 2, 2, 2, 2] and not lim.any()
    # node 0 neither fixed nor stable, no registration edge: a box of width zero, which is a box
    edges = [E(i, i + 1, R.ADJACENT) for i in range(3)] + [E(0, 2, R.SMOOTH)]
    used, early, cls, lim = R.classify([0, 0, 0, 0], [0, 0, 0, 0], edges, p)
    assert not early and list(cls) == [1, 1, 1, 1] and lim[0, 0] == 0.0 and lim[0, 1] == 0.0 and lim[1, 0] == 2.0


def test_zero_box_keeps_the_node_at_its_start():
    poses, fixed, stable, edges, p = fixture_case("loops14")
    fixed = np.zeros_like(fixed)
    r = R.solve(poses, fixed, stable, edges, p)
    assert r["status"] == 1 and r["n_fixed"] == 0 and r["n_boxed"] == 14 and r["iterations"] > 0
    assert np.array_equal(r["poses"][0][:3, 3], poses[0][:3, 3]) and np.abs(r["poses"][0] - poses[0]).max() < 1e-15
    assert np.abs(r["poses"][5] - poses[5]).max() > 1e-4


def test_early_return():
    poses, fixed, stable, edges, p = fixture_case("early_return")
    r = restated("early_return")
    assert len(poses) - int(fixed.sum()) > len(edges)
    assert r["status"] == -1 and r["iterations"] == 0 and r["termination"] == R.TERM_NOT_RUN and r["n_edges_used"] == 1
    assert (bits(r["poses"]) == bits(poses)).all()
    # one more edge and it runs
    assert R.solve(poses, fixed, stable, edges + [E(1, 2, R.ADJACENT)], p)["status"] == 1


def test_history_and_none_edges_are_skipped():
    poses, fixed, stable, edges, p = fixture_case("skipped_edges")
    kinds = [e[2] for e in edges]
    assert R.HISTORY in kinds and R.NONE in kinds
    kept = [e for e in edges if e[2] not in (R.HISTORY, R.NONE)]
    a, b = restated("skipped_edges"), R.solve(poses, fixed, stable, kept, p)
    assert a["n_edges_used"] == len(kept) == len(edges) - 2
    assert (bits(a["poses"]) == bits(b["poses"])).all() and a["final_cost"] == b["final_cost"] and a["iterations"] == b["iterations"]
    # they are not checked either
    assert not a["edge_wrong"][[k for k, t in enumerate(kinds) if t in (R.HISTORY, R.NONE)]].any()


def test_square_loop_closure_reduces_the_error():
    extra = expected("square40")[4]
    print("mean translation error before %.3f m, after %.3f m" % (extra[2], extra[3]))
    assert extra[3] < extra[2]
    r = restated("square40")
    gt = golden()["square40.gt"]
    assert np.mean(np.linalg.norm(r["poses"][:, :3, 3] - gt[:, :3, 3], axis=1)) < np.mean(np.linalg.norm(fixture_case("square40")[0][:, :3, 3] - gt[:, :3, 3], axis=1))


def test_active_box_in_the_restatement():
    """run now, not read from the fixture: the clamped quaternion before the last normalisation never leaves its box (excess <= 0, and = 0 somewhere:
    the box is active), every boxed t lies within its box, the cost does not rise"""
    r = restated("active_box")
    init, fixed, stable, edges, p = fixture_case("active_box")
    _, _, cls, lim = R.classify(fixed, stable, edges, p)
    assert r["max_box_excess"] <= 0.0 and r["max_box_excess"] == 0.0
    assert (np.abs(r["poses"][:, :3, 3] - init[:, :3, 3]) <= lim[:, :1])[cls == 1].all()
    assert r["final_cost"] <= r["initial_cost"]


def test_defaults_match_upstream_and_the_library():
    """utility.hpp:743-791 with the values mulls_slam.cpp:170-191 passes on, as the fixture lists them; the library, the ctypes helper and the restatement agree"""
    g = golden()
    want = {str(k): float(v) for k, v in zip(g["upstream_default_names"], g["upstream_default_values"])}
    assert set(want) == set(R.DEFAULTS)
    p = abi.PgoParams()
    lib.load().mulls_pgo_default_params(C.byref(p))
    q = abi.pgo_params()
    ctype = dict(abi.PgoParams._fields_)
    for k, v in want.items():
        assert getattr(p, k) == (float(np.float32(v)) if ctype[k] is C.c_float else v), k
        assert getattr(p, k) == getattr(q, k), k
        assert float(R.DEFAULTS[k]) == v, k
    assert bytes(p) == bytes(q)


def test_ctypes_layout_matches_header():
    structs = {"mulls_pgo_node": abi.PgoNode, "mulls_pgo_edge": abi.PgoEdge, "mulls_pgo_params": abi.PgoParams, "mulls_pgo_result": abi.PgoResult,
               "mulls_pgo_problem": abi.PgoProblem}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){"]
    for cname, ct in structs.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    for cname, ct in structs.items():
        assert int(got[cname]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(ct, f).offset, (cname, f)
    assert (abi.PGO_MAX_NODES, abi.PGO_MAX_EDGES, abi.PGO_MAX_BLOCKS) == (4096, 131072, 262144)


from test_ncc import REF_UTILITY  # noqa: E402  (where the reference tree is looked for)

BRIDGE_TU = r"""
#include <chrono>
#include <cstdio>
#include "ref_shim/shim.hpp"
#include "mulls_hip.h"
#define max_(a, b) (((a) > (b)) ? (a) : (b))
#define min_(a, b) (((a) < (b)) ? (a) : (b))
using namespace std;
typedef pcl::PointXYZINormal Point_T;
typedef pcl::PointCloud<Point_T>::Ptr pcTPtr;
typedef pcl::PointCloud<Point_T> pcT;
typedef pcl::search::KdTree<Point_T>::Ptr pcTreePtr;
typedef pcl::search::KdTree<Point_T> pcTree;
#include "util_typedefs.inc"
namespace lo
{
#include "util_types.inc"
} // namespace lo
#include "cregistration_hip.hpp"
// the calls of test/mulls_slam.cpp:609 / :613 (inter-submap) and :911 / :915 (inner-submap, here for all submaps at once)
bool call(mulls_ctx *ctx, lo::cloudblock_Ptrs &cblock_submaps, lo::constraints &pgo_edges, double t_limit, double r_limit,
		  std::vector<std::pair<lo::cloudblock_Ptrs *, lo::constraints *>> &inner)
{
	mulls_pgo_params P = lo::hip::pgo_params();
	P.robustify = 0, P.num_iterations = 100;
	bool a = lo::hip::optimize_pose_graph(ctx, cblock_submaps, pgo_edges, t_limit, r_limit);
	bool b = lo::hip::optimize_pose_graph(ctx, cblock_submaps, pgo_edges, t_limit, r_limit, false, P);
	std::vector<bool> c = lo::hip::optimize_pose_graph_batch(ctx, inner, 0.1, 0.01, false, P);
	return a && b && c.size() == inner.size();
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_against_the_reference_types():
    """lo::hip::optimize_pose_graph and optimize_pose_graph_batch on the reference's cloudblock_Ptrs and constraints, as tests/test_teaser_batch.py checks its bridge"""
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 592, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(BRIDGE_TU)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
