"""CPU tests of the TEASER coarse-registration solver's definition (include/mulls_hip.h: mulls_coarse_reg_teaser) as
tests/teaser_restated.py restates it, and of the product's own code built for the CPU (tests/teaser_harness.cpp: mulls_amd/csrc/teaser_math.h, the arithmetic
the kernels compile, and teaser_host.h, the clique search and the translation estimator, around plain loops in the place of the device steps): the harness
equals the restatement bit for bit, the lexicographic clique rule against exhaustive enumeration, the budget exit, every exit of the GNC loop, the edges of
the TLS estimator, planted transforms, the ABI mirror, the bridge, and the pinned fixture tests/golden/teaser_cases.npz.  The device is compared with the
same restatement in tests/test_gpu_teaser.py.

clique_nodes is the effort of the product's search and not part of the definition; the restatement finds the clique another way and has no such number.

TEASER++ is not available where these tests run: nothing here or on the device was compared with TEASER++ itself."""
import ctypes as C
import functools
import hashlib
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import teaser_restated as tr
from mulls_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "teaser_cases.npz")
INT_KEYS = ("status", "n_edges", "max_core", "clique_size", "clique_exact", "gnc_iterations", "n_rotation_inliers", "n_translation_inliers")
LIVE_LIMIT = 300  # sets up to this size are restated again here; the larger ones are held against the fixture, which pins the restatement


@functools.lru_cache(maxsize=None)
def demo():
    return np.load(os.path.join(GOLDEN, "ncc_demo.npz"))


@functools.lru_cache(maxsize=None)
def input_sets():
    return tr.input_sets(demo())


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(FIXTURE, allow_pickle=False)


def fixture_case(name):
    Z = fixture()
    res = [int(v) for v in Z[name + "_res"]]
    keys = INT_KEYS + ("gnc_exit", "n_maximum_cliques")
    out = dict(zip(keys, res))
    out.update(T=Z[name + "_T"], cost=float(Z[name + "_cost"]), clique=Z[name + "_clique"].astype(np.int64))
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement of a set, computed once for the module"""
    t, s, nb = input_sets()[name]
    return tr.restate(t, s, nb, tr.min_inlier(name))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("teaser_harness") / "teaser_harness.so")
    subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "teaser_harness.cpp"), "-o", so])
    L = C.CDLL(so)
    L.th_weight.restype = C.c_double
    L.th_weight.argtypes = [C.c_double] * 3
    L.th_tls.restype = C.c_double
    L.th_tls.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
    L.th_search.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    L.th_gnc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p]
    L.th_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def solve(L, t, s, nb, min_inlier=8, budget=abi.TEASER_DEFAULT_NODE_BUDGET):
    n = len(t)
    ints, dbl, cl = np.zeros(10, np.int64), np.zeros(18), np.full(n + 1, -1, np.int32)
    t, s = np.ascontiguousarray(t[:, :4], np.float32), np.ascontiguousarray(s[:, :4], np.float32)
    L.th_solve(vp(s), vp(t), n, nb, min_inlier, budget, vp(ints), vp(dbl), vp(cl))
    assert cl[n] == -1
    keys = ("status", "max_core", "n_edges", "clique_size", "clique_exact", "clique_nodes", "gnc_iterations", "n_rotation_inliers", "n_translation_inliers", "kept")
    out = dict(zip(keys, (int(v) for v in ints)))
    out.update(cost=float(dbl[0]), T=dbl[2:].reshape(4, 4).T.copy(), clique=cl[: ints[3]].astype(np.int64))
    return out


def assert_same(got, want, what):
    for k in INT_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["clique"], want["clique"]), what
    assert np.float64(got["cost"]).tobytes() == np.float64(want["cost"]).tobytes(), (what, got["cost"], want["cost"])
    assert np.asarray(got["T"], np.float64).tobytes() == np.asarray(want["T"], np.float64).tobytes(), (what, got["T"], want["T"])


@pytest.mark.parametrize("name", sorted(tr.input_sets(None)) + ["demo_%s_nb%d" % (n, b) for n in tr.DEMO_LISTS for b in (25, 100)])
def test_harness_equals_restatement(harness, name):
    """every integer, the clique, and every bit of cost and T"""
    t, s, nb = input_sets()[name]
    want = restated(name) if len(t) <= LIVE_LIMIT else fixture_case(name)
    got = solve(harness, t, s, nb, tr.min_inlier(name))
    assert got["clique_exact"] == 1
    assert_same(got, want, name)


def test_fixture_pins_the_restatement():
    Z = fixture()
    assert all(Z[k].dtype.kind in "iufU" for k in Z.files) and os.path.getsize(FIXTURE) < 1 << 20
    assert sorted(input_sets()) == sorted(str(c) for c in Z["cases"])
    for name, (t, s, _) in input_sets().items():
        digest = hashlib.sha1(np.ascontiguousarray(t).tobytes() + np.ascontiguousarray(s).tobytes()).digest()
        assert bytes(Z[name + "_sha"]) == digest, name
        if len(t) <= LIVE_LIMIT:
            r, want = restated(name), fixture_case(name)
            assert_same(r, want, name)
            assert r["gnc_exit"] == want["gnc_exit"] and r["n_maximum_cliques"] == want["n_maximum_cliques"]
    # the demo rows of the issue's table: edges, largest core, clique size
    for name, row in (("demo_recip_0_15_nb25", (5398, 25, 26)), ("demo_recip_0_15_nb100", (17123, 48, 45)), ("demo_fixed300_0_15_nb25", (3397, 28, 25)),
                      ("demo_fixed300_0_15_nb100", (9155, 71, 72))):
        w = fixture_case(name)
        assert (w["n_edges"], w["max_core"], w["clique_size"]) == row, name


def test_sets_cover_the_paths():
    exits = {name: fixture_case(name)["gnc_exit"] for name in input_sets()}
    assert exits["exit_mu_exact"] == 1 and exits["exit_cost"] == 2 and exits["exit_limit"] == 0
    assert fixture_case("exit_limit")["gnc_iterations"] == 100 and 1 < fixture_case("exit_cost")["gnc_iterations"] < 100
    assert fixture_case("two_cliques")["n_maximum_cliques"] == 2 and list(fixture_case("two_cliques")["clique"]) == list(range(6))
    assert fixture_case("no_edge")["clique_size"] == 1 and fixture_case("no_edge")["status"] == -1 and fixture_case("no_edge")["n_edges"] == 0
    w = fixture_case("single_edge")
    assert w["n_edges"] == 1 and list(w["clique"]) == [5, 9] and w["n_rotation_inliers"] == 1 and w["status"] == -1
    w = fixture_case("complete_300")
    assert w["clique_size"] == 300 and w["n_edges"] == 44850 and w["n_rotation_inliers"] == 44850
    w = fixture_case("nonfinite_64")  # the pairs with a NaN or an infinity have no edge
    assert not set(w["clique"]) & {3, 4, 10, 11, 20, 21} and w["status"] == 1
    assert any(fixture_case(n)["n_maximum_cliques"] > 1 for n in input_sets() if n.startswith("demo_"))
    w = fixture_case("planted_40_90")  # a clique of 4 has 6 measurements, and the inlier count is theirs: status 1 at min_inlier_num = 3
    assert w["clique_size"] == 4 and w["n_rotation_inliers"] == 6 and w["status"] == 1
    t, s, nb = input_sets()["planted_40_90"]
    assert tr.restate(t, s, nb, 8)["status"] == -1 and tr.restate(t, s, nb, 6)["status"] == 0


# ------------------------------------------------------------------------------------------------------------------------------------------ the clique
def all_cliques(adj):
    """every clique of a small graph, by extension in ascending order"""
    n = len(adj)
    out, stack = [], [([v], [u for u in range(v + 1, n) if adj[v, u]]) for v in range(n)]
    while stack:
        R, cand = stack.pop()
        out.append(R)
        for k, u in enumerate(cand):
            stack.append((R + [u], [x for x in cand[k + 1:] if adj[u, x]]))
    return out


def bit_rows(adj):
    n = len(adj)
    W = (n + 63) // 64
    rows = np.zeros((n, W), np.uint64)
    for i, j in zip(*np.nonzero(adj)):
        rows[i, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return rows


def search(L, adj, budget=1 << 40):
    rows, cl, out = bit_rows(adj), np.full(len(adj) + 1, -1, np.int32), np.zeros(4, np.uint64)
    L.th_search(vp(rows), len(adj), budget, vp(cl), vp(out))
    return dict(clique=[int(v) for v in cl[: int(out[0])]], nodes=int(out[1]), exact=int(out[2]), lb=int(out[3]))


def random_graph(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 25))
    up = np.triu(rng.random((n, n)) < rng.choice([0.2, 0.5, 0.8]), 1)
    return up | up.T


def test_lexicographic_rule_against_exhaustive_enumeration(harness):
    several = 0
    for seed in range(120):
        adj = random_graph(seed)
        cl = all_cliques(adj)
        top = max(len(c) for c in cl)
        best = [c for c in cl if len(c) == top]
        several += len(best) > 1
        want = min(best)
        got = search(harness, adj)
        assert got["exact"] == 1 and got["clique"] == want, seed
        assert tr.smallest_maximum_clique(adj) == want and len(tr.maximum_cliques(adj)) == len(best), seed
    assert several >= 20  # graphs with more than one maximum clique are in the set


def test_budget_exit_is_deterministic(harness):
    t, s, nb = input_sets()["demo_recip_0_15_nb100"]
    adj = tr.graph(t, s, nb)
    full = search(harness, adj)
    assert full["exact"] == 1 and full["nodes"] > 200 and full["clique"] == list(fixture_case("demo_recip_0_15_nb100")["clique"])
    for budget in (0, 1, 50, full["nodes"] - 1):
        a, b = search(harness, adj, budget), search(harness, adj, budget)
        assert a == b and a["exact"] == 0 and a["nodes"] == budget + 1
        c = a["clique"]
        assert len(c) >= a["lb"] and c == sorted(c) and all(adj[i, j] for i, j in itertools.combinations(c, 2))  # the largest found so far: a clique
    assert search(harness, adj, full["nodes"]) == full
    got = solve(harness, t, s, nb, budget=50)
    assert got["clique_exact"] == 0 and got["clique_nodes"] == 51 and got["clique_size"] >= 2


# ---------------------------------------------------------------------------------------------------------------------------------------- the rotation
def test_product_arithmetic_equals_restatement(harness):
    """teaser_horn_rot and teaser_weight, the text the kernels compile"""
    rng = np.random.default_rng(1)
    for k in range(400):
        H = rng.normal(size=9) * 10 ** rng.uniform(-3, 6)
        if k % 50 == 0:
            H[:] = 0
        if k % 51 == 0:
            H = np.outer(rng.normal(size=3), rng.normal(size=3)).reshape(9).copy()
        out = np.zeros(9)
        harness.th_horn(vp(H), vp(out))
        assert out.tobytes() == tr.horn_rot(H).tobytes(), k
    R = tr.horn_rot(rng.normal(size=9))
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    for k in range(2000):
        mu, nb2 = 10 ** rng.uniform(-6, 6), 10 ** rng.uniform(-4, 2)
        r = nb2 * 10 ** rng.uniform(-3, 3) if k % 3 else nb2 * rng.choice([mu / (mu + 1), (mu + 1) / mu, 1.0])
        th1, th2 = ((mu + 1.0) / mu) * nb2, (mu / (mu + 1.0)) * nb2
        want = 0.0 if r >= th1 else (1.0 if r <= th2 else np.sqrt(((nb2 * mu) * (mu + 1.0)) / r) - mu)
        assert harness.th_weight(r, mu, nb2) == want


def run_gnc(L, cs, ct, nb):
    cs, ct = np.ascontiguousarray(cs[:, :4], np.float32), np.ascontiguousarray(ct[:, :4], np.float32)
    ints, dbl = np.zeros(3, np.int64), np.zeros(11)
    nb2 = float(np.float64(np.float32(nb)) ** 2)
    L.th_gnc(vp(cs), vp(ct), len(cs), nb2 if nb2 >= 1e-16 else 1e-2, vp(ints), vp(dbl))
    return dict(iterations=int(ints[0]), stop=int(ints[1]), n_rot=int(ints[2]), cost=dbl[0], R=dbl[2:].reshape(3, 3).copy())


@pytest.mark.parametrize("name,stop", [("exit_mu_exact", 1), ("exit_mu", 1), ("exit_cost", 2), ("exit_limit", 0)])
def test_gnc_exits(harness, name, stop):
    """mu <= 0 in iteration 0 (noise-free data, and data within the bound), the cost threshold, the 100-iteration limit: the loop on the clique's points"""
    t, s, nb = input_sets()[name]
    c = restated(name)["clique"]
    R, cost, iters, exit_, n_rot = tr.gnc(s[c, :3], t[c, :3], nb)
    assert exit_ == stop
    got = run_gnc(harness, s[c], t[c], nb)
    M = len(c) * (len(c) - 1) // 2
    assert got["stop"] == stop and got["iterations"] == iters and got["R"].tobytes() == R.tobytes() and got["cost"].tobytes() == np.float64(cost).tobytes()
    if stop == 1:
        assert iters == 1 and got["n_rot"] == M and cost == 0.0  # no weight update, no cost
    else:
        assert got["n_rot"] == n_rot
        assert iters == (100 if stop == 0 else restated(name)["gnc_iterations"])
    # a zero noise bound takes nb2 = 1e-2 (the replacement below 1e-16)
    if name == "exit_cost":
        a, z = tr.gnc(s[c, :3], t[c, :3], 0.0), run_gnc(harness, s[c], t[c], 0.0)
        assert z["R"].tobytes() == a[0].tobytes() and z["iterations"] == a[2]


# ------------------------------------------------------------------------------------------------------------------------------------- the translation
def both_tls(L, x, rng):
    x = np.asarray(x, np.float64)
    a, b = L.th_tls(vp(x), len(x), rng), float(tr.tls(x, rng))
    assert np.float64(a).tobytes() == np.float64(b).tobytes(), (x, rng, a, b)
    return a


def test_tls_estimator_edges(harness):
    assert both_tls(harness, [3.25], 0.5) == 3.25  # a lone point
    assert both_tls(harness, [2.0] * 7, 0.25) == 2.0  # equal values: all open before any closes
    assert both_tls(harness, [1.0, 1.0, 1.0, 9.0], 0.5) == 1.0
    assert abs(both_tls(harness, [0.0, 0.1, 0.2, 5.0, 5.05], 0.3) - 0.1) < 1e-12  # three against two
    assert both_tls(harness, [0.0, 1.0], 0.5) == 0.0  # intervals that touch: both in costs w (0.25 + 0.25) = 2, one left out costs its range 0.5; the first wins
    assert both_tls(harness, [0.0, 0.2], 0.5) == 0.1  # both in: 4 * 0.02 = 0.08 against 0.5
    # the emptied tail: after the last closing the sums are 0 (or rounding dust) and the candidate is 0 / 0 — a NaN cost never wins
    x = np.array([0.1, 0.7, 0.3])
    est = both_tls(harness, x, 0.05)
    assert np.isfinite(est) and abs(est - 0.1) < 1e-15  # three disjoint intervals: the first strict minimum ((w x) / w is x up to one rounding)
    rng = np.random.default_rng(2)
    for k in range(200):
        n = int(rng.integers(1, 40))
        x = rng.normal(size=n) * 10 ** rng.uniform(-2, 3)
        if k % 4 == 0:
            x = np.round(x, 1)  # ties
        est = both_tls(harness, x, float(10 ** rng.uniform(-2, 1)))
        assert np.isfinite(est)
    assert both_tls(harness, [1.0, 2.0], 0.0) == 0.0  # range 0: every cost is NaN or infinite, nothing wins


@pytest.mark.parametrize("n,share", tr.PLANTED)
def test_planted_transform_conditions(n, share):
    """planted sets (inlier noise at most 0.1 noise_bound per axis): the clique holds at least the planted count, every planted pair lies within the range
    of the result's translation on all three axes, status 1 — of the restatement alone (the fixture for the large sets, which pins it)"""
    name = "planted_%d_%d" % (n, int(100 * share))
    t, s, T, mask = tr.planted(tr.planted_seed(n, share), n, share)
    r = restated(name) if n <= LIVE_LIMIT else fixture_case(name)
    n_planted = int(mask.sum())
    assert n_planted == round(n * (1 - share))
    assert r["status"] == 1  # (min_inlier_num = 3 on these sets: teaser_restated.min_inlier)
    assert r["clique_size"] >= n_planted
    R, that = r["T"][:3, :3], r["T"][:3, 3]
    x = t[mask, :3].astype(np.float64) - s[mask, :3].astype(np.float64) @ R.T
    assert (np.abs(x - that) <= np.float64(np.float32(0.2))).all()
    assert np.abs(R - T[:3, :3]).max() < 1e-3 and np.abs(that - T[:3, 3]).max() < 0.05


# ------------------------------------------------------------------------------------------------------------------------------------------ interfaces
def test_abi_mirror():
    fields = {"mulls_teaser_params": (abi.TeaserParams, [f[0] for f in abi.TeaserParams._fields_]),
              "mulls_teaser_result": (abi.TeaserResult, [f[0] for f in abi.TeaserResult._fields_])}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){"]
    for cname, (_, names) in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in names:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog.append('printf("budget %llu\\n", (unsigned long long)MULLS_TEASER_DEFAULT_NODE_BUDGET);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # the header is still plain C
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    for cname, (ct, names) in fields.items():
        assert int(got[cname]) == C.sizeof(ct), cname
        for f in names:
            assert int(got["%s.%s" % (cname, f)]) == getattr(ct, f).offset, (cname, f)
    assert C.sizeof(abi.TeaserParams) == 16 and C.sizeof(abi.TeaserResult) == 192 and abi.TeaserResult.T.offset == 64
    assert int(got["budget"]) == abi.TEASER_DEFAULT_NODE_BUDGET
    for name in ("mulls_teaser_default_params", "mulls_coarse_reg_teaser", "mulls_coarse_reg_teaser_indexed"):
        assert name in lib.EXPORTS


def test_default_params():
    p = abi.TeaserParams()
    lib.load().mulls_teaser_default_params(C.byref(p))
    q = abi.teaser_params()
    assert (p.noise_bound, p.min_inlier_num, p.clique_node_budget) == (q.noise_bound, q.min_inlier_num, q.clique_node_budget)
    assert p.noise_bound == np.float32(0.2) and p.min_inlier_num == 8 and p.clique_node_budget == abi.TEASER_DEFAULT_NODE_BUDGET  # cregistration.hpp:666
    assert p.clique_node_budget & (p.clique_node_budget - 1) == 0  # a power of two (DESIGN.md section 7.4 derives it)


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
// the call of test/mulls_reg.cpp:177, and the defaults of cregistration.hpp:666
int call(pcTPtr target_cor, pcTPtr source_cor, float keypoint_nms_radius, Eigen::Matrix4d &init_mat)
{
	int a = lo::hip::coarse_reg_teaser<Point_T>(target_cor, source_cor, init_mat, 4.0 * keypoint_nms_radius);
	int b = lo::hip::coarse_reg_teaser<Point_T>(target_cor, source_cor, init_mat);
	int c = lo::hip::coarse_reg_teaser<Point_T>(target_cor, source_cor, init_mat, 0.2, 8);
	return a + b + c;
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_with_the_reference_call():
    """lo::hip::coarse_reg_teaser with upstream's signature and defaults, against the shim headers (as tests/test_ransac.py does for the RANSAC bridge)"""
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 590, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(BRIDGE_TU)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
