"""CPU tests of the NDT registration (mulls_ndt): detmath.h's exp_cr against mpmath; mulls_amd/csrc/ndt_math.h, compiled for the host, against the numpy
restatement tests/ndt_restated.py with equal bits; the restatement against itself (derivatives, a known motion); the fixture tests/golden/ndt_cases.npz
against the restatement; the ctypes mirror against the header.  The restatement was written from reading upstream; nothing here was compared with
ndt_omp or PCL themselves."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

mpmath = pytest.importorskip("mpmath")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import ndt_restated as nr  # noqa: E402
import ndt_scenes  # noqa: E402
from mulls_amd import abi, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ndt_cases.npz")
vp = C.c_void_p


@pytest.fixture(scope="module")
def nh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("nh") / "libnh.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "ndt_math_harness.cpp"), "-o", so])
    h = C.CDLL(so)
    h.nh_script.restype = C.c_int
    return h


def ptr(a):
    return a.ctypes.data_as(vp)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- exp_cr

def test_exp_cr_correctly_rounded(nh):
    """equal to the 300-bit value rounded to double on 120 000 arguments over [-700, 0], the special arguments, and the arguments among them whose
    result lies within 2^-60 (relative) of a rounding boundary: found by measuring every candidate's distance, the hardest is printed"""
    rng = np.random.default_rng(21)
    below = float(np.nextafter(-700.0, -800.0))
    x = np.concatenate([rng.uniform(-700, 0, 70000), -np.exp(rng.uniform(np.log(1e-14), np.log(700), 30000)), rng.uniform(-40, 0, 20000),
                        [0.0, -0.0, -700.0, below, -1e-320, -5e-324, -1.0, -0.5, -np.log(2.0)]])
    out = np.empty(len(x))
    nh.nh_exp(ptr(x), ptr(out), C.c_long(len(x)))
    assert out[-9] == 1.0 and out[-8] == 1.0 and out[-6] == 0.0 and out[-7] > 0.0
    hard, hardest = 0, 1.0
    with mpmath.workprec(300):
        for xi, oi in zip(x, out):
            if xi < -700.0:
                assert oi == 0.0
                continue
            v = mpmath.exp(mpmath.mpf(float(xi)))
            ref = float(v)
            assert oi == ref, (xi, oi, ref)
            # the distance of the true value from the nearest rounding boundary (the midpoint of ref and its neighbour on v's side)
            nb = float(np.nextafter(ref, np.inf if v > ref else -np.inf))
            mid = (mpmath.mpf(ref) + mpmath.mpf(nb)) / 2
            d = float(abs(v - mid) / v)
            if d < 2.0 ** -60:
                hard += 1
                hardest = min(hardest, d)
    assert hard >= 100, hard  # (about one argument in sixty lies that close)
    print("exp_cr: %d of %d arguments within 2^-60 of a rounding boundary, the closest at 2^%.1f" % (hard, len(x), np.log2(hardest)))
    nan = np.array([np.nan, 701.0])
    o2 = np.empty(2)
    nh.nh_exp(ptr(nan), ptr(o2), C.c_long(2))
    assert np.isnan(o2[0]) and o2[1] == np.inf


# ---- ndt_math.h on the host against the restatement

def leaf_of(nh, n, s, q, min_points=6, mult=0.01):
    out = np.empty(14)
    nh.nh_leaf(C.c_int(n), ptr(np.array(s, np.float64)), ptr(np.array(q, np.float64)), C.c_int(min_points), C.c_double(mult), ptr(out))
    return out


def sums_of(P):
    s, q = [0.0] * 3, [0.0] * 6
    for x, y, z in np.asarray(P, np.float32).astype(np.float64):
        s[0] += x
        s[1] += y
        s[2] += z
        for k, v in enumerate((x * x, x * y, x * z, y * y, y * z, z * z)):
            q[k] += v
    return s, q


def test_leaf_finalisation(nh):
    rng = np.random.default_rng(1)
    grid8 = lambda n, k: rng.integers(1, 8, (n, k)) / 8.0
    leaves = {"generic%d" % k: rng.uniform(0, 1, (rng.integers(6, 40), 3)) + rng.integers(-50, 50, 3) for k in range(20)}
    leaves["few"] = rng.uniform(0, 1, (5, 3))
    leaves["planar"] = np.concatenate([grid8(8, 2), np.full((8, 1), 0.5)], axis=1)
    leaves["linear"] = np.concatenate([np.arange(8)[:, None] / 8.0, np.full((8, 2), 0.25)], axis=1)
    leaves["same"] = np.tile([[6.5, 2.5, 0.5]], (6, 1))
    leaves["thin"] = rng.uniform(0, 1, (12, 3)) * [1, 1, 1e-4]
    seen = set()
    for name, P in leaves.items():
        s, q = sums_of(P)
        L = nr.finalize_leaf(len(P), s, q)
        got = leaf_of(nh, len(P), s, q)
        want = np.array(L["mean"] + L["icov"] + L["evals"] + [L["n"], L["inflated"]], np.float64)
        assert same_bits(got, want), name
        seen.add((L["n"] > 0, L["inflated"]))
        if name == "planar":
            assert L["inflated"] == 1 and L["n"] == 8 and L["evals"][0] == 0.01 * L["evals"][2]
        if name == "linear":
            assert L["inflated"] == 2 and L["evals"][0] == L["evals"][1] == 0.01 * L["evals"][2]
        if name == "same":
            assert L["n"] == -1
        if name == "few":
            assert L["n"] == 5 and L["icov"] == [0.0] * 6
        if name == "thin":
            assert L["inflated"] >= 1
    assert {(True, 0), (True, 1), (True, 2), (False, 0)} <= seen


POSES = [[0.0] * 6, [0.02, -0.01, 0.015, 0.004, -0.003, 0.005], [0.3, 0.1, -0.2, 5e-5, 0.2, -9e-5], [1.0, -2.0, 0.5, -0.7, 0.4, 2.5]]


def test_frame_and_transform(nh):
    for p in POSES:
        F = nr.make_frame(p)
        want = np.array(F["R"] + F["t"] + [v for row in F["j"] for v in row] + [v for row in F["h"] for v in row], np.float64)
        got = np.empty(81)
        nh.nh_frame(ptr(np.array(p, np.float64)), ptr(got))
        assert same_bits(got, want), p
        x = np.array([[12.5, -3.25, 1.7]], np.float32)
        o = np.empty(3, np.float32)
        nh.nh_transform(ptr(np.array(p, np.float64)), ptr(x), ptr(o))
        assert np.array_equal(o.view(np.uint32), nr.transform(F, x)[0].view(np.uint32))


def test_point_contribution(nh):
    rng = np.random.default_rng(2)
    d1, d2, _ = nr.gauss_constants(1.0, 0.55)
    rejected = 0
    for trial in range(60):
        p = POSES[trial % len(POSES)]
        P = rng.uniform(0, 1, (10, 3)) * ([1, 1, 1] if trial % 3 else [1, 1, 0.0])
        s, q = sums_of(P)
        L = nr.finalize_leaf(10, s, q)
        x = rng.uniform(-30, 30, 3)
        xt = rng.normal(0, 0.4 if trial % 5 else 30.0, 3)
        C6 = np.array(L["icov"]) * (1.0 if trial % 7 else -1.0)  # (a negative definite matrix: the pair is rejected by the E > 1 test)
        for with_h in (0, 1):
            want = np.zeros(28) + nr.contribution(x[None], xt[None], C6[None], nr.make_frame(p), d1, d2, with_h)[0]  # (added to sums that start at +0)
            got = np.zeros(28)
            nh.nh_contribution(ptr(np.array(p, np.float64)), ptr(x), ptr(xt), ptr(C6), C.c_double(d1), C.c_double(d2), C.c_int(with_h), ptr(got))
            assert same_bits(got, want), (trial, with_h)
            rejected += int(not want.any())
            if not with_h:
                assert not want[7:].any()
    assert 0 < rejected < 100


def test_solve6(nh):
    rng = np.random.default_rng(3)
    iu = np.triu_indices(6)
    mats = []
    for k in range(12):
        B = rng.normal(size=(6, 6))
        mats.append(-(B @ B.T) - 0.1 * np.eye(6))
    J = rng.normal(size=(6, 3))
    mats.append(-(J @ J.T))  # rank 3
    mats.append(np.zeros((6, 6)))
    mats.append(np.diag([1.0, -2.0, 3.0, 0.0, 1e-30, 5.0]))
    bad = np.eye(6)
    bad[2, 4] = bad[4, 2] = np.nan
    mats.append(bad)
    for k, H in enumerate(mats):
        g = rng.normal(size=6)
        Hu = np.ascontiguousarray(H[iu])
        want = np.array(nr.solve6(Hu, g))
        got = np.empty(6)
        nh.nh_solve6(ptr(Hu), ptr(g), ptr(got))
        assert same_bits(got, want), k
        if k < 12:
            assert np.allclose(H @ got, -g, rtol=0, atol=1e-9 * np.abs(g).max() * np.linalg.cond(H))
        if k == 12:  # the minimum-norm step of the rank-deficient system: it lies in the range of J and solves the projected equations
            Pr = J @ np.linalg.pinv(J)
            assert np.allclose(Pr @ got, got, atol=1e-9) and np.allclose(H @ got, -Pr @ g, atol=1e-9)
        if k == 13:
            assert not got.any()
    assert np.isnan(got).all()


def scripted(kind):
    """28 sums per evaluation, invented: the state machine does not know where they come from"""
    rng = np.random.default_rng(7)
    sgn = -1.0 if kind == "close" else 1.0
    Hu = [sgn * (1.0 + 0.1 * i) if i == k else 0.01 * sgn * (i + k) for i in range(6) for k in range(i, 6)]
    g0 = np.array([1.2, 0.1, -0.3, 0.05, 0.02, 1.6])
    steps = [[-1.0] + list(g0) + Hu]
    seq = [(-0.5, -2.0), (-0.6, -1.5), (-0.7, 0.2), (-0.8, 0.3), (-0.9, 0.1), (-0.95, 0.05), (-0.97, 0.01), (-0.98, 0.01), (-0.99, 0.001), (-0.995, 0.001),
           (-0.999, 0.0001), (-0.9995, 0.0001)]
    for s, k in seq * 3:
        steps.append([s] + list(k * g0 * (1 if kind == "close" else -1) + rng.normal(0, 0.01, 6)) + Hu)
    return np.array(steps)


@pytest.mark.parametrize("kind", ["close", "reverse"])
def test_scripted_line_search(nh, kind):
    sums = scripted(kind)
    prm = nr.default_params(transformation_epsilon=0.2 if kind == "close" else 0.1)
    S, rows, closed, hess_only = nr.State(), [], False, 0
    for k in range(len(sums)):
        nr.advance(S, sums[k], prm, 100)
        rows.append(list(S.xt) + [S.with_hessian, S.phase, S.running, S.a_t])
        closed |= S.open_interval == 0 and S.phase == nr.PH_MT_LOOP
        hess_only += S.phase == nr.PH_HESS and S.running
        if not S.running:
            break
    out, fin = np.zeros((len(sums), 10)), np.zeros(12)
    n = nh.nh_script(ptr(sums), C.c_int(len(sums)), C.c_double(prm["step_size"]), C.c_double(prm["transformation_epsilon"]), C.c_int(prm["max_iterations"]),
                     C.c_int(prm["max_step_iterations"]), C.c_double(100.0), ptr(out), ptr(fin))
    assert n == len(rows) and same_bits(out[:n], np.array(rows, np.float64))
    assert same_bits(fin, np.array(list(S.p) + [S.nr_iterations, S.evaluations, S.converged, S.reversals, S.inner_steps, S.trans_probability], np.float64))
    if kind == "close":
        assert closed and hess_only >= 2 and S.inner_steps >= 10 and S.reversals == 0  # the interval closes, a search runs out of inner steps
    else:
        assert S.reversals >= 1 and S.inner_steps == 0 and S.converged == 1 and not S.running


# ---- the restatement against itself

def test_derivatives_against_central_differences():
    """gradient and Hessian of the restatement against central differences of its own score and gradient.  The source points sit within 0.15 m of the
    centres of occupied cells and the pose moves no point by more than 0.1 m, so that no point changes its cell between the two sides of a difference
    (the score is discontinuous there).  h = 1e-3: the float rounding of the moved point (half an ulp of 10 m, 5e-7 m) then shifts a difference
    quotient by about 1e-3 of a single point's derivative; a missing or mis-signed term shifts it by its full size.  Bound: 1e-2 of the largest entry."""
    tgt, _ = ndt_scenes.crafted()
    grid = nr.build_grid(tgt, 1.0)
    rng = np.random.default_rng(4)
    cells = []
    for key, li in grid.index.items():
        if grid.n[li] >= 6:
            k2, rem = divmod(key, grid.div_b[0] * grid.div_b[1])
            k1, k0 = divmod(rem, grid.div_b[0])
            cells.append([k0 + grid.min_b[0] + 0.5, k1 + grid.min_b[1] + 0.5, k2 + grid.min_b[2] + 0.5])
    src = (np.array(cells) + rng.uniform(-0.15, 0.15, (len(cells), 3))).astype(np.float32)
    d1, d2, _ = nr.gauss_constants(1.0, 0.55)
    p0 = np.array([0.02, -0.01, 0.015, 0.004, -0.003, 0.005])
    base = nr.evaluate(src, p0, grid, d1, d2, 1)
    grad, H = base[1:7], np.zeros((6, 6))
    H[np.triu_indices(6)] = base[7:]
    H = H + np.triu(H, 1).T
    h = 1e-3
    g_fd, H_fd = np.zeros(6), np.zeros((6, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        up, dn = nr.evaluate(src, p0 + e, grid, d1, d2, 0), nr.evaluate(src, p0 - e, grid, d1, d2, 0)
        g_fd[k] = (up[0] - dn[0]) / (2 * h)
        H_fd[k] = (up[1:7] - dn[1:7]) / (2 * h)
    print("gradient", grad, "\ndifference quotient", g_fd, "\nmax |H - H_fd|", np.abs(H - H_fd).max(), "of", np.abs(H).max())
    assert np.abs(grad - g_fd).max() <= 1e-2 * np.abs(grad).max()
    assert np.abs(H - H_fd).max() <= 1e-2 * np.abs(H).max()


def test_recovers_a_known_motion():
    """the source is a sample of the target moved by the inverse of a known motion (0.3 m, 3 degrees of yaw): the restatement's result lies 0.019 m and
    0.0002 rad from it.  The bound, 0.05 m and 0.002 rad, leaves room for that and none for a wrong sign or frame (0.3 m or 0.05 rad and more)."""
    sc = synth.Scene(3)
    A = synth.raycast(sc, synth.se3(0, 0, sc.sensor_height), n_beams=32, n_az=400, seed=1)["xyz"]
    rng = np.random.default_rng(0)
    A = A[np.sort(rng.choice(len(A), 5000, replace=False))]
    M = synth.se3(0.3, -0.1, 0.05, yaw=np.deg2rad(3))
    Mi = np.linalg.inv(M)
    src = (A[np.sort(rng.choice(len(A), 1500, replace=False))].astype(np.float64) @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32)
    res = nr.ndt(A, src, ndt_scenes.bound_of(A), ndt_scenes.bound_of(src), np.eye(4))
    dt, dr = synth.pose_error(res["T"], M)
    print("recovered to %.4f m, %.5f rad in %d iterations" % (dt, dr, res["iterations"]))
    assert res["converged"] == 1 and res["code"] == 1 and dt < 0.05 and dr < 0.002


# ---- the fixture

def load_golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["names"]))


def test_fixture_equals_the_restatement():
    import make_ndt_golden

    z, names = load_golden()
    fresh = make_ndt_golden.compute()
    assert sorted(fresh) == sorted(z.files)
    for k in z.files:
        a, b = z[k], fresh[k]
        if a.dtype.kind in "US":
            assert str(a) == str(b), k
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_cases_cover_the_paths():
    z, names = load_golden()
    I = {n: dict(zip(make_golden_fields(), z[n + "/ints"])) for n in names}
    assert I["street"]["inner_steps"] == 0 and I["street"]["evaluations"] == I["street"]["iterations"] + 1
    assert I["street_inner"]["inner_steps"] > 0 and I["street_inner"]["evaluations"] > I["street_inner"]["iterations"] + 1
    assert any(I[n]["line_search_reversals"] > 0 for n in names) and any(I[n]["line_search_reversals"] == 0 and I[n]["iterations"] > 0 for n in names)
    assert I["street_max_iter"]["iterations"] == 2 + 2  # nr_iterations > max_iterations, then the increment
    assert I["street_2m"]["iterations"] == 2 and I["street_2m"]["converged"] == 1  # the epsilon test, first allowed at the second iteration
    nl = I["no_leaves"]
    assert nl["n_leaves_used"] == 0 and nl["converged"] == 1 and nl["iterations"] == 0 and nl["evaluations"] == 1 and nl["n_tgt"] == 500
    assert z["no_leaves/T"].tobytes() == z["no_leaves/guess"].tobytes()
    assert I["street_no_crop"]["n_src"] == 400 and I["street"]["n_src"] < 400
    assert z["street_near_identity/T"].tobytes() == z["street/T"].tobytes() and z["street_guess/T"].tobytes() != z["street/T"].tobytes()
    assert len({z[n + "/T"].tobytes() for n in ("street", "street_direct1", "street_direct26", "street_2m")}) == 4
    # the hand-made leaves of the crafted target, and source points beyond the grid on every side
    tgt, src = z["crafted/tgt"], z["crafted/src"]
    grid = nr.build_grid(tgt, 1.0)
    leaf = lambda c: grid.leaves[grid.index[(c[0] - grid.min_b[0]) + (c[1] - grid.min_b[1]) * grid.div_b[0] + (c[2] - grid.min_b[2]) * grid.div_b[0] * grid.div_b[1]]]
    assert leaf((2, 2, 0))["inflated"] == 1 and leaf((4, 2, 0))["inflated"] == 2 and leaf((6, 2, 0))["n"] == -1
    assert leaf((2, 4, 0))["n"] == 5 and leaf((4, 4, 0))["n"] == 6 and leaf((4, 4, 0))["inflated"] == 0
    q = np.floor(src / np.float32(1.0)).astype(int)
    for c in range(3):
        assert (q[:, c] < grid.min_b[c] - 1).any() and (q[:, c] > grid.max_b[c] + 1).any()


def make_golden_fields():
    import make_ndt_golden

    return make_ndt_golden.INT_FIELDS


# ---- the ctypes mirror

def test_ctypes_layout_matches_header():
    fields = {"mulls_ndt_params": abi.NdtParams, "mulls_ndt_problem": abi.NdtProblem, "mulls_ndt_result": abi.NdtResult}
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "mulls_hip.h"', "int main(void){"]
    for cname, ct in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog.append('printf("tree %u\\n", MULLS_NDT_TREE); printf("search %d %d %d %d\\n", MULLS_NDT_KDTREE, MULLS_NDT_DIRECT26, MULLS_NDT_DIRECT7, MULLS_NDT_DIRECT1);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = {line.split()[0]: line.split()[1:] for line in out if line}
    for cname, ct in fields.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got["%s.%s" % (cname, f)][0]) == getattr(ct, f).offset, (cname, f)
    assert int(got["tree"][0]) == abi.NDT_TREE == nr.TREE
    assert [int(v) for v in got["search"]] == [abi.NDT_KDTREE, abi.NDT_DIRECT26, abi.NDT_DIRECT7, abi.NDT_DIRECT1] == [nr.KDTREE, nr.DIRECT26, nr.DIRECT7, nr.DIRECT1]


def test_default_params_match():
    from mulls_amd import lib

    p = abi.NdtParams()
    lib.load().mulls_ndt_default_params(C.byref(p))
    q, r = abi.ndt_params(), nr.default_params()
    for name, _ in abi.NdtParams._fields_:
        assert getattr(p, name) == getattr(q, name), name
        if name in r:
            assert getattr(p, name) == r[name], name


# ---- the bridge

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
// the calls of test/mulls_slam.cpp:635 and :672, and the batch form
int call(lo::constraint_t &con, std::vector<lo::constraint_t> &cons, Eigen::Matrix4d guess)
{
	int a = lo::hip::omp_ndt<Point_T>(con, 1.0, true, guess, true, 10.0);
	int b = lo::hip::omp_ndt<Point_T>(con);
	std::vector<int> c = lo::hip::omp_ndt_batch<Point_T>(cons, 2.0f);
	return a + b + (int)c.size();
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_against_the_reference_types():
    """lo::hip::omp_ndt and omp_ndt_batch on the reference's constraint_t (pc_down, local_bound, Trans1_2), as tests/test_pgo.py checks its bridge: the
    stand-in headers under oracle/ref_shim offer the pcl types, the reference's utility.hpp the block and constraint types.  A compile check: running
    the bridge needs the reference tree and a device together, which no test machine has."""
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
