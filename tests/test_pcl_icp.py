"""CPU tests of the classical ICP registration (mulls_pcl_icp): mulls_amd/csrc/pcl_icp_math.h, compiled for the host as a stand-alone program, against
the numpy restatement tests/pcl_icp_restated.py with equal bits on the fixture's recorded inputs; the fixture tests/golden/pcl_icp_cases.npz against
the restatement; which case takes which path; two conditions against the scenes' truth; the ctypes mirror against the header; the bridge's compile
check.  The restatement was written from the header's definition; nothing here was compared with PCL, FLANN or Eigen themselves."""
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

import pcl_icp_restated as pr  # noqa: E402
import pcl_icp_scenes  # noqa: E402
from make_pcl_icp_golden import INT_FIELDS, cloud_of  # noqa: E402
from mulls_amd import abi, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pcl_icp_cases.npz")
ALL = ["street", "street_recip", "street_plane", "street_plane_recip", "street_max_iter", "street_rel_mse", "street_plane_rel_mse", "street_guess",
       "street_near_identity", "street_no_crop", "street_tight", "street_large", "lifted", "empty", "exact_subset", "abs_mse", "crafted", "crafted_one_way",
       "crafted_plane", "singular", "late_loss", "three_pairs", "two_pairs"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ph") / "pcl_icp_math_harness")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "pcl_icp_math_harness.cpp"), "-o", exe])

    def run(args, data, width):
        out = subprocess.run([exe] + [str(a) for a in args], input=np.ascontiguousarray(data, np.float64).tobytes(), stdout=subprocess.PIPE, check=True).stdout
        return np.frombuffer(out, np.float64).reshape(-1, width)

    return run


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}, json.loads(str(z["names"]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. the fixture

@pytest.fixture(scope="module")
def fresh():
    import make_pcl_icp_golden

    return make_pcl_icp_golden.compute()


def test_fixture_equals_the_restatement(golden, fresh):
    z, _ = golden
    assert sorted(fresh) == sorted(z)
    for k in z:
        a, b = z[k], fresh[k]
        if a.dtype.kind in "US":
            assert str(a) == str(b), k
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


# ---- 2. pcl_icp_math.h on the host against the restatement, on the fixture's recorded inputs

@pytest.mark.parametrize("case", ["street", "street_plane", "crafted_plane"])
def test_harness_gives_the_restatements_bits(harness, golden, case):
    z, _ = golden
    m = lambda k: z["math/%s/%s" % (case, k)]
    prm = pr.default_params(**json.loads(str(z[case + "/prm"])))
    if prm["metrics"] == pr.POINT2PLANE:
        assert len(m("normal_out")) == 40 and same_bits(harness(["normal"], m("normal_in"), 3), m("normal_out"))
        assert len(m("term_in")) >= 20 and same_bits(harness(["term"], m("term_in"), 28), m("term_out"))
        got = harness(["plane"], m("plane_in"), 13)
        assert same_bits(got, m("plane_out"))
        assert got[-1, 12] == 0.0 and got[:-1, 12].all()  # the zero matrix has no pivot; the recorded systems have
    else:
        assert len(m("rigid_in")) == 8 and same_bits(harness(["rigid"], m("rigid_in"), 12), m("rigid_out"))
    run = harness(["run", prm["metrics"], prm["max_iter_num"], repr(prm["transformation_epsilon"]), repr(prm["euclidean_fitness_epsilon"])], m("run_in"), 32)
    assert same_bits(run, m("run_out"))
    assert run[-1, 30] == 0.0 and (run[:-1, 30] == 1.0).all()  # runs until the last recorded iteration
    ints = dict(zip(INT_FIELDS, z[case + "/ints"]))
    assert (run[-1, 27], run[-1, 28], run[-1, 29]) == (ints["iterations"], ints["converged"], ints["stop"]) and len(run) == ints["iterations"]


def test_pieces_against_numpy(golden):
    """the restatement's pieces against plain numpy: the rigid step against an SVD Kabsch, the plane step against numpy.linalg.solve, the normals
    against eigh where the smallest eigenvalue is distinct.  Bounds: a few hundred ulp of the quantities involved."""
    z, _ = golden
    for row, out in zip(z["math/street/rigid_in"], z["math/street/rigid_out"]):
        H, cs, ct = row[:9].reshape(3, 3), row[9:12], row[12:15]
        U, _, Vt = np.linalg.svd(H)
        D = np.diag([1.0, 1.0, np.linalg.det(Vt.T @ U.T)])
        R = Vt.T @ D @ U.T
        assert np.abs(out[:9].reshape(3, 3) - R).max() < 1e-12 and np.abs(out[9:] - (ct - R @ cs)).max() < 1e-10
    iu = np.triu_indices(6)
    for s, d in zip(z["math/street_plane/plane_in"][:-1], z["math/street_plane/plane_out"][:-1]):
        Hm = np.zeros((6, 6))
        Hm[iu] = s[:21]
        Hm = Hm + np.triu(Hm, 1).T
        x = np.linalg.solve(Hm, s[21:27])
        a, b, g = x[:3]
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
        tol = 1e-12 * np.linalg.cond(Hm)
        assert np.abs(d[:9].reshape(3, 3) - Rz @ Ry @ Rx).max() < tol and np.abs(d[9:12] - x[3:]).max() < tol
    for case in ("street_plane", "crafted_plane"):
        flat, want, at, distinct = z["math/%s/normal_in" % case], z["math/%s/normal_out" % case], 0, 0
        for n in want:
            k = int(flat[at])
            p, Q = flat[at + 1:at + 4], flat[at + 4:at + 4 + 3 * k].reshape(k, 3)
            at += 4 + 3 * k
            if k < 3:
                assert (n == np.float32(0.577)).all()
                continue
            ev, evec = np.linalg.eigh(np.cov(Q.T, bias=True) * k)
            assert abs(np.linalg.norm(n) - 1.0) < 1e-6 and n @ (-p) >= -1e-6
            if ev[0] < 0.5 * ev[1] and ev[1] > 1e-9:
                distinct += 1
                assert abs(abs(evec[:, 0] @ n) - 1.0) < 1e-6
        assert at == len(flat) and distinct >= 10, (case, distinct)


# ---- 3. which case takes which path

def test_cases_cover_the_paths(golden):
    z, names = golden
    assert names == ALL
    I = {n: dict(zip(INT_FIELDS, z[n + "/ints"])) for n in names}
    P = {n: pr.default_params(**json.loads(str(z[n + "/prm"]))) for n in names}
    T = lambda n: z[n + "/T"].tobytes()
    stop = lambda n: (I[n]["stop"], I[n]["converged"])
    # the four combinations, each stopped by the transformation rule well inside the iteration cap
    combos = ["street", "street_recip", "street_plane", "street_plane_recip"]
    assert [(P[n]["metrics"], P[n]["use_reciprocal_correspondence"]) for n in combos] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert len({T(n) for n in combos}) == 4
    for n in combos:
        assert stop(n) == (pr.STOP_TRANSFORM, 1) and 3 <= I[n]["iterations"] < 20 and I[n]["code"] == 1, n
    assert I["street_recip"]["n_corr"] < I["street"]["n_corr"] and I["street_plane_recip"]["n_corr"] < I["street_plane"]["n_corr"]
    # the stop rules
    assert stop("street_max_iter") == (pr.STOP_ITERATIONS, 1) and I["street_max_iter"]["iterations"] == 3
    assert stop("street_rel_mse") == (pr.STOP_REL_MSE, 1) and stop("street_plane_rel_mse") == (pr.STOP_REL_MSE, 1)
    assert I["street_rel_mse"]["iterations"] < I["street"]["iterations"] and I["street_plane_rel_mse"]["iterations"] < I["street_plane"]["iterations"]
    assert stop("abs_mse") == (pr.STOP_ABS_MSE, 1) and P["abs_mse"]["transformation_epsilon"] == 0.0
    assert stop("lifted") == (pr.STOP_NO_CORRESPONDENCES, 0) and I["lifted"]["iterations"] == 0 and I["lifted"]["n_corr"] == 0 and I["lifted"]["n_fit"] == 0
    assert z["lifted/floats"][0] == pr.DBL_MAX and I["lifted"]["code"] == -3 and T("lifted") == np.eye(4).tobytes()
    assert stop("late_loss") == (pr.STOP_NO_CORRESPONDENCES, 0) and I["late_loss"]["iterations"] == 1 and I["late_loss"]["n_corr"] == 2
    assert T("late_loss") != np.eye(4).tobytes()  # the pose reached so far is kept
    assert stop("singular") == (pr.STOP_SINGULAR, 0) and I["singular"]["iterations"] == 0 and I["singular"]["n_corr"] == I["singular"]["n_src"]
    assert stop("two_pairs") == (pr.STOP_NO_CORRESPONDENCES, 0) and I["two_pairs"]["n_corr"] == 2 and I["two_pairs"]["n_src"] == 2
    assert stop("three_pairs")[1] == 1 and I["three_pairs"]["n_corr"] == 3 and I["three_pairs"]["n_src"] == 3
    em = I["empty"]
    assert (em["n_src"], em["code"], em["stop"], em["converged"], em["iterations"]) == (0, -3, pr.STOP_NONE, 0, 0) and z["empty/floats"][0] == pr.DBL_MAX
    # the guess, the near-identity guess, the crop
    assert T("street_near_identity") == T("street") and T("street_guess") != T("street")
    assert I["street"]["n_src"] == 399 and I["street_no_crop"]["n_src"] == 400 and I["street_tight"]["iterations"] < I["street"]["iterations"]
    # street_large crosses the strided partials' width
    assert I["street_large"]["n_src"] > abi.NDT_TREE and I["street_large"]["n_fit"] > abi.NDT_TREE and I["street_large"]["n_tgt"] == 3000
    # crafted
    tgt, src = cloud_of(z, "crafted", "tgt"), cloud_of(z, "crafted", "src")
    grid = lambda c: np.array_equal(c * 8, np.round(c * 8))
    off_grid = [p for p in tgt if not grid(p)]
    assert len(off_grid) == 8  # the points on cell faces
    for edge, dist in ((pcl_icp_scenes.EDGE_T, 1.5), (pcl_icp_scenes.EDGE_R, 2.0)):
        assert float(np.float32(edge)) == edge  # the faces are floats
        q = tgt[:, 0].astype(np.float64) * (1.0 / (dist * pr.MARGIN))
        assert ((q == np.floor(q)) & (tgt[:, 0] > 0)).any() and ((np.abs(q - np.round(q)) < 1e-9) & (tgt[:, 0] < 0)).any(), dist
    match, d2 = pr.correspondences(src, tgt, 1.5, 0)
    both, _ = pr.correspondences(src, tgt, 1.5, 1)
    d = pr.dist2(src[:, None, :], tgt[None, :, :])
    tie_t = sum(int((d[i] == d[i].min()).sum() > 1 and not (tgt[d[i] == d[i].min()] == tgt[match[i]]).all()) for i in range(len(src)) if match[i] >= 0)
    assert tie_t >= 1  # two different target points equally near: the index decided
    assert (d2.astype(np.float64) == 2.25).any()  # a pair at exactly the distance is kept
    assert len(np.unique(tgt, axis=0)) < len(tgt) and len(np.unique(src, axis=0)) < len(src)  # identical points on both sides
    shared = [m for m in np.unique(match[match >= 0]) if (match == m).sum() > 1]
    assert len(shared) >= 3 and all((both == m).sum() == 1 for m in shared)
    tie_s = 0
    for m in shared:
        rivals = np.flatnonzero(match == m)
        dm = pr.dist2(src[rivals], tgt[m][None, :])
        keep = np.flatnonzero(both == m)[0]
        assert dm[list(rivals).index(keep)] == dm.min()
        tie_s += int((dm == dm.min()).sum() > 1 and keep == rivals[dm == dm.min()].min())
    assert tie_s >= 1  # two source points equally near one target point: the lower index survives
    sizes = np.array([len(pr.neighbourhood(tgt, i, 2.0)) for i in range(len(tgt))])
    assert (sizes == 2).sum() >= 2 and (sizes == 3).sum() >= 3 and sizes.max() > pcl_icp_scenes.TILE
    at_radius = sum(int((pr.dist2(tgt, tgt[i][None, :]).astype(np.float64) == 4.0).any()) for i in np.flatnonzero(sizes == 3))
    assert at_radius >= 2  # a neighbour at exactly the radius makes the third
    nrm = pr.normals(tgt, 2.0)
    assert ((nrm == np.float32(0.577)).all(axis=1)).sum() == (sizes < 3).sum()
    flat = (tgt[:, 2] == 0) & (tgt[:, 0] >= 4) & (tgt[:, 0] <= 6.375) & (tgt[:, 1] >= 4) & (tgt[:, 1] <= 6.375)
    assert flat.sum() == 400 and (np.abs(nrm[flat]) == [0.0, 0.0, 1.0]).all()  # n . p = 0: the sign the Jacobi rotations left is kept
    line = (tgt[:, 1] == 6.0) & (tgt[:, 2] == 1.0)
    assert line.sum() == 17 and (np.abs(nrm[line, 0]) < 1e-6).all()  # collinear neighbourhoods: a unit normal across the line
    # singular: every normal is (0, 0, +-1)
    st = cloud_of(z, "singular", "tgt")
    assert (np.abs(pr.normals(st, 2.0)) == [0.0, 0.0, 1.0]).all()


# ---- 4. conditions against the truth

def test_point_to_point_recovers_the_known_motion_of_an_exact_subset(golden):
    """the source is every fourth target point under the inverse of se3(0.05, 0.02, 0, yaw 0.3 deg): the restatement's pose must be that motion.
    Measured: 3.2e-8 m (the float storage of the source and of the moved cloud; the issue's float64 prototype had 8e-16 m) and a rotation
    angle of 0 as pose_error measures it, whose arccos resolves 1.5e-8 rad next to 1.  The bounds: twice the measured distance, for the float storage
    of the moved cloud, and twice that resolution."""
    z, _ = golden
    M = synth.se3(0.05, 0.02, 0.0, yaw=np.deg2rad(0.3))
    dt, dr = synth.pose_error(z["exact_subset/T"], M)
    print("exact_subset: %.3e m, %.3e rad from the known motion after %d iterations" % (dt, dr, z["exact_subset/ints"][1]))
    assert z["exact_subset/ints"][1] == 3
    assert dt < 2 * 3.2e-8 and dr <= 2 * 1.5e-8


def test_point_to_plane_ends_near_the_truth_on_street(golden):
    """Point2Plane with a radius of 2 m on `street` against the scene's true motion.  Measured: 0.0198 m and 0.00573 rad (0.33 deg; the issue's
    float64 prototype had 0.020 m and 0.33 deg).  The bounds are twice the measured values.  Point2Point has no such condition: it ends about 0.25 m
    off on these 16-beam rings, which is the method."""
    z, _ = golden
    _, T_gt = pcl_icp_scenes.build_cases()
    dt, dr = synth.pose_error(z["street_plane/T"], T_gt)
    dt0, dr0 = synth.pose_error(np.eye(4), T_gt)
    print("street_plane: %.4f m, %.5f rad from the truth at the end; %.4f m, %.5f rad at the start" % (dt, dr, dt0, dr0))
    assert dt < 2 * 0.0198 and dr < 2 * 0.00573


# ---- 5. the ctypes mirror

def test_ctypes_layout_matches_header():
    fields = {"mulls_pcl_icp_params": abi.PclIcpParams, "mulls_pcl_icp_problem": abi.PclIcpProblem, "mulls_pcl_icp_result": abi.PclIcpResult}
    enums = {"metric": ("MULLS_PCL_ICP_POINT2POINT", "MULLS_PCL_ICP_POINT2PLANE", "MULLS_PCL_ICP_PLANE2PLANE"), "ce": ("MULLS_PCL_ICP_NN", "MULLS_PCL_ICP_NS"),
             "te": ("MULLS_PCL_ICP_SVD", "MULLS_PCL_ICP_LM", "MULLS_PCL_ICP_LLS"),
             "stop": tuple("MULLS_PCL_ICP_STOP_" + s for s in ("NONE", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES", "SINGULAR"))}
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "mulls_hip.h"', "int main(void){"]
    for cname, ct in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    for name, vals in enums.items():
        prog.append('printf("%s%s\\n", %s);' % (name, " %d" * len(vals), ", ".join(vals)))
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
    assert [int(v) for v in got["metric"]] == [abi.PCL_ICP_POINT2POINT, abi.PCL_ICP_POINT2PLANE, abi.PCL_ICP_PLANE2PLANE] == [pr.POINT2POINT, pr.POINT2PLANE, pr.PLANE2PLANE]
    assert [int(v) for v in got["ce"]] == [abi.PCL_ICP_NN, abi.PCL_ICP_NS] == [pr.NN, pr.NS]
    assert [int(v) for v in got["te"]] == [abi.PCL_ICP_SVD, abi.PCL_ICP_LM, abi.PCL_ICP_LLS] == [pr.SVD, pr.LM, pr.LLS]
    stops = [abi.PCL_ICP_STOP_NONE, abi.PCL_ICP_STOP_ITERATIONS, abi.PCL_ICP_STOP_TRANSFORM, abi.PCL_ICP_STOP_ABS_MSE, abi.PCL_ICP_STOP_REL_MSE,
             abi.PCL_ICP_STOP_NO_CORRESPONDENCES, abi.PCL_ICP_STOP_SINGULAR]
    assert [int(v) for v in got["stop"]] == stops == [pr.STOP_NONE, pr.STOP_ITERATIONS, pr.STOP_TRANSFORM, pr.STOP_ABS_MSE, pr.STOP_REL_MSE,
                                                      pr.STOP_NO_CORRESPONDENCES, pr.STOP_SINGULAR]


def test_default_params_match():
    from mulls_amd import lib

    p = abi.PclIcpParams()
    lib.load().mulls_pcl_icp_default_params(C.byref(p))
    q, r = abi.pcl_icp_params(), pr.default_params()
    for name, _ in abi.PclIcpParams._fields_:
        a, b = getattr(p, name), getattr(q, name)
        assert a == b, name
        if name in r:
            assert a == r[name], name
    assert set(r) == {name for name, _ in abi.PclIcpParams._fields_} - {"scratch_limit_bytes"}


# ---- the bridge

from test_ncc import REF_UTILITY  # noqa: E402  (where the reference tree is looked for)
from test_ndt import BRIDGE_TU  # noqa: E402

REF_CREGISTRATION = os.path.join(os.path.dirname(REF_UTILITY), "cregistration.hpp")
PCL_ICP_CALLS = r"""
namespace lo
{
#include "reg_enums.inc"
} // namespace lo
// the call CRegistration::pcl_icp's body would make, the defaults, and the batch form
int call_pcl_icp(lo::constraint_t &con, std::vector<lo::constraint_t> &cons, Eigen::Matrix4d guess)
{
	int a = lo::hip::pcl_icp<Point_T>(con, 20, 1.5f, lo::Point2Plane, lo::NN, lo::LLS, true, false, 2.0, guess, true, 10.0);
	int b = lo::hip::pcl_icp<Point_T>(con, 20, 1.5f, lo::Point2Point, lo::NN, lo::SVD, false, false);
	std::vector<int> c = lo::hip::pcl_icp_batch<Point_T>(cons, 20, 1.5f, lo::Point2Point, lo::NN, lo::SVD, false, false);
	return a + b + (int)c.size();
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY) or not os.path.exists(REF_CREGISTRATION),
                    reason="the reference's utility.hpp and cregistration.hpp (constraint_t, the three enums: what the bridge header expects to be visible) are not here")
def test_bridge_compiles_against_the_reference_types():
    """lo::hip::pcl_icp and pcl_icp_batch on the reference's constraint_t and enums, as tests/test_gicp.py checks the GICP bridge.  A compile check:
    running the bridge needs the reference tree and a device together, which no test machine has."""
    lines = open(REF_UTILITY, errors="replace").read().split("\n")
    reg_lines = open(REF_CREGISTRATION, errors="replace").read().split("\n")

    def cut(src, first, last, expect):
        assert expect in src[first - 1], (first, expect)
        return "\n".join(src[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(lines, 84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(lines, 92, 157, "struct centerpoint_t") + cut(lines, 233, 558, "struct cloudblock_t") + cut(lines, 561, 592, "struct constraint_t"))
        open(os.path.join(d, "reg_enums.inc"), "w").write(cut(reg_lines, 59, 75, "enum TransformEstimationType"))
        open(os.path.join(d, "tu.cpp"), "w").write(BRIDGE_TU + PCL_ICP_CALLS)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
