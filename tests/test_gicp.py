"""CPU tests of the voxelised GICP registration (mulls_gicp): mulls_amd/csrc/gicp_math.h, compiled for the host as a stand-alone program, against the
numpy restatement tests/gicp_restated.py with equal bits on the fixture's recorded inputs; the fixture tests/golden/gicp_cases.npz against the
restatement; which case takes which path; a condition on the street scene; the ctypes mirror against the header.  The restatement was written from
reading upstream; nothing here was compared with fast_gicp, Sophus, Eigen or PCL themselves."""
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

import gicp_restated as gr  # noqa: E402
from mulls_amd import abi, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "gicp_cases.npz")
INT_FIELDS = ("code", "iterations", "converged", "stop", "n_src", "n_tgt", "n_voxels", "n_corr")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gh") / "gicp_math_harness")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "gicp_math_harness.cpp"), "-o", exe])

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
    import make_gicp_golden

    return make_gicp_golden.compute()


def test_fixture_equals_the_restatement(golden, fresh):
    z, _ = golden
    assert sorted(fresh) == sorted(z)
    for k in z:
        a, b = z[k], fresh[k]
        if a.dtype.kind in "US":
            assert str(a) == str(b), k
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


# ---- 2. gicp_math.h on the host against the restatement, on the fixture's recorded inputs

@pytest.mark.parametrize("case", ["street", "crafted"])
def test_harness_gives_the_restatements_bits(harness, golden, case):
    z, _ = golden
    m = lambda k: z["math/%s/%s" % (case, k)]
    prm = gr.default_params(**json.loads(str(z[case + "/prm"])))
    k = prm["k_correspondences"]
    assert m("cov_in").shape[1:] == (k, 3) and len(m("cov_in")) == 40
    assert same_bits(harness(["cov", k], m("cov_in"), 6), m("cov_out"))
    assert same_bits(harness(["exp"], m("exp_in"), 9), m("exp_out"))
    assert same_bits(harness(["explog"], m("exp_in"), 3), m("log_out"))
    assert len(m("term_in")) >= 20 and same_bits(harness(["term"], m("term_in"), 28), m("term_out"))
    got = harness(["step"], m("step_in"), 7)
    assert same_bits(got, m("step_out"))
    assert got[-1, 6] == 0.0 and got[:-1, 6].all()  # the zero matrix has no pivot; the recorded systems have
    run = harness(["run", prm["max_iterations"], repr(prm["rotation_epsilon"]), repr(prm["transformation_epsilon"])] + [repr(float(np.float32(v))) for v in prm["start_rotvec"]],
                  m("run_in"), 21)
    assert same_bits(run, m("run_out"))
    assert run[-1, 20] == 0.0 and (run[:-1, 20] == 1.0).all()  # runs until the last recorded evaluation
    # street converges; crafted, whose lattice points sit on voxel faces, steps to and fro until max_iterations
    assert (run[-1, 18], run[-1, 19], len(run)) == ((1.0, gr.STOP_CONVERGED, 10) if case == "street" else (0.0, gr.STOP_MAX_ITERATIONS, 64))


def test_pieces_against_numpy(golden):
    """the restatement's pieces against plain numpy: exp against Rodrigues' formula, log(exp(w)) = w, the PLANE covariance's eigenvalues (1, 1, 0.01)
    and its normal against numpy's eigenvectors, the step against numpy.linalg.solve.  Bounds: a few hundred ulp of the quantities involved."""
    z, _ = golden
    for w in z["math/street/exp_in"]:
        R = np.array(gr.so3_exp(w)).reshape(3, 3)
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        ref = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        assert np.abs(R - ref).max() < 1e-14 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14
        assert np.abs(np.array(gr.so3_log(list(R.reshape(-1)))) - w).max() < 1e-13
    for Q, c in zip(z["math/street/cov_in"], z["math/street/cov_out"]):
        Cm = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
        ev, evec = np.linalg.eigh(Cm)
        assert np.allclose(ev, [0.01, 1.0, 1.0], atol=1e-12)
        sv, svec = np.linalg.eigh(np.cov(Q.T))
        if sv[0] < 0.5 * sv[1]:  # a distinct smallest direction: the normal
            assert abs(abs(evec[:, 0] @ svec[:, 0]) - 1.0) < 1e-8
    iu = np.triu_indices(6)
    for s, d in zip(z["math/street/step_in"][:-1], z["math/street/step_out"][:-1]):
        H = np.zeros((6, 6))
        H[iu] = s[:21]
        H = H + np.triu(H, 1).T
        assert np.allclose(H @ d[:6], s[21:27], rtol=0, atol=1e-9 * np.abs(s[21:27]).max() * np.linalg.cond(H))


# ---- 3. which case takes which path

def test_cases_cover_the_paths(golden):
    z, names = golden
    assert names == ["street", "street_guess", "street_near_identity", "street_crop", "street_2m", "street_half", "street_k5", "street_k32", "street_max_iter",
                     "street_tight", "street_large", "crafted", "exact_k", "k_plus_1", "too_few", "no_overlap", "outliers"]
    I = {n: dict(zip(INT_FIELDS, z[n + "/ints"])) for n in names}
    T = lambda n: z[n + "/T"].tobytes()
    for n in names:
        if n not in ("street_max_iter", "too_few", "no_overlap", "crafted"):
            assert I[n]["converged"] == 1 and I[n]["stop"] == gr.STOP_CONVERGED and 0 < I[n]["iterations"] < 63, n
    assert I["street"]["n_src"] == 400 and I["street"]["n_tgt"] == 1500 and I["street_large"]["n_src"] == 1200 and I["street_large"]["n_tgt"] == 3000
    assert T("street_near_identity") == T("street") and T("street_guess") != T("street")
    assert I["street_crop"]["n_src"] < 400 and T("street_crop") != T("street")
    assert I["street_2m"]["n_voxels"] < I["street"]["n_voxels"] < I["street_half"]["n_voxels"]
    assert len({T(n) for n in ("street", "street_2m", "street_half", "street_k5", "street_k32")}) == 5
    cr = I["crafted"]
    assert cr["converged"] == 0 and cr["iterations"] == 63 and cr["stop"] == gr.STOP_MAX_ITERATIONS  # every one of the 64 ticks
    mi = I["street_max_iter"]
    assert mi["converged"] == 0 and mi["iterations"] == 2 and mi["stop"] == gr.STOP_MAX_ITERATIONS
    assert I["exact_k"]["n_src"] == 20 and I["k_plus_1"]["n_src"] == 21 and I["exact_k"]["n_corr"] > 0
    tf = I["too_few"]
    assert tf["n_src"] == 19 and tf["code"] == -3 and tf["stop"] == gr.STOP_NONE and tf["converged"] == 0 and T("too_few") == z["too_few/guess"].tobytes()
    assert z["too_few/floats"][0] == gr.DBL_MAX
    no = I["no_overlap"]
    assert no["n_corr"] == 0 and no["stop"] == gr.STOP_SINGULAR and no["iterations"] == 0 and no["converged"] == 0 and no["n_voxels"] > 0
    assert T("no_overlap") == z["no_overlap/guess"].tobytes()  # (the case starts the loop from r = 0: the pose it keeps is the guess)
    # outliers: points whose 20th neighbour lies beyond three cells of 1 m, in both clouds: no ring walk can certify them
    for cloud, few in ((z["outliers/tgt"], 4), (z["outliers/src"], 3)):
        d = cloud[-few:, None, :] - cloud[None, :, :]
        d2 = np.sort((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2], axis=1)
        assert (d2[:, 19] > 9.0 * 100).all()
    # crafted: points on voxel faces on both sides of 0, voxels of one point, ties in (d2, index), equal eigenvalues, colliding keys
    tgt, src = z["crafted/tgt"], z["crafted/src"]
    assert np.array_equal(tgt * 8, np.round(tgt * 8)) and np.array_equal(src * 8, np.round(src * 8))
    q = tgt[:, 0].astype(np.float32) / np.float32(1.0) - np.float32(0.5)
    assert ((q == np.floor(q)) & (tgt[:, 0] > 0)).any() and ((q == np.floor(q)) & (tgt[:, 0] < 0)).any()
    coords, ok = gr.voxel_coords(tgt, 1.0)
    assert ok.all() and (coords < 0).any() and (coords > 0).any()
    keys = [gr.pack(c) for c in coords]
    counts = {k: keys.count(k) for k in set(keys)}
    assert sum(1 for v in counts.values() if v == 1) >= 3 and max(counts.values()) >= 25
    lg = gr.table_log2(len(tgt))
    homes = [gr.home_slot(k, lg) for k in counts]
    assert lg == 10 and len(set(homes)) < len(homes)  # two occupied voxels share a home slot: the probe sequence runs
    nb = gr.neighbours(tgt, 20)
    ties = same_point = equal_eigen = 0
    for i in range(len(tgt)):
        d = tgt - tgt[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside, rest = d2[nb[i]], np.delete(d2, nb[i])
        ties += int(inside.max() == rest.min())  # the index decided who is the 20th
        same_point += int((d2 == 0).sum() > 20)
        Q = [[float(v) for v in row] for row in tgt[nb[i]].astype(np.float64)]
        m = np.mean(Q, axis=0)
        S = sum(np.outer(r - m, r - m) for r in np.array(Q))
        ev = gr.plane_covariance([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])[1]
        equal_eigen += int(ev[1] == ev[2] or ev[0] == ev[1])
    assert ties >= 10 and same_point >= 25 and equal_eigen >= 10, (ties, same_point, equal_eigen)


# ---- 4. a condition on the street scene

def test_street_ends_nearer_to_the_truth_than_it_starts(golden):
    """the restatement's final pose on `street` is nearer to the scene's ground truth than the start (the identity), in translation and in rotation
    angle.  A condition on the scene, not an accuracy claim; the two errors are printed (and written into DESIGN.md 7.9)."""
    import gicp_scenes

    z, _ = golden
    _, T_gt = gicp_scenes.build_cases()
    dt, dr = synth.pose_error(z["street/T"], T_gt)
    dt0, dr0 = synth.pose_error(np.eye(4), T_gt)
    print("street: %.4f m, %.5f rad from the truth at the end; %.4f m, %.5f rad at the start" % (dt, dr, dt0, dr0))
    assert dt < dt0 and dr < dr0


# ---- 5. the ctypes mirror

def test_ctypes_layout_matches_header():
    fields = {"mulls_gicp_params": abi.GicpParams, "mulls_gicp_problem": abi.GicpProblem, "mulls_gicp_result": abi.GicpResult}
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "mulls_hip.h"', "int main(void){"]
    for cname, ct in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog.append('printf("stop %d %d %d %d\\n", MULLS_GICP_STOP_NONE, MULLS_GICP_STOP_CONVERGED, MULLS_GICP_STOP_MAX_ITERATIONS, MULLS_GICP_STOP_SINGULAR);')
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
    assert [int(v) for v in got["stop"]] == [abi.GICP_STOP_NONE, abi.GICP_STOP_CONVERGED, abi.GICP_STOP_MAX_ITERATIONS, abi.GICP_STOP_SINGULAR]
    assert [int(v) for v in got["stop"]] == [gr.STOP_NONE, gr.STOP_CONVERGED, gr.STOP_MAX_ITERATIONS, gr.STOP_SINGULAR]


def test_default_params_match():
    from mulls_amd import lib

    p = abi.GicpParams()
    lib.load().mulls_gicp_default_params(C.byref(p))
    q, r = abi.gicp_params(), gr.default_params()
    for name, _ in abi.GicpParams._fields_:
        a, b = getattr(p, name), getattr(q, name)
        if name == "start_rotvec":
            assert list(a) == list(b) == r[name], name
            continue
        assert a == b, name
        if name in r:
            assert a == r[name], name


# ---- the bridge

from test_ncc import REF_UTILITY  # noqa: E402  (where the reference tree is looked for)
from test_ndt import BRIDGE_TU  # noqa: E402

GICP_CALLS = r"""
// the calls of test/mulls_slam.cpp:638 and :675, and the batch form
int call_gicp(lo::constraint_t &con, std::vector<lo::constraint_t> &cons, Eigen::Matrix4d guess)
{
	int a = lo::hip::omp_gicp<Point_T>(con, 20, 1.5, true, 1.0, guess, false, 10.0);
	int b = lo::hip::omp_gicp<Point_T>(con);
	std::vector<int> c = lo::hip::omp_gicp_batch<Point_T>(cons, 2.0f);
	return a + b + (int)c.size();
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_against_the_reference_types():
    """lo::hip::omp_gicp and omp_gicp_batch on the reference's constraint_t, as tests/test_ndt.py checks the NDT bridge.  A compile check: running the
    bridge needs the reference tree and a device together, which no test machine has."""
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 592, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(BRIDGE_TU + GICP_CALLS)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
