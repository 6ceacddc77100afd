"""CPU tests of the FPFH descriptor and the FPFH-based SAC-IA coarse registration (mulls_fpfh, mulls_coarse_reg_fpfhsac): mulls_amd/csrc/fpfh_math.h,
compiled for the host as a stand-alone program, against the numpy restatement tests/fpfh_restated.py with equal bits on the fixture's recorded inputs;
the fixture tests/golden/fpfh_cases.npz against the restatement; which scene reaches which edge; analytic anchors of the restatement itself; the ctypes mirror is held
against the header in tests/test_fpfh_abi.py, which needs no mpmath.  The restatement was written from the header's definition; nothing here was compared with PCL, FLANN or Eigen."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

mpmath = pytest.importorskip("mpmath")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import fpfh_restated as fr  # noqa: E402
import fpfh_scenes  # noqa: E402
from fpfh_names import FLOAT_FIELDS, FPFH_CASES, GOLDEN, INT_FIELDS, SAC_CASES  # noqa: E402,F401
from make_fpfh_golden import DRAWS  # noqa: E402
from mulls_amd import abi, synth  # noqa: E402



@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fh") / "fpfh_math_harness")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "fpfh_math_harness.cpp"), "-o", exe])

    def run(args, data, width):
        out = subprocess.run([exe] + [str(a) for a in args], input=np.ascontiguousarray(data, np.float64).tobytes(), stdout=subprocess.PIPE, check=True).stdout
        return np.frombuffer(out, np.float64).reshape(-1, width)

    return run


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def sac_prm(g, name):
    return fr.fpfhsac_default_params(**json.loads(str(g[name + "/prm"])))


# ---- 1. the fixture

def test_fixture_equals_the_restatement(golden):
    import make_fpfh_golden

    fresh = make_fpfh_golden.compute()
    assert sorted(fresh) == sorted(golden)
    for k in golden:
        a, b = golden[k], fresh[k]
        if a.dtype.kind in "US":
            assert str(a) == str(b), k
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


# ---- 2. fpfh_math.h on the host against the restatement, on the fixture's recorded inputs

def test_harness_gives_the_restatements_bits(harness, golden):
    m = lambda k: golden["math/" + k]
    got = harness(["pair"], m("pair_in"), 7)
    assert len(got) > 1000 and same_bits(got, m("pair_out"))
    assert (got[:, 0] == 0.0).sum() >= 10 and (got[:, 0] == 1.0).sum() >= 1000  # pairs that add nothing (f4 = 0, |v| = 0) and pairs that do
    assert same_bits(harness(["bins"], m("bins_in"), 4), m("bins_out"))
    assert len(m("spfh_in")) > 1000 and same_bits(harness(["spfh"], m("spfh_in"), 1), m("spfh_out"))
    assert len(m("norm_in")) > 100 and same_bits(harness(["norm"], m("norm_in"), 33), m("norm_out"))
    assert len(m("error_in")) == 360 and same_bits(harness(["error"], m("error_in"), 1), m("error_out"))
    assert same_bits(harness(["dist"], m("dist_in"), 1), m("dist_out"))
    assert len(m("order_in")) == 72 and same_bits(harness(["order"], m("order_in"), 1), m("order_out"))  # NaN after every number, equal errors by index


@pytest.mark.parametrize("name,iters", DRAWS)
def test_harness_draws_the_restatements_sequence(harness, golden, name, iters):
    args = golden["math/draw/%s/args" % name]
    n, k_eff, it, seed = int(args[0]), int(args[1]), int(args[2]), int(args[4])
    assert it == iters
    got = harness(["draw", n, k_eff, it, repr(float(args[3])), seed], golden[name + "/src"][:n].astype(np.float64), 6)
    assert same_bits(got, golden["math/draw/%s/out" % name])
    assert (got[:-1, :3].astype(np.int64) == golden[name + "/samples"]).all()


def test_bins_at_their_edges(golden):
    """the arithmetic of the bins on features given as doubles that sit exactly on inner edges, 11 x == k, for every k and every feature the search
    of tests/golden/make_fpfh_golden.py finds; fpfh_scenes.bin_edges has clouds that put f3 and f2 exactly on an inner edge (EXACT_EDGES), the outer
    edges, and f2 a float ulp either side of an inner edge, which the device runs (tests/test_gpu_fpfh.py)"""
    rows, out = golden["math/bins_in"], golden["math/bins_out"]
    inner = [(r, o) for r, o in zip(rows, out) if o[0] == 1.0 and abs(r[1]) < 1.0 and abs(r[0]) < 3.0]
    assert len(inner) >= 10
    on_edge = 0
    for r, o in inner:
        x2, x1 = 11.0 * ((r[1] + 1.0) * 0.5), 11.0 * ((r[0] + fr.PI) * fr.INV_2PI)
        if r[1] != 0.0:
            assert x2 == np.floor(x2) and o[2] == x2 and o[3] == x2  # on the edge: the upper bin
            below = r[1] - 1e-12  # (a few doubles around the edge round onto it)
            assert fr.bins_of(np.array([[0.0, below, below]]))[0][0, 1] == x2 - 1
            on_edge += 1
        else:
            assert x1 == np.floor(x1) and o[1] == x1
            on_edge += 1
    assert on_edge >= 10
    b, good = fr.bins_of(np.array([[fr.PI, 1.0, 1.0], [-fr.PI, -1.0, -1.0], [np.nan, 0.0, 0.0]]))
    assert b[0].tolist() == [10, 10, 10] and b[1].tolist() == [0, 0, 0] and good.tolist() == [True, True, False]


# ---- 3. which scene reaches which edge

def test_scenes_reach_their_edges(golden):
    g = golden
    assert json.loads(str(g["fpfh_names"])) == FPFH_CASES and json.loads(str(g["sac_names"])) == SAC_CASES
    H, K, U = (lambda n: g[n + "/hist"]), (lambda n: g[n + "/k"]), (lambda n: g[n + "/pairs_used"])
    assert K("one").tolist() == [1] and not H("one").any()
    assert K("two").tolist() == [2, 2] and H("two").any(axis=1).all()
    assert K("three").tolist() == [2, 2, 1] and not H("three")[2].any()  # no neighbour: all zeros
    dup = g["duplicates/pts"]
    assert len(np.unique(dup, axis=0)) == 13 and K("duplicates")[-3:].tolist() == [3, 3, 3] and not H("duplicates")[-3:].any() and not U("duplicates")[-3:].any()
    assert (U("duplicates")[:12] < K("duplicates")[:12] - 1).any()  # a copy of the point itself is counted in k and adds no pair
    assert (g["normals/nrm"] == 0).all(axis=1).sum() == 3 and K("normals")[-2:].tolist() == [2, 2] and U("normals")[-2:].tolist() == [0, 0]
    assert K("radius_edge").tolist() == [3, 2, 1, 2]  # from the first: exactly at the radius and an ulp inside count, an ulp beyond does not
    d = fr.dist2(g["radius_edge/pts"], g["radius_edge/pts"][0][None, :]).astype(np.float64)
    assert d[1] == 1.0 and d[2] > 1.0 and d[3] < 1.0
    ks = K("sizes")
    for m in fpfh_scenes.SIZES:
        assert (ks == m).sum() == m, m
    assert (ks == 70).sum() == 70
    cells, ok = fr.cells_of(g["sizes/pts"], 1.0)
    assert ok and len(np.unique(cells[ks == 257], axis=0)) == 1 and len(np.unique(cells[ks == 70], axis=0)) == 2  # one cell of 257; a ball across a face
    be = H("bin_edges")
    # (a point's histogram is the weighted sum of its neighbours' SPFH: the pair feature of query 2 j shows in the histogram of 2 j + 1)
    assert be[1, 11 + 10] == 100.0 and be[3, 11 + 0] == 100.0  # f2 = +1 and f2 = -1: the last and the first bin
    assert be[5, 10] == 100.0 and be[7, 0] == 100.0  # f1 = +pi: the last bin; f1 = -pi: the first
    assert U("bin_edges")[8:12].tolist() == [0, 0, 0, 0] and not be[8:12].any()  # f3 = +-1: |v| = 0, the pair adds nothing
    near = [int(np.argmax(be[13 + 2 * j, 11:22])) for j in range(3)]  # f2 a float ulp below, at and above the float next to the edge of bins 2 and 3
    assert near in ([2, 2, 3], [2, 3, 3])
    for j, (_, _, which, k) in enumerate(fpfh_scenes.EXACT_EDGES):  # a feature exactly on an inner edge, 11 x == k: the upper bin
        i = 2 * (fpfh_scenes.N_EDGE_PAIRS + j)
        P, N = g["bin_edges/pts"], g["bin_edges/nrm"]
        f, adds = fr.pair_features(P[i], N[i], P[i + 1:i + 2], N[i + 1:i + 2])
        assert adds[0] and 11.0 * ((f[0, which] + 1.0) * 0.5) == float(k) and fr.bins_of(f)[0][0, which] == k
        lower = f.copy()
        lower[0, which] = np.nextafter(f[0, which], -1.0) - 1e-12
        assert fr.bins_of(lower)[0][0, which] == k - 1
        assert be[i + 1, 11 * which + k] == 100.0 and K("bin_edges")[i] == 2
    cells, ok = fr.cells_of(g["dense_table/pts"], 1.0)
    assert ok and len(g["dense_table/pts"]) == 2000 and len(np.unique(cells, axis=0)) > 1900  # 4 096 slots at a load above 0.46
    # SAC-IA
    I = {n: dict(zip(INT_FIELDS, g[n + "/ints"])) for n in SAC_CASES}
    E = {n: g[n + "/errors"] for n in SAC_CASES}
    assert I["sac_default"]["best_iteration"] == 0 and not E["sac_default"].any() and np.isinf(sac_prm(g, "sac_default")["max_correspondence_distance"])
    assert I["sac_three"]["n_src"] == 3 and I["sac_few_targets"]["n_tgt"] == 7 < sac_prm(g, "sac_few_targets")["k_correspondences"]
    assert g["sac_equal_descriptors/corr"].max() < 15 and len(np.unique(g["sac_equal_descriptors/corr"])) > 5  # every d2 is 0: the index decides
    assert 0.0 < g["sac_halving/min_d"] < 1000.0 and g["sac_it1/min_d"] == 0.0
    assert [I["sac_it%d" % k]["iterations"] for k in (1, 64, 65)] == [1, 64, 65] and I["sac_it65"]["best_iteration"] > 0
    assert I["sac_chunks"]["iterations"] == 1030 > abi.FPFH_HYP_CHUNK and len(np.unique(E["sac_chunks"][abi.FPFH_HYP_CHUNK:])) == 6
    nan = np.isnan(E["sac_nan_errors"])
    assert nan[:3].all() and not nan[3] and nan[3:].any() and I["sac_nan_errors"]["best_iteration"] == 3 and g["sac_nan_errors/floats"][0] == 0.0
    assert (E["sac_equal_error"] == 60.0).all() and I["sac_equal_error"]["best_iteration"] == 0  # equal errors: the first wins
    thr = np.float32(sac_prm(g, "sac_threshold_truncated")["max_correspondence_distance"])
    assert thr == np.float32(sac_prm(g, "sac_threshold_huber")["max_correspondence_distance"]) and (g["sac_threshold_truncated/e2"] == thr).sum() >= 1
    assert g["sac_threshold_truncated/errors"].tobytes() != g["sac_threshold_huber/errors"].tobytes()
    assert (I["sac_recovery"]["n_src"], I["sac_recovery"]["n_tgt"]) == (1200, 1500) and I["sac_recovery"]["best_iteration"] > 0


# ---- 4. analytic anchors of the restatement

def test_sub_histograms_sum_to_100(golden):
    """every non-empty sub-histogram sums to 100 within 1e-3: 11 float roundings of values of at most 100"""
    seen = 0
    for name in FPFH_CASES:
        h = golden[name + "/hist"].astype(np.float64).reshape(-1, 3, 11)
        s = h.sum(axis=2)
        live = h.any(axis=2)
        seen += int(live.sum())
        assert (np.abs(s[live] - 100.0) < 1e-3).all(), (name, np.abs(s[live] - 100.0).max())
        assert (h >= 0).all()
    assert seen > 5000


def test_counts_add_up_to_the_pairs_that_contributed():
    for name in ("duplicates", "normals", "bin_edges", "two"):
        c = fpfh_scenes.fpfh_cases()[name]
        d = {}
        _, k = fr.fpfh(c["pts"], c["nrm"], c["search_radius"], d)
        for s in range(3):
            assert (d["counts"][:, 11 * s:11 * (s + 1)].sum(axis=1) == d["used"]).all(), (name, s)
        assert (d["used"] <= k.astype(np.int64) - 1).all() and (d["used"] < k.astype(np.int64) - 1).any() == (name != "two")


def test_recovery_of_a_known_motion(golden):
    """the source is 1 200 of the target's 1 500 points under the inverse of a known motion; with a finite max_correspondence_distance the restatement
    recovers it to within the scene's point spacing.  Measured: every source point lands within 2.5e-7 m of its place (the float storage of the
    source); the bound is the spacing, 0.25 m."""
    g = golden
    T, M = g["sac_recovery/T"], fpfh_scenes.sac_truth()
    src = g["sac_recovery/src"].astype(np.float64)
    off = np.linalg.norm((src @ T[:3, :3].T + T[:3, 3]) - (src @ M[:3, :3].T + M[:3, 3]), axis=1).max()
    dt, dr = synth.pose_error(T, M)
    print("sac_recovery: the farthest source point is %.3e m from its place; pose error %.3e m, %.3e rad; hypothesis %d of %d" % (
        off, dt, dr, g["sac_recovery/ints"][0], g["sac_recovery/ints"][1]))
    assert np.isfinite(sac_prm(g, "sac_recovery")["max_correspondence_distance"])
    assert off < fpfh_scenes.RECOVERY_SPACING


def test_restatements_defaults_are_the_librarys():
    p, r = abi.fpfhsac_params(), fr.fpfhsac_default_params()
    for name, _ in abi.FpfhSacParams._fields_:
        assert getattr(p, name) == r[name], name
    assert abi.fpfh_params().search_radius == fr.fpfh_default_params()["search_radius"] and (abi.SACIA_TRUNCATED, abi.SACIA_HUBER) == (fr.TRUNCATED, fr.HUBER)
    assert abi.FPFH_DIMS == fr.DIMS and fr.MAX_CELL_POINTS == abi.FPFH_MAX_CELL_POINTS
