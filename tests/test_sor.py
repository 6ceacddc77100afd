"""CPU tests of the statistical outlier removal's definition (include/mulls_hip.h: mulls_sor_filter) as tests/sor_restated.py restates
it: the two neighbour searches against each other, an analytic lattice, the pinned fixture tests/golden/sor_cases.npz, the product's own arithmetic
(mulls_amd/csrc/sor_math.h built for the CPU) bit for bit, the ABI mirror, the bridge's signatures, and the condition that makes the library's choice of the
double square root irrelevant to every committed expectation.  The device is compared with the same restatement in tests/test_gpu_sor.py.

PCL is not available where these tests run: nothing here or on the device was compared with PCL itself."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import sor_restated as sr
from mulls_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "sor_cases.npz")

try:
    import scipy.spatial  # noqa: F401

    HAVE_SCIPY = True
except ImportError:
    HAVE_SCIPY = False
needs_scipy = pytest.mark.skipif(not HAVE_SCIPY, reason="scipy (cKDTree, the large cases' neighbour search) is not importable")


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(FIXTURE, allow_pickle=False)


def fixture_case(name):
    Z = fixture()
    n, n_kept = (int(v) for v in Z[name + "_n"])
    keep = np.unpackbits(Z[name + "_keep"])[:n].astype(bool)
    mean, stddev, thr = (np.float64(v) for v in Z[name + "_stats"])
    return dict(n=n, n_kept=n_kept, keep=keep, kept_idx=np.flatnonzero(keep).astype(np.int32), mean=mean, stddev=stddev, threshold=thr,
                sha=Z[name + "_sha"].tobytes(), dist=Z[name + "_dist"] if name + "_dist" in Z.files else None)


@functools.lru_cache(maxsize=None)
def large_case(name):
    """(xyz, restatement with the double sqrt, restatement with the float sqrt) of a large case, computed once"""
    xyz = sr.LARGE_CASES[name](GOLDEN)
    r = sr.restate(xyz, 20, 2.0)
    return xyz, r, sr.restate(xyz, 20, 2.0, float_sqrt=True, d2_sorted=r["d2"])


def bits(x):
    return np.asarray(x, np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------------------- the restatement
@needs_scipy
@pytest.mark.parametrize("n,mean_k", [(22, 20), (500, 1), (3000, 8), (3000, 20), (3000, 64)])
def test_two_searches_agree(n, mean_k):
    rng = np.random.default_rng(n + mean_k)
    xyz = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    xyz[: n // 10] = xyz[n // 10: 2 * (n // 10)]  # some coincident points
    a, b = sr.restate(xyz, mean_k, 1.0, method="brute"), sr.restate(xyz, mean_k, 1.0, method="tree")
    assert np.array_equal(a["d2"], b["d2"]) and a["dist"].tobytes() == b["dist"].tobytes()
    assert bits(a["threshold"]) == bits(b["threshold"]) and np.array_equal(a["keep"], b["keep"])


def test_lattice_is_analytic():
    """a cubic lattice of spacing a, mean_k 6: interior points have their six face neighbours at exactly a; one planted far point is the only one removed"""
    a, m = 0.5, 12
    g = np.arange(m, dtype=np.float64) * a
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    xyz = np.concatenate([xyz, np.array([[40.0, 41.0, 42.0]], np.float32)])
    r = sr.restate(xyz, 6, 2.0)
    ijk = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    interior = np.concatenate([((ijk > 0) & (ijk < m - 1)).all(1), [False]])
    assert (r["dist"][interior] == np.float32(a)).all()
    assert (r["dist"][:-1] <= np.float32(a * (3 + 3 * np.sqrt(2)) / 6) * (1 + 1e-6)).all()  # a corner: three at a, three at a sqrt 2
    assert list(np.flatnonzero(~r["keep"])) == [len(xyz) - 1]


def test_statistics_follow_the_arithmetic():
    """equal distances: the variance is zero or a rounding residue of either sign; a negative one gives a NaN threshold and every point passes"""
    for v in (0.1, 0.3, 1.7, 123.456):
        for n in (22, 1000, 20001):
            d = np.full(n, v, np.float32)
            mean, stddev, thr = sr.statistics(d, 2.0)
            s, q = sr.sums(d)
            var = (q - s * s / n) / (n - 1.0)
            assert (np.isnan(thr) and var < 0) or (var >= 0 and thr == mean + 2.0 * np.sqrt(var))
            keep = ~(d.astype(np.float64) > thr)
            if np.isnan(thr):
                assert keep.all()
    d = np.random.default_rng(3).uniform(0, 1, 100000).astype(np.float32)
    s, q = sr.sums(d)
    assert abs(s - d.astype(np.float64).sum()) < 1e-9 * s and abs(q - (d * d).astype(np.float64).sum()) < 1e-9 * q


# ---------------------------------------------------------------------------------------------------------------- the fixture
@needs_scipy
@pytest.mark.parametrize("name", sorted(sr.LARGE_CASES))
def test_fixture_equals_restatement(name):
    xyz, r, _ = large_case(name)
    want = fixture_case(name)
    assert len(xyz) == want["n"] and int(r["keep"].sum()) == want["n_kept"]
    assert hashlib.sha256(r["dist"].tobytes()).digest() == want["sha"]
    assert bits([r["mean"], r["stddev"], r["threshold"]]) == bits([want["mean"], want["stddev"], want["threshold"]])
    assert np.array_equal(r["keep"], want["keep"])
    if want["dist"] is not None:
        assert want["dist"].tobytes() == r["dist"].tobytes()


@needs_scipy
@pytest.mark.parametrize("name", sorted(sr.LARGE_CASES))
def test_fixture_does_not_depend_on_the_sqrt_reading(name):
    """the keep mask is the same under the float and the double reading of PCL's unqualified sqrt, and no distance is within a float ulp's reach of the threshold"""
    _, r, rf = large_case(name)
    assert np.array_equal(r["keep"], rf["keep"])
    assert sr.gap(r) > 1e-6 and sr.gap(rf) > 1e-6  # a float ulp moves a distance by about 1e-7 relative
    assert 0 < (~r["keep"]).sum() < len(r["keep"]) // 10


def test_fixture_sizes():
    Z = fixture()
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert sorted(k.rsplit("_", 1)[0] for k in Z.files if k.endswith("_stats")) == sorted(sr.LARGE_CASES)
    assert fixture_case("scan7")["n"] == 28800 and fixture_case("scan3")["n"] == 121586 and fixture_case("map8")["n"] > 900000
    assert fixture_case(sr.KEEPS_DIST)["dist"] is not None


# ---------------------------------------------------------------------------------------------------------------- the product's own code, built for the CPU
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """mulls_amd/csrc/sor_math.h (distance, k-best insertion, mean distance, summation order, certificate: the text the kernels compile) behind C entry points"""
    so = str(tmp_path_factory.mktemp("sor_harness") / "sor_harness.so")
    subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "sor_harness.cpp"), "-o", so])
    L = C.CDLL(so)
    L.sh_mean_dists.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sh_mean_dist_list.argtypes = [C.c_void_p, C.c_int]
    L.sh_mean_dist_list.restype = C.c_float
    L.sh_statistics.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_void_p]
    L.sh_keeps.argtypes = [C.c_float, C.c_double]
    L.sh_certified.argtypes = [C.c_float, C.c_int, C.c_double]
    L.sh_cell.argtypes = [C.c_float, C.c_double, C.c_double]
    L.sh_cell.restype = C.c_longlong
    return L


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("mean_k,cap", [(1, 9), (8, 9), (8, 17), (16, 17), (20, 33), (32, 33), (20, 65), (64, 65)])
def test_product_kbest_equals_restatement(harness, mean_k, cap):
    """SorKBest of every capacity the kernels instantiate, fed every point of clouds with ties and coincident points: mean_dist bit for bit, and its worst
    entry is the (mean_k + 1)-th smallest squared distance"""
    rng = np.random.default_rng(100 * mean_k + cap)
    for n, scale in ((mean_k + 1, 1.0), (300, 1.0), (1200, 1e5)):
        xyz = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
        xyz[: n // 7] = np.round(xyz[: n // 7])  # lattice points: exact ties and coincident points
        xyz = (xyz + np.float32(scale if scale > 1 else 0)).astype(np.float32)
        r = sr.restate(xyz, mean_k, 2.0, method="brute")
        dist, worst = np.zeros(n, np.float32), np.zeros(n, np.float32)
        assert harness.sh_mean_dists(vp(np.ascontiguousarray(xyz)), n, mean_k, cap, vp(dist), vp(worst)) == 0
        assert dist.tobytes() == r["dist"].tobytes(), (n, scale)
        assert np.array_equal(worst, r["d2"][:, mean_k])
        row = np.ascontiguousarray(r["d2"][n // 2])
        assert np.float32(harness.sh_mean_dist_list(vp(row), mean_k + 1)) == r["dist"][n // 2]


def test_product_statistics_equal_restatement(harness):
    rng = np.random.default_rng(9)
    for n in (2, 21, 16383, 16384, 16385, 100000, 1000003):
        for std_mul in (-1.0, 0.0, 2.0):
            d = (rng.uniform(0, 1, n) ** 3 * 5).astype(np.float32)
            if n == 21:
                d[:] = np.float32(0.3)  # equal distances: the variance is a rounding residue
            out = np.zeros(5, np.float64)
            harness.sh_statistics(vp(d), n, std_mul, vp(out))
            s, q = sr.sums(d)
            mean, stddev, thr = sr.statistics(d, std_mul)
            assert bits(out[:2]) == bits([s, q]), n
            for a, b in zip(out[2:], (mean, stddev, thr)):
                assert bits(a) == bits(b) or (np.isnan(a) and np.isnan(b)), (n, std_mul)
            for v in d[:50]:
                assert bool(harness.sh_keeps(float(v), float(thr))) == (not (np.float64(v) > thr))
    assert harness.sh_keeps(1e30, float("nan")) == 1


def test_certificate_is_conservative(harness):
    """whatever lies outside the rings <= R of a query's cell is, in float arithmetic, no nearer than what the certificate admits"""
    rng = np.random.default_rng(4)
    for edge, lo, span in ((0.37, -50.0, 100.0), (0.011, 99990.0, 30.0), (3.3, -4000.0, 9000.0)):
        inv = 1.0 / edge
        q = (lo + rng.uniform(0, span, (400, 3))).astype(np.float32)
        p = (q + rng.normal(0, 2.5 * edge, (400, 3))).astype(np.float32)
        for R in (0, 1, 2, 3):
            for a, b in zip(q, p):
                ca = [harness.sh_cell(float(v), lo - 1.0, inv) for v in a]
                cb = [harness.sh_cell(float(v), lo - 1.0, inv) for v in b]
                if max(abs(x - y) for x, y in zip(ca, cb)) <= R:
                    continue  # scanned
                d2 = sr.d2_f32(a[None], b[None])[0, 0]
                # an unscanned point's distance must never be below a certified k-th best: anything certified is <= the bound, so d2 must exceed it
                assert not harness.sh_certified(float(np.nextafter(d2, np.float32(0))), R, edge) or R == 0 and d2 == 0, (edge, R)
    assert harness.sh_certified(0.0, 0, 1.0) == 1 and harness.sh_certified(1e-30, 0, 1.0) == 0
    assert harness.sh_certified(float("inf"), 3, 1.0) == 0 and harness.sh_certified(0.99, 1, 1.0) == 1 and harness.sh_certified(1.0, 1, 1.0) == 0


# ---------------------------------------------------------------------------------------------------------------- ABI and bridge
def test_abi_mirror():
    fields = {"mulls_sor_params": (abi.SorParams, [f[0] for f in abi.SorParams._fields_]),
              "mulls_sor_report": (abi.SorReport, [f[0] for f in abi.SorReport._fields_])}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){"]
    for cname, (_, names) in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in names:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
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
    assert C.sizeof(abi.SorParams) == 16 and abi.SorParams.std_mul.offset == 8
    assert C.sizeof(abi.SorReport) == 40 and abi.SorReport.mean.offset == 8 and abi.SorReport.ms_total.offset == 32 and abi.SorReport.n_fallback.offset == 36
    for name in ("mulls_sor_default_params", "mulls_sor_filter"):
        assert name in lib.EXPORTS


def test_default_params_and_constants(harness):
    p = abi.SorParams()
    lib.load().mulls_sor_default_params(C.byref(p))
    q = abi.sor_params()
    assert (p.mean_k, p.reserved, p.std_mul) == (q.mean_k, q.reserved, q.std_mul) == (20, 0, 2.0)  # mulls_slam.cpp:1009
    assert harness.sh_constants(0) == 64 and harness.sh_constants(1) == 1 << 24 and harness.sh_constants(2) == sr.PARTIALS


from test_ransac import BRIDGE_TU, REF_UTILITY  # noqa: E402  (the shim prelude and where the reference tree is looked for)

SOR_TU = BRIDGE_TU.split("// the call of")[0] + r"""
// the call of test/mulls_slam.cpp:1009, and the two signatures of cfilter.hpp:204 and :225
bool call(pcTPtr pc_map_merged, pcTPtr cloud_out)
{
	bool a = lo::hip::sor_filter<Point_T>(pc_map_merged, 20, 2.0);
	bool b = lo::hip::sor_filter<Point_T>(pc_map_merged, cloud_out, 20, 2.0);
	int mean_k = 10;
	double n_std = 1.5;
	return a && b && lo::hip::sor_filter<Point_T>(pc_map_merged, cloud_out, mean_k, n_std);
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_with_the_reference_call():
    """lo::hip::sor_filter with upstream's two signatures, against the shim headers (syntax only: running it needs a mode in oracle/adapter_check.cpp, which this
    change leaves alone; the bridge is a dozen lines around mulls_sor_filter, which tests/test_gpu_sor.py covers)"""
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 590, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(SOR_TU)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
