"""CPU tests of the key-point non-maximum suppression's definition (include/mulls_hip.h: mulls_non_max_suppress):
the restated walk (tests/nms_restated.py) against clouds the reference's own lines made (tests/golden/demo_pair.npz: the *_down class clouds), the
library's shared (key, index) sort (mulls_amd/csrc/nms_host.h) against a std::sort of whole records (tests/nms_harness.cpp) on inputs full of ties, the
restatement against the harness, the pinned fixture tests/golden/nms_cases.npz, the ABI mirror and the bridge's signatures.  The device is compared with the
harness and the fixture in tests/test_gpu_nms.py.

PCL is not available where these tests run: the radius test restates pcl::search::KdTree::radiusSearch from memory."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import nms_restated as nr
from mulls_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "nms_cases.npz")


class Harness:
    """tests/nms_harness.cpp built for the CPU: upstream's record sort and sequential walk"""

    def __init__(self, so):
        self.L = L = C.CDLL(so)
        vp = C.c_void_p
        L.nh_record_order.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
        L.nh_record_order.restype = None
        L.nh_pair_order.argtypes = [vp, C.c_uint32, vp]
        L.nh_pair_order.restype = None
        L.nh_suppress.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp]

    def record_order(self, recs):
        recs = np.ascontiguousarray(recs)
        order = np.zeros(len(recs), np.int32)
        self.L.nh_record_order(recs.ctypes.data, len(recs), recs.shape[1], order.ctypes.data)
        return order

    def pair_order(self, keys):
        keys = np.ascontiguousarray(keys, np.float32)
        order = np.zeros(len(keys), np.int32)
        self.L.nh_pair_order(keys.ctypes.data, len(keys), order.ctypes.data)
        return order

    def suppress(self, recs, radius):
        """(kept records, kept_idx, order), or None under the gate"""
        recs = np.ascontiguousarray(recs)
        n = len(recs)
        out, idx, order = np.zeros((n, 48), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
        k = self.L.nh_suppress(recs.ctypes.data, n, recs.shape[1], float(radius), out.ctypes.data, idx.ctypes.data, order.ctypes.data)
        return None if k < 0 else (out[:k].copy(), idx[:k].copy(), order)


@functools.lru_cache(maxsize=None)
def build_harness():
    d = tempfile.mkdtemp(prefix="nms_harness_")
    so = os.path.join(d, "nms_harness.so")
    subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "nms_harness.cpp"), "-o", so])
    return Harness(so)


@pytest.fixture(scope="module")
def harness():
    return build_harness()


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(FIXTURE, allow_pickle=False)


@functools.lru_cache(maxsize=None)
def demo_keypoints():
    Z = np.load(os.path.join(GOLDEN, "ncc_demo.npz"), allow_pickle=False)
    return {"kpts_0": np.ascontiguousarray(Z["kpts_0"]), "kpts_15": np.ascontiguousarray(Z["kpts_15"])}


def tie_records(name):
    Z = fixture()
    return nr.make_records(Z[name + "_xyz"], Z[name + "_keys"], seed=len(Z[name + "_keys"]))


# ---------------------------------------------------------------------------------------------------------------- the walk, against the reference's clouds
def test_walk_reproduces_the_reference_down_clouds():
    """the class clouds of the demo scans were left sorted by the reference's own non_max_suppress, the *_down clouds are what its walk kept at
    0.25 * 1.0 m: the restated walk in identity order gives them back bit for bit"""
    D = np.load(os.path.join(GOLDEN, "demo_pair.npz"), allow_pickle=False)
    sizes = []
    for k in (0, 1, 15):
        for cls in ("pillar", "beam", "facade"):
            full, down = D["ex_%d_%s" % (k, cls)], D["ex_%d_%s_down" % (k, cls)]
            kept = nr.walk(full, np.arange(len(full)), 0.25)
            assert full[kept].tobytes() == down.tobytes(), (k, cls)
            sizes.append(len(kept))
    assert sizes == [305, 1035, 815, 332, 984, 801, 336, 903, 915]


# ---------------------------------------------------------------------------------------------------------------- the sort
@pytest.mark.parametrize("levels", [2, 8, 64])
@pytest.mark.parametrize("n", [10, 16, 17, 33, 1000, 5000])
def test_pair_sort_equals_record_sort(harness, n, levels):
    """the (key, index) sort the library runs leaves the permutation std::sort leaves on the 48-byte records (16 / 17: libstdc++'s insertion-sort threshold)"""
    for seed in range(3):
        rng = np.random.default_rng(1000 * n + 10 * levels + seed)
        keys = (np.floor(rng.uniform(0, 1, n) * levels) / levels).astype(np.float32)
        recs = nr.make_records(rng.uniform(-1, 1, (n, 3)), keys, seed)
        a, b = harness.record_order(recs), harness.pair_order(keys)
        assert np.array_equal(a, b), (n, levels, seed)
        assert sorted(a.tolist()) == list(range(n)) and (np.diff(keys[a]) <= 0).all()
        if n >= 1000:
            assert not np.array_equal(a, np.argsort(-keys.astype(np.float64), kind="stable"))  # the tie order is std::sort's, not the stable one
    wide = np.zeros((n, 64), np.uint8)
    wide[:, :48] = recs
    assert np.array_equal(harness.record_order(wide), a)


# ---------------------------------------------------------------------------------------------------------------- restatement against harness
@pytest.mark.parametrize("n,radius", [(10, 0.5), (11, 0.5), (257, 0.3), (1500, 0.25), (1500, 1.0), (1500, 0.0), (1500, -0.25)])
def test_restatement_equals_harness_without_ties(harness, n, radius):
    rng = np.random.default_rng(n)
    xyz = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    recs = nr.make_records(xyz, rng.permutation(n).astype(np.float32) / n, n)
    kept_idx, order, ran = nr.suppress(recs, radius)
    out, h_idx, h_order = harness.suppress(recs, radius)
    assert ran and np.array_equal(order, h_order) and np.array_equal(kept_idx, h_idx) and out.tobytes() == recs[kept_idx].tobytes()
    assert (len(kept_idx) == n) == (radius == 0.0) or n <= 11
    if radius < 0:
        assert np.array_equal(kept_idx, nr.suppress(recs, -radius)[0])


def test_gate(harness):
    recs = nr.make_records(np.zeros((9, 3)), np.arange(9), 1)
    assert harness.suppress(recs, 0.25) is None
    kept_idx, order, ran = nr.suppress(recs, 0.25)
    assert not ran and list(kept_idx) == list(order) == list(range(9))
    assert harness.suppress(nr.make_records(np.zeros((10, 3)), np.arange(10), 1), 0.25)[1].tolist() == [9]  # coincident points: the best key alone


@pytest.mark.parametrize("name", ["kpts_0", "kpts_15"])
@pytest.mark.parametrize("radius", [0.25, 1.0])
def test_demo_keypoints(harness, name, radius):
    """the reference's demo key points: the walk over the harness's order is the harness's result, and the fixture holds it"""
    recs = demo_keypoints()[name]
    out, idx, order = harness.suppress(recs, radius)
    assert np.array_equal(nr.walk(recs, order, radius), idx) and out.tobytes() == recs[idx].tobytes()
    Z = fixture()
    assert np.array_equal(Z["%s_r%g_kept" % (name, radius)], idx) and np.array_equal(Z["%s_order" % name], order)
    keys = nr.keys_of(recs)
    if radius == 0.25:
        # with equal keys taken in input order (a stable sort) the walk keeps 913 and 851; in std::sort's order, the one upstream visits in, 915 and 851
        stable = np.argsort(-keys.astype(np.float64), kind="stable")
        assert len(nr.walk(recs, stable, radius)) == {"kpts_0": 913, "kpts_15": 851}[name]
        assert len(idx) == {"kpts_0": 915, "kpts_15": 851}[name]
    assert len(recs) - len(np.unique(keys)) == {"kpts_0": 74, "kpts_15": 43}[name]  # equal keys: the order among them is std::sort's


@pytest.mark.parametrize("name", sorted(nr.TIE_CASES))
def test_fixture_tie_cases(harness, name):
    """the fixture's synthetic inputs are the seeded ones, its indices the harness's"""
    Z = fixture()
    xyz, keys = nr.tie_cloud(name)
    assert Z[name + "_xyz"].tobytes() == xyz.tobytes() and Z[name + "_keys"].tobytes() == keys.tobytes()
    recs = tie_records(name)
    radius = nr.TIE_CASES[name][4]
    out, idx, order = harness.suppress(recs, radius)
    assert np.array_equal(Z[name + "_kept"], idx) and np.array_equal(Z[name + "_order"], order)
    assert np.array_equal(nr.walk(recs, order, radius), idx)
    assert len(np.unique(keys)) <= nr.TIE_CASES[name][2] and 1 < len(idx) < len(recs)


def test_fixture_size():
    assert os.path.getsize(FIXTURE) < 200 << 10


# ---------------------------------------------------------------------------------------------------------------- ABI and bridge
def test_abi_mirror():
    fields = {"mulls_nms_params": (abi.NmsParams, [f[0] for f in abi.NmsParams._fields_]),
              "mulls_nms_report": (abi.NmsReport, [f[0] for f in abi.NmsReport._fields_])}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){"]
    for cname, (_, names) in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in names:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog.append('printf("max %u\\nlds %u\\n", MULLS_NMS_MAX_POINTS, MULLS_NMS_LDS_MAX_POINTS);')
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
    assert C.sizeof(abi.NmsParams) == 8 and C.sizeof(abi.NmsReport) == 24
    assert int(got["max"]) == abi.NMS_MAX_POINTS == 1 << 18 and int(got["lds"]) == abi.NMS_LDS_MAX_POINTS >= 4096
    for name in ("mulls_nms_default_params", "mulls_non_max_suppress"):
        assert name in lib.EXPORTS


def test_default_params():
    p = abi.NmsParams()
    lib.load().mulls_nms_default_params(C.byref(p))
    q = abi.nms_params()
    assert (p.non_max_radius, p.path) == (q.non_max_radius, q.path) == (0.25, 0)


from test_ransac import BRIDGE_TU, REF_UTILITY  # noqa: E402  (the shim prelude and where the reference tree is looked for)

NMS_TU = BRIDGE_TU.split("// the call of")[0] + r"""
// the calls of test/mulls_reg.cpp:147 and test/mulls_slam.cpp:462, and the signatures of cfilter.hpp:1183 and :1243
bool call(pcTPtr pc_vertex, pcTPtr cloud_down, pcTreePtr tree_vertex, float keypoint_nms_radius)
{
	bool a = lo::hip::non_max_suppress<Point_T>(pc_vertex, keypoint_nms_radius);
	bool b = lo::hip::non_max_suppress<Point_T>(pc_vertex, keypoint_nms_radius, false, tree_vertex);
	bool c = lo::hip::non_max_suppress<Point_T>(pc_vertex, cloud_down, keypoint_nms_radius);
	bool d = lo::hip::non_max_suppress<Point_T>(pc_vertex, cloud_down, keypoint_nms_radius, false, 35.0, false, tree_vertex);
	return a && b && c && d;
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_with_the_reference_call():
    """lo::hip::non_max_suppress with upstream's two cloud signatures and defaults, against the shim headers (syntax only: running it needs a mode in
    oracle/adapter_check.cpp, which this change leaves alone; the bridge is a few lines around mulls_non_max_suppress, which tests/test_gpu_nms.py covers)"""
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 590, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(NMS_TU)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
