"""GPU tests of mulls_fpfh and mulls_coarse_reg_fpfhsac through mulls_amd/lib.py against the numpy restatement of the library's definition
(tests/fpfh_restated.py), read from tests/golden/fpfh_cases.npz (tests/test_fpfh.py keeps the fixture equal to the restatement and asserts which
scene reaches which edge).

Every comparison is equality of bits: of the 33 floats and the neighbourhood's size of every point, and of T, best_error, fitness and the integer
fields.  The definition has no operation whose host and device results may differ (+ - * / sqrt in double or float in a stated order, atan2 from
detmath.h, integer counts, no contraction), and the restatement's searches are brute force, so equal bits also say that the 27-cell walks are exact.

PCL, FLANN and Eigen are not available where these tests run: nothing here was compared with them."""
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from mulls_amd import abi, lib
from fpfh_names import FLOAT_FIELDS, FPFH_CASES, GOLDEN, INT_FIELDS, ROOT, SAC_CASES

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -100, -103


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def fpfh_args(g, name):
    return (g[name + "/pts"], g[name + "/nrm"]), abi.fpfh_params(float(g[name + "/search_radius"]))


def sac_args(g, name, **over):
    prm = json.loads(str(g[name + "/prm"]))
    prm.update(over)
    return (g[name + "/tgt"], g[name + "/tgt_nrm"]), (g[name + "/src"], g[name + "/src_nrm"]), abi.fpfhsac_params(**prm)


def key(res):
    """everything a result holds, as bytes"""
    return (tuple(getattr(res, k) for k in INT_FIELDS), np.array([getattr(res, k) for k in FLOAT_FIELDS]).tobytes(), np.array(res.T).tobytes())


def pose(res):
    return np.array(res.T).reshape(4, 4).T


def check_sac(res, g, name, what=None):
    what = what or name
    for k, v in zip(INT_FIELDS, g[name + "/ints"]):
        assert getattr(res, k) == v, (what, k, getattr(res, k), v)
    got = np.array([getattr(res, k) for k in FLOAT_FIELDS])
    assert got.tobytes() == g[name + "/floats"].tobytes(), (what, got, g[name + "/floats"])
    assert pose(res).tobytes() == g[name + "/T"].tobytes(), (what, np.abs(pose(res) - g[name + "/T"]).max())


def check_fpfh(got, g, name, what=None):
    hist, k = got
    assert k.tobytes() == g[name + "/k"].tobytes(), (what or name, np.flatnonzero(k != g[name + "/k"])[:8])
    want = g[name + "/hist"]
    assert hist.shape == want.shape and hist.tobytes() == want.tobytes(), (what or name, np.argwhere(hist != want)[:8], np.abs(hist - want).max())


class DevRecords:
    """records in a device allocation of the caller's own (straight from the HIP runtime the library runs on): the coordinates at floats 0 .. 2 and the
    normals at floats 4 .. 6 of a stride of the caller's choice"""

    def __init__(self, pts, nrm, stride_floats):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        buf = np.full((len(pts), stride_floats), 7.0, np.float32)
        buf[:, :3], buf[:, 4:7] = pts, nrm
        self.p = self.alloc(buf.nbytes)
        assert self.hip.hipMemcpy(self.p, C.c_void_p(buf.ctypes.data), buf.nbytes, 1) == 0  # hipMemcpyHostToDevice
        self.cloud = abi.Cloud()
        self.cloud.pts, self.cloud.n, self.cloud.stride = self.p.value, len(pts), 4 * stride_floats
        self.extra = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0
        return p

    def device_array(self, nbytes):
        p = self.alloc(nbytes)
        self.extra.append(p)
        return p

    def read(self, p, out):
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), p, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free(self):
        for p in [self.p] + self.extra:
            assert self.hip.hipFree(p) == 0


# ---- the descriptor

@pytest.mark.parametrize("name", FPFH_CASES)
def test_fpfh_fixture_case(ctx_auto, golden, name):
    """clouds of 1, 2 and 3 points and a point without a neighbour (all zeros); copies of points (d2 = 0 skipped in the weighting, f4 = 0 in the pairs); a
    zero normal and a normal along dp (|v| = 0); a neighbour at exactly the radius and one a float ulp beyond; neighbourhoods of 63, 64, 65, 255, 256 and
    257 points, one cell of 257 points and a ball on both sides of a cell face (sizes); f2 = +-1, f1 = +-pi, f3 = +-1, f2 a float ulp either side of an
    inner edge, and f3 and f2 exactly on an inner edge, 11 x == k (bin_edges); a table of 4 096 slots
    at a load of 0.48 (dense_table)"""
    cloud, prm = fpfh_args(golden, name)
    check_fpfh(ctx_auto.fpfh(cloud, prm), golden, name)


def test_fpfh_host_and_device_clouds(ctx_auto, golden):
    g = golden
    for name, stride in (("normals", 7), ("sizes", 12), ("dense_table", 9)):
        (pts, nrm), prm = fpfh_args(g, name)
        dev = DevRecords(pts, nrm, stride)
        check_fpfh(ctx_auto.fpfh(dev.cloud, prm), g, name, name + " from device memory")
        # the outputs in device memory as well
        n = len(pts)
        d_hist, d_k = dev.device_array(132 * n), dev.device_array(4 * n)
        rc = ctx_auto.lib.mulls_fpfh(ctx_auto.h, C.byref(dev.cloud), C.byref(prm), d_hist, d_k)
        assert rc == 0, ctx_auto.lib.mulls_last_error(ctx_auto.h)
        check_fpfh((dev.read(d_hist, np.zeros((n, 33), np.float32)), dev.read(d_k, np.zeros(n, np.uint32))), g, name, name + " to device memory")
        # no n_neighbours
        hist = np.zeros((n, 33), np.float32)
        assert ctx_auto.lib.mulls_fpfh(ctx_auto.h, C.byref(dev.cloud), C.byref(prm), hist.ctypes.data, None) == 0
        assert hist.tobytes() == g[name + "/hist"].tobytes()
        dev.free()


def test_fpfh_refusals_write_nothing(ctx_auto, golden):
    g = golden
    (pts, nrm), prm = fpfh_args(g, "normals")
    n = len(pts)

    def call(p, q, params, stride=None, count=None):
        """-> rc, and whether the outputs were left alone"""
        raw = abi.make_points(p, q)
        c = abi.as_cloud(raw)
        if stride is not None:
            c.stride = stride
        if count is not None:
            c.n = count
        hist, k = np.full((max(len(p), 1), 33), -5.0, np.float32), np.full(max(len(p), 1), 77, np.uint32)
        rc = ctx_auto.lib.mulls_fpfh(ctx_auto.h, C.byref(c), C.byref(params), hist.ctypes.data, k.ctypes.data)
        return rc, bool((hist == -5.0).all() and (k == 77).all())

    assert call(pts, nrm, prm) == (0, False)
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            p, q = pts.copy(), nrm.copy()
            (p, q)[which][n // 2, 1] = bad
            assert call(p, q, prm) == (E_INVALID, True), (bad, which)
            assert "finite" in ctx_auto.lib.mulls_last_error(ctx_auto.h).decode()
    for r in (0.0, -1.0, np.nan, np.inf, 3.0e38):
        assert call(pts, nrm, abi.fpfh_params(r)) == (E_INVALID, True), r
    for stride in (12, 24, 30):
        assert call(pts, nrm, prm, stride=stride) == (E_INVALID, True), stride
    assert call(pts, nrm, prm, count=0) == (E_INVALID, True)
    assert call(pts, nrm, prm, count=(1 << 24) + 1) == (E_UNSUPPORTED, True)
    far = np.concatenate([pts, [[2.0e6, 0.0, 0.0]]]).astype(np.float32)  # 2e6 m at 1 m cells: beyond 2^20 cells
    assert call(far, np.concatenate([nrm, nrm[:1]]), prm) == (E_UNSUPPORTED, True)
    assert "2^20" in ctx_auto.lib.mulls_last_error(ctx_auto.h).decode()
    hist = np.zeros((n, 33), np.float32)
    assert ctx_auto.lib.mulls_fpfh(ctx_auto.h, None, C.byref(prm), hist.ctypes.data, None) == E_INVALID
    c = abi.as_cloud(abi.make_points(pts, nrm))
    assert ctx_auto.lib.mulls_fpfh(ctx_auto.h, C.byref(c), C.byref(prm), None, None) == E_INVALID
    cloud, prm = fpfh_args(g, "normals")
    check_fpfh(ctx_auto.fpfh(cloud, prm), g, "normals", "after the refused calls")


def test_a_cell_at_and_above_its_limit(ctx_auto):
    """MULLS_FPFH_MAX_CELL_POINTS points in one cell run (every point has them all as neighbours; no restatement at this size: the sizes and the sums
    of the sub-histograms are checked); one more is refused with MULLS_E_UNSUPPORTED, by mulls_fpfh and by mulls_coarse_reg_fpfhsac"""
    rng = np.random.default_rng(17)
    n = abi.FPFH_MAX_CELL_POINTS
    d = rng.normal(size=(n + 1, 3))
    pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * (0.3 * rng.uniform(0, 1, (n + 1, 1)) ** (1 / 3)) + 0.5).astype(np.float32)
    d = rng.normal(size=(n + 1, 3))
    nrm = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    hist, k = ctx_auto.fpfh((pts[:n], nrm[:n]), abi.fpfh_params(0.5))
    assert (k == n).all()
    assert (np.abs(hist.astype(np.float64).reshape(n, 3, 11).sum(axis=2) - 100.0) < 1e-3).all()
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.fpfh((pts, nrm), abi.fpfh_params(0.5))
    assert e.value.args[1] == E_UNSUPPORTED and "MULLS_FPFH_MAX_CELL_POINTS" in str(e.value)
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.coarse_reg_fpfhsac((pts, nrm), (pts[:50], nrm[:50]), abi.fpfhsac_params(search_radius=0.5))
    assert e.value.args[1] == E_UNSUPPORTED and "the target" in str(e.value)


# ---- SAC-IA

@pytest.mark.parametrize("name", SAC_CASES)
def test_sac_fixture_case(ctx_auto, golden, name):
    """the default infinite range, where hypothesis 0 wins (sac_default); n_src = 3; n_tgt below k_correspondences; equal target descriptors, the index
    decides; a min_sample_distance that forces the halving rule; 1, 64 and 65 iterations; 1 030, past the 1 024 hypotheses held at a time; hypotheses of equal error, the first wins; e exactly at the
    threshold under both error functions; errors that are NaN, which come after every number; HUBER; the recovery of a known motion on 1 500 / 1 200 points"""
    tgt, src, prm = sac_args(golden, name)
    res = ctx_auto.coarse_reg_fpfhsac(tgt, src, prm)
    check_sac(res, golden, name)
    if name in ("sac_default", "sac_equal_error"):
        assert res.best_iteration == 0


def test_sac_host_and_device_clouds(ctx_auto, golden):
    g = golden
    for name in ("sac_it65", "sac_halving"):
        tgt, src, prm = sac_args(g, name)
        dt, ds = DevRecords(tgt[0], tgt[1], 12), DevRecords(src[0], src[1], 8)
        check_sac(ctx_auto.coarse_reg_fpfhsac(dt.cloud, ds.cloud, prm), g, name, name + " from device memory")
        check_sac(ctx_auto.coarse_reg_fpfhsac(dt.cloud, src, prm), g, name, name + " with a device target and a host source")
        dt.free(), ds.free()


def test_sac_refusals_write_nothing(ctx_auto, golden):
    g = golden
    tgt, src, prm = sac_args(g, "sac_it64")

    def call(t, s, params):
        keep = []
        ct, cs = ctx_auto._normal_cloud(t, keep), ctx_auto._normal_cloud(s, keep)
        res = abi.FpfhSacResult()
        C.memset(C.byref(res), 0x5A, C.sizeof(res))
        rc = ctx_auto.lib.mulls_coarse_reg_fpfhsac(ctx_auto.h, C.byref(ct), C.byref(cs), C.byref(params), C.byref(res))
        return rc, bytes(res) == b"\x5a" * C.sizeof(res)

    P = lambda **kw: sac_args(g, "sac_it64", **kw)[2]
    assert call(tgt, src, prm) == (0, False)
    assert call(tgt, (src[0][:2], src[1][:2]), prm) == (E_INVALID, True)  # n_src < 3
    empty = abi.Cloud()
    empty.pts, empty.n, empty.stride = None, 0, 48
    assert call(empty, src, prm) == (E_INVALID, True)  # n_tgt = 0
    for which in (0, 1):
        for part in (0, 1):
            t, s = [a.copy() for a in tgt], [a.copy() for a in src]
            (t, s)[which][part][5, 2] = np.nan
            assert call(tuple(t), tuple(s), prm) == (E_INVALID, True), (which, part)
    invalid = [dict(search_radius=0.0), dict(search_radius=np.nan), dict(nr_samples=0), dict(k_correspondences=0), dict(k_correspondences=65), dict(max_iterations=0),
               dict(min_sample_distance=-1.0), dict(min_sample_distance=np.inf), dict(min_sample_distance=np.nan), dict(max_correspondence_distance=np.nan),
               dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=-1.0), dict(error_function=2), dict(error_function=-1)]
    for over in invalid:
        assert call(tgt, src, P(**over)) == (E_INVALID, True), over
    for over in (dict(nr_samples=2), dict(nr_samples=4), dict(max_iterations=65537)):
        assert call(tgt, src, P(**over)) == (E_UNSUPPORTED, True), over
    for which in (0, 1):
        t, s = [a.copy() for a in tgt], [a.copy() for a in src]
        (t, s)[which][0][0, 0] = 3.0e6  # beyond 2^20 cells of 0.8 m
        assert call(tuple(t), tuple(s), prm) == (E_UNSUPPORTED, True), which
        assert "2^20" in ctx_auto.lib.mulls_last_error(ctx_auto.h).decode()
    rt, rs = abi.make_points(*tgt), abi.make_points(*src)  # (kept alive: a cloud borrows its array)
    for stride in (12, 24, 30):
        for which in (0, 1):
            ct, cs = abi.as_cloud(rt), abi.as_cloud(rs)
            (ct, cs)[which].stride = stride
            assert call(ct, cs, prm) == (E_INVALID, True), (stride, which)
    ct = abi.as_cloud(rt)
    ct.n = (1 << 24) + 1
    assert call(ct, src, prm) == (E_UNSUPPORTED, True)
    check_sac(ctx_auto.coarse_reg_fpfhsac(tgt, src, prm), g, "sac_it64", "after the refused calls")


# ---- determinism

def test_repeats_and_two_contexts_from_two_threads(ctx_auto, golden):
    g = golden
    names_f, names_s = ["sizes", "duplicates"], ["sac_it65", "sac_threshold_huber"]
    first = {n: ctx_auto.fpfh(*fpfh_args(g, n)) for n in names_f}
    for n in names_f:  # the call repeated on one context
        again = ctx_auto.fpfh(*fpfh_args(g, n))
        assert again[0].tobytes() == first[n][0].tobytes() and again[1].tobytes() == first[n][1].tobytes()
    for n in names_s:
        assert key(ctx_auto.coarse_reg_fpfhsac(*sac_args(g, n))) == key(ctx_auto.coarse_reg_fpfhsac(*sac_args(g, n)))
    out, errors = {}, []

    def work(tid):
        try:
            c = lib.Context(0)
            try:
                for rep in range(2):
                    for n in names_f[tid::2] + names_f[1 - tid::2]:
                        h, k = c.fpfh(*fpfh_args(g, n))
                        out[(tid, rep, n)] = (h.tobytes(), k.tobytes())
                    for n in names_s[tid::2] + names_s[1 - tid::2]:
                        out[(tid, rep, n)] = key(c.coarse_reg_fpfhsac(*sac_args(g, n)))
            finally:
                c.close()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for (tid, rep, n), k in out.items():
        assert k == out[(0, 0, n)], (tid, rep, n)
    for n in names_f:
        assert out[(0, 0, n)] == (g[n + "/hist"].tobytes(), g[n + "/k"].tobytes())


# ---- the bridge

def test_bridge_returns_the_c_calls_bits(ctx_auto, golden, tmp_path):
    """lo::hip::compute_fpfh_feature and lo::hip::coarse_reg_fpfhsac (include/cregistration_fpfh_hip.hpp) in a stand-alone program built against the
    stand-in PCL and Eigen types of oracle/ref_shim: the descriptors, the pose and the fitness of the C calls, and traned_source moved by that pose"""
    g, name = golden, "sac_it64"
    tgt, src, prm = sac_args(g, name)
    exe = str(tmp_path / "fpfh_bridge_harness")
    so = os.path.join(ROOT, "mulls_amd", "libmulls_hip.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "fpfh_bridge_harness.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    rt, rs = abi.make_points(*tgt), abi.make_points(*src)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(rt), len(rs)], np.uint32).tobytes() + rt.tobytes() + rs.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), repr(float(prm.search_radius)), str(prm.max_iterations), str(prm.k_correspondences),
                           repr(float(prm.max_correspondence_distance)), str(prm.seed)])
    raw = open(tmp_path / "out.bin", "rb").read()
    n = len(rs)
    hist = np.frombuffer(raw, np.float32, 33 * n).reshape(n, 33)
    T = np.frombuffer(raw, np.float64, 16, 132 * n).reshape(4, 4).T
    fitness = np.frombuffer(raw, np.float64, 1, 132 * n + 128)[0]
    moved = np.frombuffer(raw, abi.POINT_DTYPE, n, 132 * n + 136)
    want_hist, _ = ctx_auto.fpfh(src, abi.fpfh_params(prm.search_radius))
    res = ctx_auto.coarse_reg_fpfhsac(tgt, src, prm)
    assert hist.tobytes() == want_hist.tobytes()
    assert T.tobytes() == pose(res).tobytes() == g[name + "/T"].tobytes() and fitness == res.fitness == g[name + "/floats"][1]
    x = src[0].astype(np.float64)
    for a, field in enumerate("xyz"):
        assert (moved[field] == (((T[a, 0] * x[:, 0] + T[a, 1] * x[:, 1]) + T[a, 2] * x[:, 2]) + T[a, 3]).astype(np.float32)).all(), field
    assert (moved["nx"] == rs["nx"]).all() and (moved["nz"] == rs["nz"]).all()
