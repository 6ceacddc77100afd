"""GPU tests of mulls_compute_fpfh_batch and mulls_coarse_reg_fpfhsac_batch through mulls_amd/lib.py.  The expectations are the numpy restatement's
(tests/fpfh_restated.py), read from tests/golden/fpfh_cases.npz (the descriptors) and tests/golden/fpfh_batch_cases.npz (the SAC-IA scenes, one
restatement call per problem; tests/test_fpfh_batch.py keeps that file equal to the restatement and asserts which scene reaches which edge), and the
single calls on the same context.  Every comparison is equality of bits: a batch redefines no arithmetic, no order of summation, no tie rule and no draw.

PCL, FLANN and Eigen are not available where these tests run: nothing here was compared with them."""
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import fpfh_batch_plan as plan
from fpfh_names import FLOAT_FIELDS, FPFH_CASES, GOLDEN, INT_FIELDS, ROOT
from mulls_amd import abi, lib
from test_gpu_fpfh import DevRecords, check_fpfh

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -100, -103
RADIUS = 0.5  # the search radius every descriptor case of the fixture has


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def batch_golden():
    z = np.load(plan.BATCH_GOLDEN)
    return {k: z[k] for k in z.files}


def key(res):
    """everything a result holds, as bytes"""
    return (tuple(getattr(res, k) for k in INT_FIELDS), np.array([getattr(res, k) for k in FLOAT_FIELDS]).tobytes(), np.array(res.T).tobytes())


def pose(res):
    return np.array(res.T).reshape(4, 4).T


def scene(g, bg, name, **over):
    """-> params, [(tgt, src), ...]: a cloud that several problems name is one Python object, so one mulls_cloud"""
    prm = json.loads(str(bg[name + "/prm"]))
    prm.update(over)
    seen = {}

    def cloud(ref):
        ref = tuple(ref)
        if ref not in seen:
            seen[ref] = (g["%s/%s" % ref], g["%s/%s_nrm" % ref])
        return seen[ref]

    return abi.fpfhsac_params(**prm), [(cloud(t), cloud(s)) for t, s in json.loads(str(bg[name + "/problems"]))]


def sizes_of(problems):
    return [(len(s[0]), len(t[0])) for t, s in problems]


def check_scene(results, bg, name, what=""):
    assert len(results) == len(bg[name + "/ints"])
    for b, res in enumerate(results):
        where = (name, b, what)
        for k, v in zip(INT_FIELDS, bg[name + "/ints"][b]):
            assert getattr(res, k) == v, (where, k, getattr(res, k), v)
        got = np.array([getattr(res, k) for k in FLOAT_FIELDS])
        assert got.tobytes() == bg[name + "/floats"][b].tobytes(), (where, got, bg[name + "/floats"][b])
        assert pose(res).tobytes() == bg[name + "/T"][b].tobytes(), (where, np.abs(pose(res) - bg[name + "/T"][b]).max())


# ---- the descriptors

def fpfh_clouds(g, names):
    return [(g[n + "/pts"], g[n + "/nrm"]) for n in names]


def test_fpfh_batch_all_cases_in_one_call(ctx_auto, golden):
    """all nine descriptor scenes, 1 to 2 000 points, in one call; the same with a cloud named twice; every cloud alone (scratch_limit_bytes = 1)"""
    g, prm = golden, abi.fpfh_params(RADIUS)
    assert all(float(g[n + "/search_radius"]) == RADIUS for n in FPFH_CASES)
    clouds = fpfh_clouds(g, FPFH_CASES)
    for limit in (0, 1):
        for name, got in zip(FPFH_CASES, ctx_auto.fpfh_batch(clouds, prm, limit)):
            check_fpfh(got, g, name, "%s in a batch, limit %d" % (name, limit))
    twice = list(FPFH_CASES) + ["sizes"]
    for limit in (0, 1, plan.cloud_bytes(len(g["sizes/pts"])) * 2):
        got = ctx_auto.fpfh_batch(clouds + [clouds[FPFH_CASES.index("sizes")]], prm, limit)
        for name, one in zip(twice, got):
            check_fpfh(one, g, name, "%s with sizes named twice, limit %d" % (name, limit))
    assert ctx_auto.fpfh_batch([], prm) == []
    single = ctx_auto.fpfh(clouds[3], prm)
    assert single[0].tobytes() == got[3][0].tobytes() and single[1].tobytes() == got[3][1].tobytes()


def test_fpfh_batch_device_clouds_and_outputs(ctx_auto, golden):
    g, prm = golden, abi.fpfh_params(RADIUS)
    names = ("normals", "dense_table", "sizes")
    devs = [DevRecords(g[n + "/pts"], g[n + "/nrm"], stride) for n, stride in zip(names, (7, 9, 12))]
    try:
        for name, got in zip(names, ctx_auto.fpfh_batch([d.cloud for d in devs], prm)):
            check_fpfh(got, g, name, name + " from device memory")
        arr = (abi.Cloud * 3)(*[d.cloud for d in devs])
        ns = [len(g[n + "/pts"]) for n in names]
        d_hist, d_k = [d.device_array(132 * n) for d, n in zip(devs, ns)], [d.device_array(4 * n) for d, n in zip(devs, ns)]
        hp, kp = (C.c_void_p * 3)(*[p.value for p in d_hist]), (C.c_void_p * 3)(*[p.value for p in d_k])
        assert ctx_auto.lib.mulls_compute_fpfh_batch(ctx_auto.h, arr, 3, C.byref(prm), hp, kp, 0) == 0, ctx_auto.lib.mulls_last_error(ctx_auto.h)
        for name, d, ph, pk, n in zip(names, devs, d_hist, d_k, ns):
            check_fpfh((d.read(ph, np.zeros((n, 33), np.float32)), d.read(pk, np.zeros(n, np.uint32))), g, name, name + " to device memory")
        # n_neighbours NULL as a whole, then NULL for one cloud; host outputs from device clouds
        hist = [np.zeros((n, 33), np.float32) for n in ns]
        hp = (C.c_void_p * 3)(*[h.ctypes.data for h in hist])
        assert ctx_auto.lib.mulls_compute_fpfh_batch(ctx_auto.h, arr, 3, C.byref(prm), hp, None, 0) == 0
        for name, h in zip(names, hist):
            assert h.tobytes() == g[name + "/hist"].tobytes(), name
        hist, ks = [np.zeros((n, 33), np.float32) for n in ns], [np.full(n, 77, np.uint32) for n in ns]
        hp, kp = (C.c_void_p * 3)(*[h.ctypes.data for h in hist]), (C.c_void_p * 3)(ks[0].ctypes.data, None, ks[2].ctypes.data)
        assert ctx_auto.lib.mulls_compute_fpfh_batch(ctx_auto.h, arr, 3, C.byref(prm), hp, kp, 1) == 0
        for i, name in enumerate(names):
            assert hist[i].tobytes() == g[name + "/hist"].tobytes(), name
            assert (ks[i] == 77).all() if i == 1 else ks[i].tobytes() == g[name + "/k"].tobytes(), name
    finally:
        for d in devs:
            d.free()


def test_fpfh_batch_refusals_write_nothing(ctx_auto, golden):
    g, prm = golden, abi.fpfh_params(RADIUS)
    names = ["two", "normals", "duplicates", "radius_edge", "three"]
    good = fpfh_clouds(g, names)
    last_error = lambda: ctx_auto.lib.mulls_last_error(ctx_auto.h).decode()

    def call(clouds, params=prm, limit=0, stride=None, null_hist=None, no_hist=False):
        """-> rc, and whether every output was left alone"""
        raws = [abi.make_points(p, q) for p, q in clouds]
        arr = (abi.Cloud * len(raws))(*[abi.as_cloud(r) for r in raws])
        if stride is not None:
            arr[stride[0]].stride = stride[1]
        hist, ks = [np.full((len(r), 33), -5.0, np.float32) for r in raws], [np.full(len(r), 77, np.uint32) for r in raws]
        hp = (C.c_void_p * len(raws))(*[None if i == null_hist else h.ctypes.data for i, h in enumerate(hist)])
        kp = (C.c_void_p * len(raws))(*[k.ctypes.data for k in ks])
        rc = ctx_auto.lib.mulls_compute_fpfh_batch(ctx_auto.h, arr, len(raws), C.byref(params), None if no_hist else hp, kp, limit)
        return rc, all((h == -5.0).all() for h in hist) and all((k == 77).all() for k in ks)

    assert call(good) == (0, False)
    assert call(good, stride=(2, 24)) == (E_INVALID, True) and "cloud 2" in last_error()
    assert call(good, null_hist=1) == (E_INVALID, True) and "cloud 1" in last_error()
    assert call(good, no_hist=True) == (E_INVALID, True)
    assert call(good, abi.fpfh_params(0.0)) == (E_INVALID, True)
    for limit in (0, 1):  # in one sub-batch; every cloud alone, so that the clouds before the refused one already ran
        bad = [(p.copy(), q.copy()) for p, q in good]
        bad[3][1][2, 1] = np.nan  # found on the device, clouds 0 .. 2 good
        assert call(bad, limit=limit) == (E_INVALID, True), limit
        assert "cloud 3" in last_error() and "finite" in last_error()
        bad = [(p.copy(), q.copy()) for p, q in good]
        bad[4][0][1, 0] = 2.0e6  # beyond 2^20 cells of 1 m, in the last cloud
        assert call(bad, limit=limit) == (E_UNSUPPORTED, True), limit
        assert "cloud 4" in last_error() and "2^20" in last_error()
    for name, got in zip(names, ctx_auto.fpfh_batch(good, prm)):
        check_fpfh(got, g, name, name + " after the refused calls")


# ---- SAC-IA

@pytest.mark.parametrize("name", plan.SCENES)
def test_sac_scene(ctx_auto, golden, batch_golden, name):
    """mixed: five sizes under 65 hypotheses, k_eff = 7 beside 15, no winner is hypothesis 0; chunks: 3 090 flat hypotheses, the stretches of 1 024 begin
    and end inside problems; shared: one target against four sources and as a source itself; default: the infinite range, hypothesis 0; nan: NaN errors
    come last; huber.  Against the restatement, and against the single calls on the same context byte for byte."""
    prm, problems = scene(golden, batch_golden, name)
    got = ctx_auto.coarse_reg_fpfhsac_batch(problems, prm)
    check_scene(got, batch_golden, name)
    for b, (tgt, src) in enumerate(problems):
        assert key(got[b]) == key(ctx_auto.coarse_reg_fpfhsac(tgt, src, prm)), (name, b)
    if name == "shared":
        assert key(got[0]) == key(got[3])
    if name == "default":
        assert [r.best_iteration for r in got] == [0, 0, 0]


@pytest.mark.parametrize("name", ["mixed", "chunks"])
def test_sac_sub_batches_and_stretches_give_the_same_bytes(ctx_auto, golden, batch_golden, name):
    """every problem alone with the distance pool at its minimum (scratch_limit_bytes = 1); a limit from the header's byte counts that cuts five problems
    2 + 2 + 1 (three: 2 + 1); for chunks a limit that leaves a pool of a hundred hypotheses of the 60-point source, so that the stretch boundaries fall
    every hundred slots inside that problem and in front of all three winners"""
    prm, problems = scene(golden, batch_golden, name)
    sizes, iters = sizes_of(problems), prm.max_iterations
    want = [key(r) for r in ctx_auto.coarse_reg_fpfhsac_batch(problems, prm)]
    limits = {"alone": 1}
    pairs = [plan.counted(sizes[k:k + 2], iters) for k in range(0, len(sizes) - 1, 2)]
    limits["pairs"] = max(pairs)
    assert plan.cuts(sizes, iters, limits["pairs"]) == ([0, 2, 4, 5] if name == "mixed" else [0, 2, 3])
    if name == "chunks":
        counted = plan.counted(sizes, iters)
        limits["pool"] = counted - sum(plan.up256(4 * s) for s, _ in sizes) + 100 * 4 * 60
        assert plan.cuts(sizes, iters, limits["pool"]) == [0, 3] and plan.pool_bytes([s for s, _ in sizes], iters, counted, limits["pool"]) == 24000
    for what, limit in limits.items():
        got = ctx_auto.coarse_reg_fpfhsac_batch(problems, prm, limit)
        check_scene(got, batch_golden, name, what)
        assert [key(r) for r in got] == want, what


def test_sac_batch_of_one_is_the_single_call(ctx_auto, golden):
    g, name = golden, "sac_recovery"
    prm = abi.fpfhsac_params(**json.loads(str(g[name + "/prm"])))
    tgt, src = (g[name + "/tgt"], g[name + "/tgt_nrm"]), (g[name + "/src"], g[name + "/src_nrm"])
    assert (len(tgt[0]), len(src[0]), prm.max_iterations) == (1500, 1200, 120)
    (got,) = ctx_auto.coarse_reg_fpfhsac_batch([(tgt, src)], prm)
    assert key(got) == key(ctx_auto.coarse_reg_fpfhsac(tgt, src, prm)) and got.best_iteration == 1
    assert tuple(getattr(got, k) for k in INT_FIELDS) == tuple(g[name + "/ints"]) and pose(got).tobytes() == g[name + "/T"].tobytes()
    assert np.array([got.best_error, got.fitness]).tobytes() == g[name + "/floats"].tobytes()
    assert ctx_auto.coarse_reg_fpfhsac_batch([], prm) == []


def test_sac_shared_clouds_in_host_and_device_memory(ctx_auto, golden, batch_golden):
    prm, problems = scene(golden, batch_golden, "shared")
    check_scene(ctx_auto.coarse_reg_fpfhsac_batch(problems, prm), batch_golden, "shared", "host clouds")
    devs = {}

    def dev(cloud, stride):
        if id(cloud) not in devs:
            devs[id(cloud)] = DevRecords(cloud[0], cloud[1], stride)
        return devs[id(cloud)].cloud

    try:
        target = problems[0][0]
        mixed = [(dev(t, 12) if t is target else t, dev(s, 12) if s is target else s) for t, s in problems]
        check_scene(ctx_auto.coarse_reg_fpfhsac_batch(mixed, prm), batch_golden, "shared", "the shared target on the device, the sources on the host")
        for limit in (0, 1):
            on_device = [(dev(t, 12), dev(s, 9 if s is not target else 12)) for t, s in problems]
            check_scene(ctx_auto.coarse_reg_fpfhsac_batch(on_device, prm, limit), batch_golden, "shared", "device clouds, limit %d" % limit)
    finally:
        for d in devs.values():
            d.free()


def test_sac_refusals_write_nothing(ctx_auto, golden, batch_golden):
    g, bg = golden, batch_golden
    prm, problems = scene(g, bg, "mixed")
    B = len(problems)
    last_error = lambda: ctx_auto.lib.mulls_last_error(ctx_auto.h).decode()

    def call(probs, params=prm, limit=0, stride=None, no_results=False, no_params=False):
        """-> rc, and whether every result byte was left alone"""
        keep = []
        arr = (abi.FpfhSacProblem * len(probs))()
        for b, (t, s) in enumerate(probs):
            arr[b].tgt, arr[b].src = ctx_auto._normal_cloud(t, keep), ctx_auto._normal_cloud(s, keep)
        if stride is not None:
            arr[stride[0]].src.stride = stride[1]
        res = (abi.FpfhSacResult * len(probs))()
        C.memset(res, 0x5A, C.sizeof(res))
        rc = ctx_auto.lib.mulls_coarse_reg_fpfhsac_batch(ctx_auto.h, arr, len(probs), None if no_params else C.byref(params), limit, None if no_results else res)
        return rc, bytes(res) == b"\x5a" * C.sizeof(res)

    def with_source(b, change):
        probs = list(problems)
        src = [a.copy() for a in problems[b][1]]
        src = change(src) or src
        probs[b] = (problems[b][0], tuple(src))
        return probs

    assert call(problems) == (0, False)
    assert call(problems, stride=(2, 24)) == (E_INVALID, True) and "problem 2: the source" in last_error()
    assert call(with_source(1, lambda s: [s[0][:2], s[1][:2]])) == (E_INVALID, True) and "problem 1: the source has fewer than 3" in last_error()
    assert call(problems, no_results=True) == (E_INVALID, True)
    assert call(problems, no_params=True) == (E_INVALID, True)
    for over, code in ((dict(k_correspondences=65), E_INVALID), (dict(max_iterations=0), E_INVALID), (dict(nr_samples=4), E_UNSUPPORTED)):
        assert call(problems, scene(g, bg, "mixed", **over)[0]) == (code, True), over
        assert "problem 0" in last_error()

    def nan_normal(s):
        s[1][5, 2] = np.nan

    def far_coordinate(s):
        s[0][0, 0] = 3.0e6  # beyond 2^20 cells of 0.8 m

    for limit in (0, 1):  # (under limit 1 the sub-batches before the refused one already ran)
        assert call(with_source(3, nan_normal), limit=limit) == (E_INVALID, True), limit  # found on the device, problems 0 .. 2 good
        assert "problem 3: the source" in last_error() and "finite" in last_error()
        assert call(with_source(B - 1, far_coordinate), limit=limit) == (E_UNSUPPORTED, True), limit
        assert "problem %d: the source" % (B - 1) in last_error() and "2^20" in last_error()
    # a refused cloud that several problems share names the first of them, as its target
    shared_prm, shared = scene(g, bg, "shared")
    bad = (shared[0][0][0].copy(), shared[0][0][1].copy())
    bad[0][7, 1] = np.inf
    probs = [shared[1]] + [(bad if t is shared[0][0] else t, bad if s is shared[0][0] else s) for t, s in shared[2:]]
    assert call(probs, shared_prm) == (E_INVALID, True) and "problem 1: the target" in last_error()
    check_scene(ctx_auto.coarse_reg_fpfhsac_batch(problems, prm), bg, "mixed", "after the refused calls")


# ---- determinism

def test_repeats_and_two_contexts_from_two_threads(ctx_auto, golden, batch_golden):
    g, bg = golden, batch_golden
    names = ["mixed", "shared"]
    clouds = fpfh_clouds(g, ["sizes", "duplicates", "sizes"])
    first = {n: [key(r) for r in ctx_auto.coarse_reg_fpfhsac_batch(*reversed(scene(g, bg, n)))] for n in names}
    for n in names:  # the call repeated on one context
        assert [key(r) for r in ctx_auto.coarse_reg_fpfhsac_batch(*reversed(scene(g, bg, n)))] == first[n]
    first_f = [(h.tobytes(), k.tobytes()) for h, k in ctx_auto.fpfh_batch(clouds, abi.fpfh_params(RADIUS))]
    out, errors = {}, []

    def work(tid):
        try:
            c = lib.Context(0)
            try:
                for rep in range(2):
                    for n in names[tid::2] + names[1 - tid::2]:
                        out[(tid, rep, n)] = [key(r) for r in c.coarse_reg_fpfhsac_batch(*reversed(scene(g, bg, n)))]
                    out[(tid, rep, "fpfh")] = [(h.tobytes(), k.tobytes()) for h, k in c.fpfh_batch(clouds, abi.fpfh_params(RADIUS))]
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
        assert k == (first_f if n == "fpfh" else first[n]), (tid, rep, n)


# ---- the bridge

def test_bridge_returns_the_c_calls_bits(ctx_auto, golden, batch_golden, tmp_path):
    """lo::hip::compute_fpfh_feature_batch and lo::hip::coarse_reg_fpfhsac_batch (include/cregistration_fpfh_hip.hpp) in a stand-alone program built against
    the stand-in PCL and Eigen types of oracle/ref_shim, on the shared scene with the shared cloud as one pointer: the descriptors, the poses and the
    fitness scores of the C calls, and every moved source under its pose"""
    g, bg, name = golden, batch_golden, "shared"
    prm, problems = scene(g, bg, name)
    exe = str(tmp_path / "fpfh_batch_bridge_harness")
    so = os.path.join(ROOT, "mulls_amd", "libmulls_hip.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "fpfh_batch_bridge_harness.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    distinct, index = [], {}
    for pair in problems:
        for cloud in pair:
            if id(cloud) not in index:
                index[id(cloud)] = len(distinct)
                distinct.append(cloud)
    raws = [abi.make_points(*c) for c in distinct]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint32(len(raws)).tobytes())
        for r in raws:
            f.write(np.uint32(len(r)).tobytes() + r.tobytes())
        f.write(np.uint32(len(problems)).tobytes())
        for t, s in problems:
            f.write(np.array([index[id(t)], index[id(s)]], np.uint32).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), repr(float(prm.search_radius)), str(prm.max_iterations), str(prm.k_correspondences),
                           repr(float(prm.max_correspondence_distance)), str(prm.seed)])
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0
    want_hist = ctx_auto.fpfh_batch(distinct, abi.fpfh_params(prm.search_radius))
    for c, r in enumerate(raws):
        hist = np.frombuffer(raw, np.float32, 33 * len(r), at)
        at += 132 * len(r)
        assert hist.tobytes() == want_hist[c][0].tobytes() == ctx_auto.fpfh(distinct[c], abi.fpfh_params(prm.search_radius))[0].tobytes(), c
    want = ctx_auto.coarse_reg_fpfhsac_batch(problems, prm)
    for b, (t, s) in enumerate(problems):
        n = len(s[0])
        T = np.frombuffer(raw, np.float64, 16, at).reshape(4, 4).T
        fitness = np.frombuffer(raw, np.float64, 1, at + 128)[0]
        moved = np.frombuffer(raw, abi.POINT_DTYPE, n, at + 136)
        at += 136 + 48 * n
        assert T.tobytes() == pose(want[b]).tobytes() == bg[name + "/T"][b].tobytes() and fitness == want[b].fitness == bg[name + "/floats"][b][1], b
        x, rs = s[0].astype(np.float64), raws[index[id(s)]]
        for a, field in enumerate("xyz"):
            assert (moved[field] == (((T[a, 0] * x[:, 0] + T[a, 1] * x[:, 1]) + T[a, 2] * x[:, 2]) + T[a, 3]).astype(np.float32)).all(), (b, field)
        assert (moved["nx"] == rs["nx"]).all() and (moved["nz"] == rs["nz"]).all()
    assert at == len(raw)
