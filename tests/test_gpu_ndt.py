"""GPU tests of mulls_ndt / mulls_ndt_batch through mulls_amd/lib.py against the numpy restatement of the library's definition (tests/ndt_restated.py),
read from tests/golden/ndt_cases.npz (tests/test_ndt.py keeps the fixture equal to the restatement and asserts which case takes which path).

Every comparison with the restatement and between launch forms is equality of bits of T, fitness, trans_probability and the integer fields: the
definition has no operation whose host and device results may differ (+ - * / sqrt in double or float in a stated order, sin / cos / exp from
detmath.h, no contraction).

Neither ndt_omp nor PCL is available where these tests run: nothing here was compared with them."""
import ctypes as C
import json
import threading

import numpy as np
import pytest

from mulls_amd import abi, lib
from test_ndt import GOLDEN

pytestmark = pytest.mark.gpu

INT_FIELDS = ("code", "iterations", "evaluations", "converged", "n_leaves", "n_leaves_used", "n_src", "n_tgt", "line_search_reversals", "inner_steps")
FLOAT_FIELDS = ("fitness", "trans_probability", "gauss_d1", "gauss_d2", "gauss_d3")
E_INVALID, E_UNSUPPORTED = -100, -103


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}, json.loads(str(z["names"]))


def problem(g, name, **over):
    p = dict(tgt=g[name + "/tgt"], src=g[name + "/src"], tgt_bound=g[name + "/tgt_bound"], src_bound=g[name + "/src_bound"], init_guess=g[name + "/guess"])
    p.update(over)
    return p


def params(g, name, **over):
    prm = json.loads(str(g[name + "/prm"]))
    prm.update(over)
    return abi.ndt_params(**prm)


def key(res):
    """everything a result holds, as bytes"""
    return (tuple(getattr(res, k) for k in INT_FIELDS), np.array([getattr(res, k) for k in FLOAT_FIELDS]).tobytes(), np.array(res.T).tobytes())


def pose(res):
    return np.array(res.T).reshape(4, 4).T


def check(res, g, name, what=None):
    what = what or name
    for k, v in zip(INT_FIELDS, g[name + "/ints"]):
        assert getattr(res, k) == v, (what, k, getattr(res, k), v)
    got = np.array([getattr(res, k) for k in FLOAT_FIELDS])
    assert got.tobytes() == g[name + "/floats"].tobytes(), (what, got, g[name + "/floats"])
    assert pose(res).tobytes() == g[name + "/T"].tobytes(), (what, np.abs(pose(res) - g[name + "/T"]).max())


def run(ctx, g, name):
    return ctx.ndt(**problem(g, name), params=params(g, name))


ALL = ["street", "street_inner", "street_max_iter", "street_direct1", "street_direct26", "street_2m", "street_no_crop", "street_guess", "street_near_identity",
       "street_large", "street_tight", "crafted", "crafted_26", "no_leaves"]


@pytest.mark.parametrize("name", ALL)
def test_fixture_case(ctx_auto, golden, name):
    """the paths: no inner loop / inner loop and the extra Hessian pass (street_inner), reversed directions, max_iterations (street_max_iter), the epsilon
    test at the second iteration (street_2m), the zero-step return (no_leaves), leaves of 5 and 6 points, planar, linear and identical leaves and source
    points beyond the grid on every side (crafted), the guess and the near-identity guess, the crop off, DIRECT1 / 7 / 26, leaves of 1 and 2 m"""
    g, names = golden
    assert names == ALL
    res = run(ctx_auto, g, name)
    check(res, g, name)
    if name == "no_leaves":
        assert res.n_leaves_used == 0 and res.converged == 1 and pose(res).tobytes() == g[name + "/guess"].tobytes()
    if name == "street_inner":
        assert res.evaluations > res.iterations + 1


def test_input_validation(ctx_auto, golden):
    g, _ = golden
    P = problem(g, "street")
    empty = np.zeros((0, 3), np.float32)
    for over in (dict(src=empty), dict(tgt=empty)):
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.ndt(**dict(P, **over))
        assert e.value.args[1] == E_INVALID and "empty" in str(e.value)
    for which, bad in (("src", np.nan), ("tgt", np.inf), ("src", -np.inf)):
        c = P[which].copy()
        c[len(c) // 2, 1] = bad
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.ndt(**dict(P, **{which: c}))
        assert e.value.args[1] == E_INVALID and "finite" in str(e.value)
    guess = np.eye(4)
    guess[0, 3] = np.nan
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.ndt(**dict(P, init_guess=guess))
    assert e.value.args[1] == E_INVALID
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.ndt(**P, params=abi.ndt_params(search_method=abi.NDT_KDTREE))
    assert e.value.args[1] == E_UNSUPPORTED
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.ndt(**P, params=abi.ndt_params(resolution=0.0))
    assert e.value.args[1] == E_INVALID
    # a grid of more than INT32_MAX cells: two far corners at 0.05 m leaves
    far = np.concatenate([P["tgt"], [[4000.0, 4000.0, 300.0]]]).astype(np.float32)
    wide = np.array([-1e4, -1e4, -1e4, 1e4, 1e4, 1e4])
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.ndt(far, P["src"], wide, wide, None, abi.ndt_params(resolution=0.05))
    assert e.value.args[1] == E_UNSUPPORTED
    check(run(ctx_auto, g, "street"), g, "street", "after the refused calls")


def test_crop_to_nothing(ctx_auto, golden):
    """[LIB] a cloud that is empty after the crop: no registration, T = the guess, fitness DBL_MAX, code -3"""
    g, _ = golden
    P = problem(g, "street_guess")
    away = P["tgt_bound"] + 1000.0
    res = ctx_auto.ndt(**dict(P, tgt_bound=away))
    assert res.n_src == 0 and res.n_tgt == 0 and res.code == -3 and res.converged == 0 and res.iterations == 0 and res.fitness == 1.7976931348623157e308
    assert pose(res).tobytes() == P["init_guess"].tobytes()


class DevCloud:
    """the coordinates in a device allocation of the caller's own (straight from the HIP runtime the library runs on), at a stride of its own"""

    def __init__(self, pts, stride_floats):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        buf = np.zeros((len(pts), stride_floats), np.float32)
        buf[:, :3] = pts
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), buf.nbytes) == 0
        assert self.hip.hipMemcpy(self.p, C.c_void_p(buf.ctypes.data), buf.nbytes, 1) == 0  # hipMemcpyHostToDevice
        self.cloud = abi.Cloud()
        self.cloud.pts, self.cloud.n, self.cloud.stride = self.p.value, len(pts), 4 * stride_floats

    def free(self):
        assert self.hip.hipFree(self.p) == 0


def test_host_and_device_clouds(ctx_auto, golden):
    g, _ = golden
    for name in ("street_guess", "crafted"):
        P = problem(g, name)
        want = key(run(ctx_auto, g, name))
        dt, ds = DevCloud(P["tgt"], 3), DevCloud(P["src"], 5)
        assert key(ctx_auto.ndt(**dict(P, tgt=dt.cloud, src=ds.cloud), params=params(g, name))) == want, name
        # host records of 48 bytes
        rec_t, rec_s = np.zeros(len(P["tgt"]), abi.POINT_DTYPE), np.zeros(len(P["src"]), abi.POINT_DTYPE)
        for rec, pts in ((rec_t, P["tgt"]), (rec_s, P["src"])):
            rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
        assert key(ctx_auto.ndt(**dict(P, tgt=rec_t, src=rec_s), params=params(g, name))) == want, name
        # mixed: a device target with a host source
        assert key(ctx_auto.ndt(**dict(P, tgt=dt.cloud), params=params(g, name))) == want, name
        dt.free(), ds.free()


BATCH = ["street", "no_leaves", "street_large", "crafted", "street_guess", "no_leaves", "street_near_identity", "street_tight"]


def test_batch_equals_single_calls(ctx_auto, golden):
    """mixed sizes under one parameter set; no_leaves ends at its first tick among problems that run for several"""
    g, _ = golden
    for over in (dict(), dict(transformation_epsilon=0.2), dict(search_method=abi.NDT_DIRECT26, resolution=2.0)):
        prm = abi.ndt_params(apply_intersection_filter=0, **over)
        probs = [problem(g, n) for n in BATCH]
        single = [key(ctx_auto.ndt(**p, params=prm)) for p in probs]
        ticks = [k[0][2] for k in single]
        assert min(ticks) == 1 and max(ticks) >= 4
        got = [key(r) for r in ctx_auto.ndt_batch(probs, prm)]
        assert got == single, over
        # cut into sub-batches by a small scratch limit: 1 MiB holds none of these problems (each then runs alone), 4 MiB two or three
        for limit in (1 << 20, 4 << 20):
            cut = abi.ndt_params(apply_intersection_filter=0, scratch_limit_bytes=limit, **over)
            assert [key(r) for r in ctx_auto.ndt_batch(probs, cut)] == single, (over, limit)
    assert ctx_auto.ndt_batch([], abi.ndt_params()) == []


def test_batch_with_defaults_equals_the_fixture(ctx_auto, golden):
    g, _ = golden
    names = ["street", "street_guess", "street_near_identity", "street_tight"]  # the cases that run under the default parameters
    for res, n in zip(ctx_auto.ndt_batch([problem(g, n) for n in names]), names):
        check(res, g, n, n + " in a batch")


def test_bad_problem_in_a_batch_is_refused(ctx_auto, golden):
    g, _ = golden
    P = problem(g, "street")
    bad = dict(P, src=np.zeros((0, 3), np.float32))
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.ndt_batch([P, bad, P])
    assert e.value.args[1] == E_INVALID and "problem 1" in str(e.value)
    nf = P["src"].copy()
    nf[3, 2] = np.nan
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.ndt_batch([P, P, dict(P, src=nf)])
    assert e.value.args[1] == E_INVALID and "problem 2" in str(e.value)


def test_two_contexts_from_two_threads(golden):
    g, _ = golden
    names = ["street_inner", "crafted", "street_large", "street_guess"]
    out, errors = {}, []

    def work(tid):
        try:
            c = lib.Context(0)
            try:
                for rep in range(3):
                    for n in names[tid::2] + names[1 - tid::2]:
                        out[(tid, rep, n)] = key(run(c, g, n))
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
    c = lib.Context(0)
    try:
        for n in names:
            res = run(c, g, n)
            check(res, g, n)
            assert key(res) == out[(0, 0, n)]
    finally:
        c.close()
