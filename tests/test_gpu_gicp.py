"""GPU tests of mulls_gicp / mulls_gicp_batch through mulls_amd/lib.py against the numpy restatement of the library's definition
(tests/gicp_restated.py), read from tests/golden/gicp_cases.npz (tests/test_gicp.py keeps the fixture equal to the restatement and asserts which case
takes which path).

Every comparison with the restatement and between launch forms is equality of bits of T, fitness, loss and the integer fields: the definition has no
operation whose host and device results may differ (+ - * / sqrt in double or float in a stated order, sin / atan2 from detmath.h, no contraction).

Neither fast_gicp, Sophus, Eigen nor PCL is available where these tests run: nothing here was compared with them."""
import json
import threading

import numpy as np
import pytest

from mulls_amd import abi, lib
from test_gicp import GOLDEN
from test_gpu_ndt import DevCloud

pytestmark = pytest.mark.gpu

INT_FIELDS = ("code", "iterations", "converged", "stop", "n_src", "n_tgt", "n_voxels", "n_corr")
FLOAT_FIELDS = ("fitness", "loss")
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
    return abi.gicp_params(**prm)


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
    return ctx.gicp(**problem(g, name), params=params(g, name))


ALL = ["street", "street_guess", "street_near_identity", "street_crop", "street_2m", "street_half", "street_k5", "street_k32", "street_max_iter",
       "street_tight", "street_large", "crafted", "exact_k", "k_plus_1", "too_few", "no_overlap", "outliers"]


@pytest.mark.parametrize("name", ALL)
def test_fixture_case(ctx_auto, golden, name):
    """the paths: the guess and the near-identity guess, the crop, voxels of 0.5, 1 and 2 m, k = 5, 20 and 32 (the three capacities of the register
    list), max_iterations reached (street_max_iter; crafted, all 64 ticks), ties in (d2, index), identical points, equal eigenvalues, points on voxel
    faces and colliding keys (crafted), a source of exactly k and of k + 1 points, too few points after the crop, no point in any voxel, neighbours
    past the ring walk (outliers)"""
    g, names = golden
    assert names == ALL
    res = run(ctx_auto, g, name)
    check(res, g, name)
    if name == "too_few":
        assert res.n_src == 19 and res.code == -3 and res.stop == abi.GICP_STOP_NONE and pose(res).tobytes() == g[name + "/guess"].tobytes()
    if name == "no_overlap":
        assert res.n_corr == 0 and res.stop == abi.GICP_STOP_SINGULAR and res.iterations == 0 and pose(res).tobytes() == g[name + "/guess"].tobytes()


def test_input_validation(ctx_auto, golden):
    g, _ = golden
    P = problem(g, "street")
    empty = np.zeros((0, 3), np.float32)
    for over in (dict(src=empty), dict(tgt=empty)):
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.gicp(**dict(P, **over))
        assert e.value.args[1] == E_INVALID and "empty" in str(e.value)
    for which, bad in (("src", np.nan), ("tgt", np.inf), ("src", -np.inf)):
        c = P[which].copy()
        c[len(c) // 2, 1] = bad
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.gicp(**dict(P, **{which: c}))
        assert e.value.args[1] == E_INVALID and "finite" in str(e.value)
    guess = np.eye(4)
    guess[0, 3] = np.nan
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.gicp(**dict(P, init_guess=guess))
    assert e.value.args[1] == E_INVALID
    for k in (2, 33):
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.gicp(**P, params=abi.gicp_params(k_correspondences=k))
        assert e.value.args[1] == E_INVALID and "k_correspondences" in str(e.value)
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.gicp(**P, params=abi.gicp_params(using_voxel_gicp=0))
    assert e.value.args[1] == E_UNSUPPORTED
    # a coordinate beyond 2^20 voxels: 3e6 m at 1 m voxels, in the target and in the source
    for which in ("tgt", "src"):
        far = np.concatenate([P[which], [[3.0e6, 0.0, 0.0]]]).astype(np.float32)
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.gicp(**dict(P, **{which: far}))
        assert e.value.args[1] == E_UNSUPPORTED and "2^20" in str(e.value)
    check(run(ctx_auto, g, "street"), g, "street", "after the refused calls")


def test_host_and_device_clouds(ctx_auto, golden):
    g, _ = golden
    for name in ("street_guess", "crafted"):
        P = problem(g, name)
        want = key(run(ctx_auto, g, name))
        dt, ds = DevCloud(P["tgt"], 3), DevCloud(P["src"], 5)
        assert key(ctx_auto.gicp(**dict(P, tgt=dt.cloud, src=ds.cloud), params=params(g, name))) == want, name
        # host records of 48 bytes
        rec_t, rec_s = np.zeros(len(P["tgt"]), abi.POINT_DTYPE), np.zeros(len(P["src"]), abi.POINT_DTYPE)
        for rec, pts in ((rec_t, P["tgt"]), (rec_s, P["src"])):
            rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
        assert key(ctx_auto.gicp(**dict(P, tgt=rec_t, src=rec_s), params=params(g, name))) == want, name
        # mixed: a device target with a host source
        assert key(ctx_auto.gicp(**dict(P, tgt=dt.cloud), params=params(g, name))) == want, name
        dt.free(), ds.free()


BATCH = ["street", "no_overlap", "street_large", "crafted", "too_few", "street_guess", "exact_k", "no_overlap", "outliers", "street_tight"]


def test_batch_equals_single_calls(ctx_auto, golden):
    """mixed sizes under one parameter set; no_overlap ends at its first tick and too_few runs none, among problems that run for several (crafted: 64)"""
    g, _ = golden
    for over in (dict(), dict(voxel_resolution=2.0, k_correspondences=7), dict(apply_intersection_filter=1, max_iterations=5)):
        prm = abi.gicp_params(**over)
        probs = [problem(g, n) for n in BATCH]
        single = [ctx_auto.gicp(**p, params=prm) for p in probs]
        ticks = [r.iterations for r in single]
        assert min(ticks) == 0 and max(ticks) >= 4
        single = [key(r) for r in single]
        got = [key(r) for r in ctx_auto.gicp_batch(probs, prm)]
        assert got == single, over
        # cut into sub-batches by a small scratch limit: 1 MiB holds none of these problems (each then runs alone), 4 MiB two or three
        for limit in (1 << 20, 4 << 20):
            cut = abi.gicp_params(scratch_limit_bytes=limit, **over)
            assert [key(r) for r in ctx_auto.gicp_batch(probs, cut)] == single, (over, limit)
    assert ctx_auto.gicp_batch([], abi.gicp_params()) == []


def test_batch_with_defaults_equals_the_fixture(ctx_auto, golden):
    g, _ = golden
    names = ["street", "street_guess", "street_near_identity", "street_tight", "street_large", "crafted", "exact_k", "k_plus_1", "outliers"]  # default parameters
    for res, n in zip(ctx_auto.gicp_batch([problem(g, n) for n in names]), names):
        check(res, g, n, n + " in a batch")


def test_bad_problem_in_a_batch_is_refused(ctx_auto, golden):
    g, _ = golden
    P = problem(g, "street")
    bad = dict(P, src=np.zeros((0, 3), np.float32))
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.gicp_batch([P, bad, P])
    assert e.value.args[1] == E_INVALID and "problem 1" in str(e.value)
    nf = P["src"].copy()
    nf[3, 2] = np.nan
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.gicp_batch([P, P, dict(P, src=nf)])
    assert e.value.args[1] == E_INVALID and "problem 2" in str(e.value)
    far = np.concatenate([P["tgt"], [[0.0, -3.0e6, 0.0]]]).astype(np.float32)
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.gicp_batch([dict(P, tgt=far), P])
    assert e.value.args[1] == E_UNSUPPORTED and "problem 0" in str(e.value)


def test_two_contexts_from_two_threads(golden):
    g, _ = golden
    names = ["street_k32", "crafted", "street_large", "street_guess"]
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
