"""GPU tests of mulls_pcl_icp / mulls_pcl_icp_batch through mulls_amd/lib.py against the numpy restatement of the library's definition
(tests/pcl_icp_restated.py), read from tests/golden/pcl_icp_cases.npz (tests/test_pcl_icp.py keeps the fixture equal to the restatement and asserts
which case takes which path).

Every comparison with the restatement and between launch forms is equality of bits of T, fitness, mse and the integer fields: the definition has no
operation whose host and device results may differ (+ - * / sqrt in double or float in a stated order, sin / cos from detmath.h, no contraction), and
the restatement's searches are brute force, so equal bits also say that the 27-cell walks are exact.

PCL, FLANN and Eigen are not available where these tests run: nothing here was compared with them."""
import json
import threading

import numpy as np
import pytest

from mulls_amd import abi, lib
from test_gpu_ndt import DevCloud
from test_pcl_icp import ALL, GOLDEN, cloud_of

pytestmark = pytest.mark.gpu

INT_FIELDS = ("code", "iterations", "converged", "stop", "n_src", "n_tgt", "n_corr", "n_fit")
FLOAT_FIELDS = ("fitness", "mse")
E_INVALID, E_UNSUPPORTED = -100, -103


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}, json.loads(str(z["names"]))


def problem(g, name, **over):
    p = dict(tgt=cloud_of(g, name, "tgt"), src=cloud_of(g, name, "src"), tgt_bound=g[name + "/tgt_bound"], src_bound=g[name + "/src_bound"],
             init_guess=g[name + "/guess"])
    p.update(over)
    return p


def params(g, name, **over):
    prm = json.loads(str(g[name + "/prm"]))
    prm.update(over)
    return abi.pcl_icp_params(**prm)


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
    return ctx.pcl_icp(**problem(g, name), params=params(g, name))


@pytest.mark.parametrize("name", ALL)
def test_fixture_case(ctx_auto, golden, name):
    """the paths: Point2Point and Point2Plane with and without reciprocity, every stop rule (ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE,
    NO_CORRESPONDENCES at iteration 0 and at a later one, SINGULAR), the guess and the near-identity guess, the crop and no crop, a start at the truth,
    a cloud that is empty after the crop, more than MULLS_NDT_TREE source points (street_large), ties in (d2, index) from both sides, identical points,
    points on cell faces, a pair at exactly the distance, neighbourhoods of 2 and of 3 points and one larger than a tile of the normals kernel
    (crafted*), a source of exactly 3 pairs and of 2"""
    g, names = golden
    assert names == ALL
    res = run(ctx_auto, g, name)
    check(res, g, name)
    if name == "empty":
        assert res.n_src == 0 and res.code == -3 and res.stop == abi.PCL_ICP_STOP_NONE and pose(res).tobytes() == np.eye(4).tobytes()
    if name == "lifted":
        assert res.n_corr == 0 and res.stop == abi.PCL_ICP_STOP_NO_CORRESPONDENCES and res.iterations == 0


def test_refusals_leave_the_context_usable(ctx_auto, golden):
    g, _ = golden
    P = problem(g, "street")
    empty = np.zeros((0, 3), np.float32)
    for over in (dict(src=empty), dict(tgt=empty)):
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.pcl_icp(**dict(P, **over))
        assert e.value.args[1] == E_INVALID and "empty" in str(e.value)
    for which, bad in (("src", np.nan), ("tgt", np.inf), ("src", -np.inf)):
        c = P[which].copy()
        c[len(c) // 2, 1] = bad
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.pcl_icp(**dict(P, **{which: c}))
        assert e.value.args[1] == E_INVALID and "finite" in str(e.value)
    guess = np.eye(4)
    guess[0, 3] = np.nan
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.pcl_icp(**dict(P, init_guess=guess))
    assert e.value.args[1] == E_INVALID
    invalid = [dict(max_iter_num=0), dict(max_iter_num=-3), dict(dis_thre_unit=0.0), dict(dis_thre_unit=-1.0), dict(dis_thre_unit=np.inf), dict(dis_thre_unit=np.nan),
               dict(neighbor_radius=0.0), dict(neighbor_radius=np.nan), dict(transformation_epsilon=-1e-9), dict(transformation_epsilon=np.inf),
               dict(euclidean_fitness_epsilon=-1.0), dict(euclidean_fitness_epsilon=np.nan), dict(metrics=3), dict(ce=2), dict(te=-1)]
    for over in invalid:
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.pcl_icp(**P, params=abi.pcl_icp_params(**over))
        assert e.value.args[1] == E_INVALID, over
    unsupported = [(dict(metrics=abi.PCL_ICP_PLANE2PLANE), "Plane2Plane"), (dict(te=abi.PCL_ICP_LM), "LM"), (dict(ce=abi.PCL_ICP_NS, metrics=abi.PCL_ICP_POINT2PLANE), "NS"),
                   (dict(use_trimmed_rejector=1), "trimmed")]
    for over, word in unsupported:
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.pcl_icp(**P, params=abi.pcl_icp_params(**over))
        assert e.value.args[1] == E_UNSUPPORTED and word in str(e.value), over
    # a coordinate beyond 2^20 cells: 3e6 m at 1.5 m cells, in the target and in the source; and of the normals' cells alone
    for which in ("tgt", "src"):
        far = np.concatenate([P[which], [[3.0e6, 0.0, 0.0]]]).astype(np.float32)
        with pytest.raises(lib.MullsError) as e:
            ctx_auto.pcl_icp(**dict(P, **{which: far}), params=abi.pcl_icp_params(apply_intersection_filter=0))
        assert e.value.args[1] == E_UNSUPPORTED and "2^20" in str(e.value)
    far = np.concatenate([P["tgt"], [[0.0, -3.0e5, 0.0]]]).astype(np.float32)
    wide = abi.pcl_icp_params(apply_intersection_filter=0, metrics=abi.PCL_ICP_POINT2PLANE, neighbor_radius=0.25)
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.pcl_icp(**dict(P, tgt=far), params=wide)
    assert e.value.args[1] == E_UNSUPPORTED and "2^20" in str(e.value)
    for name in ("street", "street_plane_recip"):
        check(run(ctx_auto, g, name), g, name, "after the refused calls")


def test_host_and_device_clouds(ctx_auto, golden):
    g, _ = golden
    for name in ("street_guess", "crafted_plane"):
        P = problem(g, name)
        want = key(run(ctx_auto, g, name))
        dt, ds = DevCloud(P["tgt"], 3), DevCloud(P["src"], 5)
        assert key(ctx_auto.pcl_icp(**dict(P, tgt=dt.cloud, src=ds.cloud), params=params(g, name))) == want, name
        # host records of 48 bytes
        rec_t, rec_s = np.zeros(len(P["tgt"]), abi.POINT_DTYPE), np.zeros(len(P["src"]), abi.POINT_DTYPE)
        for rec, pts in ((rec_t, P["tgt"]), (rec_s, P["src"])):
            rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
        assert key(ctx_auto.pcl_icp(**dict(P, tgt=rec_t, src=rec_s), params=params(g, name))) == want, name
        # mixed: a device target with a host source
        assert key(ctx_auto.pcl_icp(**dict(P, tgt=dt.cloud), params=params(g, name))) == want, name
        dt.free(), ds.free()


BATCH = ["street", "lifted", "street_large", "crafted", "empty", "street_guess", "three_pairs", "two_pairs", "late_loss", "street_tight", "singular"]


def test_batch_equals_single_calls(ctx_auto, golden):
    """mixed sizes under one parameter set: lifted and two_pairs stop at tick 0, empty runs no tick at all, late_loss stops at tick 1, and under
    max_iter_num = 4 the street problems run to the cap"""
    g, _ = golden
    sets = (dict(), dict(metrics=abi.PCL_ICP_POINT2PLANE, use_reciprocal_correspondence=1, max_iter_num=4, neighbor_radius=1.5),
            dict(use_reciprocal_correspondence=1, dis_thre_unit=1.0, apply_intersection_filter=0, transformation_epsilon=0.0))
    for over in sets:
        prm = abi.pcl_icp_params(**over)
        probs = [problem(g, n) for n in BATCH]
        single = [ctx_auto.pcl_icp(**p, params=prm) for p in probs]
        ticks = dict(zip(BATCH, [r.iterations for r in single]))
        assert ticks["lifted"] == 0 and ticks["empty"] == 0 and ticks["two_pairs"] == 0 and max(ticks.values()) >= 4
        if over.get("apply_intersection_filter", 1):
            assert single[BATCH.index("empty")].stop == abi.PCL_ICP_STOP_NONE and single[BATCH.index("empty")].n_src == 0
        if "max_iter_num" in over:
            assert sum(r.stop == abi.PCL_ICP_STOP_ITERATIONS and r.iterations == over["max_iter_num"] for r in single) >= 3
        single = [key(r) for r in single]
        got = [key(r) for r in ctx_auto.pcl_icp_batch(probs, prm)]
        assert got == single, over
        # cut into sub-batches by a small scratch limit: under 1 MiB every problem runs alone (the partial sums take 0.9 MiB a problem), 4 MiB holds two to four
        for limit in (1 << 20, 4 << 20):
            cut = abi.pcl_icp_params(scratch_limit_bytes=limit, **over)
            assert [key(r) for r in ctx_auto.pcl_icp_batch(probs, cut)] == single, (over, limit)
    assert ctx_auto.pcl_icp_batch([], abi.pcl_icp_params()) == []


def test_batch_with_defaults_equals_the_fixture(ctx_auto, golden):
    g, _ = golden
    names = [n for n in ALL if json.loads(str(g[n + "/prm"])) == {}]  # default parameters
    assert names == ["street", "street_guess", "street_near_identity", "street_tight", "empty", "exact_subset"]
    for res, n in zip(ctx_auto.pcl_icp_batch([problem(g, n) for n in names]), names):
        check(res, g, n, n + " in a batch")


def test_bad_problem_in_a_batch_is_refused(ctx_auto, golden):
    g, _ = golden
    P = problem(g, "street")
    bad = dict(P, src=np.zeros((0, 3), np.float32))
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.pcl_icp_batch([P, bad, P])
    assert e.value.args[1] == E_INVALID and "problem 1" in str(e.value)
    nf = P["src"].copy()
    nf[3, 2] = np.nan
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.pcl_icp_batch([P, P, dict(P, src=nf)])
    assert e.value.args[1] == E_INVALID and "problem 2" in str(e.value)
    far = np.concatenate([P["tgt"], [[0.0, -3.0e6, 0.0]]]).astype(np.float32)
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.pcl_icp_batch([dict(P, tgt=far), P], abi.pcl_icp_params(apply_intersection_filter=0))
    assert e.value.args[1] == E_UNSUPPORTED and "problem 0" in str(e.value)
    check(ctx_auto.pcl_icp_batch([P])[0], g, "street", "after the refused batches")


def test_two_contexts_from_two_threads(golden):
    g, _ = golden
    names = ["street_plane_recip", "crafted", "street_large", "street_guess"]
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
