"""GPU tests of what mulls_ndt, mulls_gicp and mulls_pcl_icp share inside one context: one device arena and pinned buffer, one set of cell-table kernels with
their clear, one per-problem head.  A call must not see what another method, or a larger problem, left there: stale keys, counts or fill words in the part
of the arena its tables now occupy, a head of another method, a running word left set.

Every comparison is equality of bits of the whole result (the keys of tests/test_gpu_ndt.py, test_gpu_gicp.py and test_gpu_pcl_icp.py) with the same call
on a fresh context, which has no history."""

import numpy as np
import pytest

import reg_edges as E
import test_gpu_gicp as tg
import test_gpu_ndt as tn
import test_gpu_pcl_icp as tp
from mulls_amd import abi, lib
from test_reg_edges import GOLDEN as EDGES

pytestmark = pytest.mark.gpu

METHODS = ("ndt", "gicp", "pcl_plane_recip", "pcl_point")
ORDER = ("ndt", "gicp", "pcl_plane_recip", "pcl_point", "gicp", "ndt")
HELPERS = {"ndt": tn, "gicp": tg, "pcl_plane_recip": tp, "pcl_point": tp}


def _load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    """(problem, params) of every method's small and large case: the fixtures' street pairs of 1 500 and 400 points, and a pair of more than 4 096 source
    points and six times the target (wide_8193 of the edge fixtures; mulls_pcl_icp on it is cut to 4 iterations)"""
    gn, gg, gp = _load(tn.GOLDEN), _load(tg.GOLDEN), _load(tp.GOLDEN)
    en, eg = _load(EDGES["ndt"]), _load(EDGES["gicp"])
    plane = dict(metrics=abi.PCL_ICP_POINT2PLANE, use_reciprocal_correspondence=1, max_iter_num=4)
    wide = E.problem(eg, "wide_8193")
    out = {("ndt", "small"): (tn.problem(gn, "street"), tn.params(gn, "street")),
           ("ndt", "large"): (E.problem(en, "wide_8193"), tn.params(en, "wide_8193")),
           ("gicp", "small"): (tg.problem(gg, "street"), tg.params(gg, "street")),
           ("gicp", "large"): (E.problem(eg, "wide_8193"), tg.params(eg, "wide_8193")),
           ("pcl_plane_recip", "small"): (tp.problem(gp, "street_plane_recip"), tp.params(gp, "street_plane_recip")),
           ("pcl_plane_recip", "large"): (wide, abi.pcl_icp_params(**plane)),
           ("pcl_point", "small"): (tp.problem(gp, "street"), tp.params(gp, "street")),
           ("pcl_point", "large"): (wide, abi.pcl_icp_params(max_iter_num=4))}
    for m in METHODS:
        small, large = out[(m, "small")][0], out[(m, "large")][0]
        assert len(small["tgt"]) == 1500 and len(small["src"]) == 400, m
        assert len(large["src"]) > 4096 and len(large["src"]) >= 4 * len(small["src"]) and len(large["tgt"]) >= 4 * len(small["tgt"]), m
    return out


def call(ctx, method, P, prm):
    return getattr(ctx, "pcl_icp" if method.startswith("pcl") else method)(**P, params=prm)


def batch(ctx, method, probs, prm):
    return getattr(ctx, ("pcl_icp" if method.startswith("pcl") else method) + "_batch")(probs, prm)


def fresh(method, P, prm):
    """the call's key on a context of its own"""
    c = lib.Context(0)
    try:
        return HELPERS[method].key(call(c, method, P, prm))
    finally:
        c.close()


@pytest.fixture(scope="module")
def alone(cases):
    return {k: fresh(k[0], *v) for k, v in cases.items()}


def test_methods_and_sizes_in_turn_on_one_context(cases, alone):
    """NDT, GICP, pcl_icp Point2Plane reciprocal, pcl_icp Point2Point, GICP, NDT on one context, each on the small pair, the large one and the small one
    again: the small tables after the large ones lie where the large problem's arrays were"""
    assert len({alone[(m, "small")] for m in METHODS}) == len(METHODS)  # (four different answers: a result taken from another method's would show)
    c = lib.Context(0)
    try:
        for turn, m in enumerate(ORDER):
            for size in ("small", "large", "small"):
                got = HELPERS[m].key(call(c, m, *cases[(m, size)]))
                assert got == alone[(m, size)], (turn, m, size)
    finally:
        c.close()


@pytest.mark.parametrize("method", METHODS)
def test_batch_around_a_problem_the_crop_empties(cases, alone, method):
    """a batch of three whose middle problem is empty after the crop equals the single calls: the problem that builds no table and runs no tick stands
    between two that do, on a context whose arena the large problem has filled before"""
    small, large = cases[(method, "small")][0], cases[(method, "large")][0]
    prm = {"ndt": lambda: abi.ndt_params(apply_intersection_filter=1), "gicp": lambda: abi.gicp_params(apply_intersection_filter=1),
           "pcl_plane_recip": lambda: abi.pcl_icp_params(metrics=abi.PCL_ICP_POINT2PLANE, use_reciprocal_correspondence=1, max_iter_num=4),
           "pcl_point": lambda: abi.pcl_icp_params(max_iter_num=4)}[method]()  # (the crop is on by default in mulls_pcl_icp)
    gone = dict(small, tgt_bound=small["tgt_bound"] + 1000.0)
    probs = [small, gone, large]
    key = HELPERS[method].key
    single = [fresh(method, P, prm) for P in probs]
    c = lib.Context(0)
    try:
        res = call(c, method, gone, prm)
        assert res.n_src == 0 and res.n_tgt == 0 and res.code == -3 and res.iterations == 0
        assert key(call(c, method, large, prm)) == single[2]
        assert [key(r) for r in batch(c, method, probs, prm)] == single, method
        assert [key(r) for r in batch(c, method, probs[::-1], prm)] == single[::-1], method
    finally:
        c.close()
