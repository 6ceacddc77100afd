"""GPU tests of mulls_ndt / mulls_gicp and their batch forms at size and at their tables' edges: the cases of tests/reg_edges.py, read from
tests/golden/ndt_edges.npz and tests/golden/gicp_edges.npz (tests/test_reg_edges.py keeps the fixtures equal to the numpy restatements and asserts which
case reaches which edge: the later trips of the strided partials, probe sequences that run long and wrap past the last slot, tables of 32 768 slots,
cells fuller than the one-lane sort's first gap, cells at -1048576 and 1048575, int32 keys near 2^31, k = 3, 8, 9 and 21).

Every comparison is equality of bits, as in tests/test_gpu_ndt.py and tests/test_gpu_gicp.py, whose helpers run here.

Neither ndt_omp, fast_gicp nor PCL is available where these tests run: nothing here was compared with them."""
import json

import numpy as np
import pytest

import reg_edges as E
import test_gpu_gicp as tg
import test_gpu_ndt as tn
from mulls_amd import abi, lib
from test_gpu_ndt import DevCloud
from test_reg_edges import GICP_NAMES, GOLDEN, NDT_NAMES

pytestmark = pytest.mark.gpu


class Solver:
    def __init__(self, name, helpers, names, old_golden, make_params, first_tick):
        self.name, self.h, self.names, self.old_golden, self.make_params, self.first_tick = name, helpers, names, old_golden, make_params, first_tick

    def call(self, ctx, **kw):
        return getattr(ctx, self.name)(**kw)

    def batch(self, ctx, probs, prm):
        return getattr(ctx, self.name + "_batch")(probs, prm)

    def run(self, ctx, g, name):
        return self.call(ctx, **E.problem(g, name), params=self.h.params(g, name))


SOLVERS = {"ndt": Solver("ndt", tn, NDT_NAMES, tn.GOLDEN, abi.ndt_params, "no_leaves"),
           "gicp": Solver("gicp", tg, GICP_NAMES, tg.GOLDEN, abi.gicp_params, "no_overlap")}


@pytest.fixture(scope="module")
def golden():
    out = {}
    for s, S in SOLVERS.items():
        z, old = np.load(GOLDEN[s]), np.load(S.old_golden)
        out[s] = ({k: z[k] for k in z.files}, {k: old[k] for k in old.files})
        assert json.loads(str(z["names"])) == S.names
    return out


@pytest.mark.parametrize("solver,name", [(s, n) for s, S in SOLVERS.items() for n in S.names])
def test_fixture_case(ctx_auto, golden, solver, name):
    """every case gives the restatement's bits: integer fields, float fields and T"""
    S, (g, _) = SOLVERS[solver], golden[solver]
    res = S.run(ctx_auto, g, name)
    S.h.check(res, g, name)
    assert res.iterations >= 1


@pytest.mark.parametrize("solver", ["ndt", "gicp"])
def test_device_clouds_and_host_records(ctx_auto, golden, solver):
    """wide_8193 and dense_table from device clouds at strides of 3 and 5 floats, and from host records of 48 bytes"""
    S, (g, _) = SOLVERS[solver], golden[solver]
    for name in ("wide_8193", "dense_table"):
        P, prm = E.problem(g, name), S.h.params(g, name)
        want = S.h.key(S.call(ctx_auto, **P, params=prm))
        S.h.check(S.call(ctx_auto, **P, params=prm), g, name)
        for st, ss in ((3, 5), (5, 3)):
            dt, ds = DevCloud(P["tgt"], st), DevCloud(P["src"], ss)
            try:
                assert S.h.key(S.call(ctx_auto, **dict(P, tgt=dt.cloud, src=ds.cloud), params=prm)) == want, (name, st, ss)
            finally:
                dt.free(), ds.free()
        rec_t, rec_s = np.zeros(len(P["tgt"]), abi.POINT_DTYPE), np.zeros(len(P["src"]), abi.POINT_DTYPE)
        for rec, pts in ((rec_t, P["tgt"]), (rec_s, P["src"])):
            rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
        assert S.h.key(S.call(ctx_auto, **dict(P, tgt=rec_t, src=rec_s), params=prm)) == want, name


BATCH = ["wide_8193", "old:street", "old:first_tick", "dense_table", "full_cell", "wide_4097"]


@pytest.mark.parametrize("solver", ["ndt", "gicp"])
def test_batch_equals_single_calls(ctx_auto, golden, solver):
    """one parameter set (the crop off, else the defaults) over the wide problem, small ones and one that ends at its first tick: the launches' n_max and
    table_max come from wide_8193 while the small problems share the grid.  Then under a scratch limit that cuts the batch (consecutive problems are
    taken while their arenas fit: the three small ones in the middle share a sub-batch, the others run alone) and under one that no problem fits."""
    S, (g, old) = SOLVERS[solver], golden[solver]
    prm = dict(apply_intersection_filter=0)
    probs = []
    for n in BATCH:
        if n.startswith("old:"):
            probs.append(S.h.problem(old, S.first_tick if n == "old:first_tick" else n[4:]))
        else:
            probs.append(E.problem(g, n))
    single = [S.call(ctx_auto, **p, params=S.make_params(**prm)) for p in probs]
    for n, r in zip(BATCH, single):
        if not n.startswith("old:"):  # (these cases' own parameters are this set)
            assert json.loads(str(g[n + "/prm"])) in ({}, prm)
            S.h.check(r, g, n, n + " alone")
    ft = single[BATCH.index("old:first_tick")]
    assert (ft.evaluations == 1 and ft.iterations == 0) if solver == "ndt" else (ft.iterations == 0 and ft.stop == abi.GICP_STOP_SINGULAR and ft.n_corr == 0)
    assert max(r.iterations for r in single) >= 3
    single = [S.h.key(r) for r in single]
    assert [S.h.key(r) for r in S.batch(ctx_auto, probs, S.make_params(**prm))] == single
    for limit in ((1 << 20, 4 << 20) if solver == "ndt" else (1 << 20, 8 << 20)):
        cut = S.make_params(scratch_limit_bytes=limit, **prm)
        assert [S.h.key(r) for r in S.batch(ctx_auto, probs, cut)] == single, limit


@pytest.mark.parametrize("solver", ["ndt", "gicp"])
def test_repeats_in_one_context(golden, solver):
    """a context of its own, so that the scratch arena's history is this test's: small, wide_8193, small, wide_8193.  The arena and the 28 x 4096 partials
    are reused; after wide_8193 the lanes beyond a small problem's n must hold zeros again."""
    S, (g, old) = SOLVERS[solver], golden[solver]
    c = lib.Context(0)
    try:
        for step in range(2):
            small = S.call(c, **S.h.problem(old, "street"), params=S.h.params(old, "street"))
            S.h.check(small, old, "street", "street, round %d" % step)
            S.h.check(S.run(c, g, "wide_8193"), g, "wide_8193", "wide_8193, round %d" % step)
            S.h.check(S.run(c, g, "dense_table"), g, "dense_table", "dense_table after wide_8193, round %d" % step)
    finally:
        c.close()
