"""GPU tests of mulls_coarse_reg_teaser_batch through mulls_amd/lib.py: results[b] and the clique of problem b are what the definition gives for problem b alone.

Expected values are the fixture tests/golden/teaser_cases.npz (the numpy restatement, tests/test_teaser.py) where a set's own noise bound and min_inlier_num
are the batch's, and the same restatement (tests/teaser_restated.py: restate) run at the batch's parameters where they are not: a batch has ONE
mulls_teaser_params, and the fixture's sets do not all share theirs (exit_limit: 1e6; the planted sets: min_inlier_num 3; the demo lists: 0.25 and 1.0).  So the
mixed batch runs at 0.2 (the fixture's bound of all its sets but exit_limit) and again at 1e6 (exit_limit's: it runs all 100 GNC iterations beside problems that
stop at iteration 0), and the demo lists run at 0.25 and at 1.0.  The single entry points compile the kernel text of the batch and share its argument checker, so no expectation comes
from them: they appear only where the search's effort (clique_nodes, which the restatement does not define) must be the same through either entry form, and in
test_one_problem_equals_the_single_call, which holds the two entry forms against each other.

Every comparison is equality, as in tests/test_gpu_teaser.py: the integers, the clique list, every bit of cost and T; clique_nodes equals the single call's
when the host search runs."""
import ctypes as C

import numpy as np
import pytest

import teaser_restated as tr
from mulls_amd import abi, lib
from test_gpu_teaser import as_dict, assert_same, cloud_of, device, strided
from test_teaser import demo, fixture_case, input_sets

pytestmark = pytest.mark.gpu

MIXED = ["no_edge", "single_edge", "two_cliques", "exit_mu", "exit_mu_exact", "exit_cost", "exit_limit", "nonfinite_64", "size_31", "size_32", "size_33",
         "size_63", "size_64", "size_65", "planted_40_50", "complete_300", "three_pairs", "unequal"]
EDGES = ["size_1023", "size_1024", "size_1025", "size_64", "size_33"]
FAILED = dict(status=-1, n_edges=0, max_core=0, clique_size=0, clique_exact=0, gnc_iterations=0, n_rotation_inliers=0, n_translation_inliers=0, cost=0.0,
              T=np.eye(4), clique=np.zeros(0, np.int64), clique_nodes=0)


def clouds(name):
    """(t, s) of a set as (n, 48) records; three_pairs and unequal are upstream's early returns"""
    if name == "three_pairs":
        t, s, _ = input_sets()["size_31"]
        return tr.records(t[:3]), tr.records(s[:3])
    if name == "unequal":
        return tr.records(input_sets()["size_33"][0]), tr.records(input_sets()["size_31"][1])
    t, s, _ = input_sets()[name]
    return tr.records(t), tr.records(s)


def run_batch(ctx, problems, nb, min_inlier=8, limit=0):
    return [as_dict(r, c) for r, c in ctx.coarse_reg_teaser_batch(problems, abi.teaser_params(nb, min_inlier), limit)]


@pytest.fixture(scope="module")
def expected(ctx_auto):
    """what problem `name` must give at (nb, min_inlier): the fixture where its parameters are these, else the numpy restatement run at them (every such set is
    small: at most 0.3 s, complete_300 at 1e6) — computed once, left unchanged.  single=True: the single entry point, for its clique_nodes and for the
    test of the two entry forms against each other."""
    cache, from_fixture = {}, set()

    def get(name, nb, min_inlier=8, single=False):
        key = (name, nb, min_inlier, single)
        if key not in cache:
            if name in ("three_pairs", "unequal"):
                cache[key] = FAILED
            elif single:
                t, s = clouds(name)
                cache[key] = device(ctx_auto, t, s, nb, min_inlier)
            elif np.float32(input_sets()[name][2]) == np.float32(nb) and tr.min_inlier(name) == min_inlier:
                cache[key] = fixture_case(name)
                from_fixture.add(key[:3])
            else:
                t, s, _ = input_sets()[name]
                cache[key] = tr.restate(t, s, nb, min_inlier)
                assert cache[key]["clique_exact"] == 1
        return cache[key]

    get.from_fixture = from_fixture  # the (name, nb, min_inlier) whose expectation is the fixture's and not the restatement's run here
    return get


def check(got, names, nb, expected, what, nodes=True):
    assert len(got) == len(names)
    for g, name in zip(got, names):
        assert_same(g, expected(name, nb), (what, name))
        if nodes and name not in ("three_pairs", "unequal"):  # the host search's effort is the single call's
            assert g["clique_nodes"] == expected(name, nb, single=True)["clique_nodes"], (what, name)


@pytest.mark.parametrize("nb", [0.2, 1e6], ids=["nb02", "nb1e6"])
def test_mixed_batch_forward_reversed_and_one_per_sub_batch(ctx_auto, expected, nb):
    """problems that stop the GNC loop at iteration 0 (mu <= 0), after a few (the cost settles) and never (exit_limit at 1e6: 100 iterations), that never enter it
    (no edge), and upstream's early returns, in one batch: the stop mask and the frozen records.  Reversed, and cut into one problem per sub-batch, the same."""
    problems = [clouds(name) for name in MIXED]
    exits = {name: expected(name, nb)["gnc_iterations"] for name in MIXED}
    if nb == 1e6:
        assert exits["exit_limit"] == 100 and ("exit_limit", nb, 8) in expected.from_fixture and exits["size_64"] < 100
    else:
        assert exits["no_edge"] == 0 and exits["exit_mu"] == 1 and 1 < exits["exit_cost"] < 100  # three kinds of exit side by side
    check(run_batch(ctx_auto, problems, nb), MIXED, nb, expected, "forward")
    check(run_batch(ctx_auto, problems[::-1], nb), MIXED[::-1], nb, expected, "reversed")
    check(run_batch(ctx_auto, problems, nb, limit=1), MIXED, nb, expected, "limit 1")


def test_word_and_wave_edges_of_unequal_sizes(ctx_auto, expected):
    """N = 1023, 1024, 1025, 64, 33 in one launch of every kernel: each problem's loops end at its own n / W / m"""
    check(run_batch(ctx_auto, [clouds(name) for name in EDGES], 0.2), EDGES, 0.2, expected, "edges")


def test_min_inlier_of_the_planted_sets(ctx_auto, expected):
    names = ["planted_40_50", "planted_40_90", "planted_200_90", "size_31"]
    got = run_batch(ctx_auto, [clouds(name) for name in names], 0.2, 3)
    for g, name in zip(got, names):
        assert_same(g, expected(name, 0.2, 3), name)
    assert ("planted_40_90", 0.2, 3) in expected.from_fixture and got[1]["status"] == 1


@pytest.fixture(scope="module")
def device_kpts():
    """the demo key points of both scans in device memory of the caller's own (straight from the HIP runtime)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    out, held = {}, []
    for k in (0, 15):
        raw = abi.records(demo()["kpts_%d" % k]).copy()
        dev = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev), raw.nbytes) == 0
        assert hip.hipMemcpy(dev, C.c_void_p(raw.ctypes.data), raw.nbytes, 1) == 0  # hipMemcpyHostToDevice
        c = abi.Cloud()
        c.pts, c.n, c.stride = dev.value, len(raw), abi.POINT_BYTES
        out[k], held = c, held + [dev]
    yield out
    for dev in held:
        assert hip.hipFree(dev) == 0


@pytest.mark.parametrize("nb", [0.25, 1.0], ids=["nb25", "nb100"])
def test_demo_lists_three_ways_strided_and_capped(ctx_auto, device_kpts, nb):
    """demo_recip_0_15 and demo_fixed300_15_0 as gathered host clouds, as indexed problems on the host key points, as indexed problems on device-resident key
    points (on both sides and on one), as a strided host cloud, and with a clique buffer smaller than the clique: the fixture's results"""
    Z = demo()
    problems, wants, caps = [], [], []
    held = []
    for name, (a, b) in (("recip_0_15", (0, 15)), ("fixed300_15_0", (15, 0))):
        want = fixture_case("demo_%s_nb%d" % (name, int(100 * nb)))
        t, s, _ = input_sets()["demo_%s_nb%d" % (name, int(100 * nb))]
        rt, rs = tr.records(t), tr.records(s)
        kt, ks, pr = Z["kpts_%d" % a], Z["kpts_%d" % b], Z[name + "_pairs"]
        bt, ct = strided(rt, 36, 5)
        held.append(bt)
        cap = want["clique_size"] - 3
        for prob in (dict(tgt=rt, src=rs), dict(tgt=kt, src=ks, tgt_idx=pr[:, 0], src_idx=pr[:, 1]),
                     dict(tgt=device_kpts[a], src=device_kpts[b], tgt_idx=pr[:, 0], src_idx=pr[:, 1]),
                     dict(tgt=device_kpts[a], src=ks, tgt_idx=pr[:, 0], src_idx=pr[:, 1]), dict(tgt=ct, src=rs), dict(tgt=rt, src=rs, cap=cap),
                     dict(tgt=kt, src=device_kpts[b], tgt_idx=pr[:, 0], src_idx=pr[:, 1], cap=0)):
            problems.append(prob)
            wants.append(want)
            caps.append(prob.get("cap"))
    got = run_batch(ctx_auto, problems, nb)  # (lib.py checks that the slot behind every cap is left alone)
    for k, (g, want, cap) in enumerate(zip(got, wants, caps)):
        assert_same(g, want, (k, nb), clique=cap is None)
        if cap is not None:
            assert 0 <= cap < want["clique_size"] and np.array_equal(g["clique"], want["clique"][:cap]), k


def test_one_problem_equals_the_single_call(ctx_auto, expected):
    for name in ("size_65", "exit_cost", "no_edge", "three_pairs"):
        (got,) = run_batch(ctx_auto, [clouds(name)], 0.2)
        assert_same(got, expected(name, 0.2), name)
        assert_same(got, expected(name, 0.2, single=True), name)
        assert got["clique_nodes"] == expected(name, 0.2, single=True)["clique_nodes"]
    assert ctx_auto.coarse_reg_teaser_batch([]) == []  # n_problems = 0: MULLS_OK


def test_device_search_gives_the_same_batch(expected):
    """MULLS_OPT_TEASER_DEVICE_SEARCH = 1: everything but clique_nodes, which need not repeat"""
    ctx = lib.Context(0)
    try:
        ctx.set_option(abi.OPT_TEASER_DEVICE_SEARCH, 1)
        names = MIXED + ["size_1025"]
        got = run_batch(ctx, [clouds(name) for name in names], 0.2)
        check(got, names, 0.2, expected, "device search", nodes=False)
        assert all(g["clique_exact"] == 1 for g, name in zip(got, names) if name not in ("three_pairs", "unequal"))
    finally:
        ctx.close()


def raw_problems(specs):
    """mulls_teaser_problem records by hand: (tgt cloud, src cloud, tgt_idx, src_idx) and a clique buffer of four slots, filled with -7, for each"""
    arr = (abi.TeaserProblem * len(specs))()
    bufs = np.full((len(specs), 8), -7, np.int32)
    for k, (ct, cs, ti, si) in enumerate(specs):
        arr[k].tgt, arr[k].src = ct, cs
        if ti is not None:
            arr[k].tgt_idx, arr[k].src_idx, arr[k].n_corr = ti.ctypes.data, si.ctypes.data, len(ti)
        arr[k].clique_cap, arr[k].clique = 4, bufs[k].ctypes.data
    return arr, bufs


def test_refusals_reset_every_result_and_the_context_goes_on(ctx_auto, expected):
    L = lib.load()
    t, s = clouds("size_64")
    t3, s3 = clouds("three_pairs")
    good = (cloud_of(t), cloud_of(s), None, None)
    idx = np.arange(64, dtype=np.int32)
    bad_idx = idx.copy()
    bad_idx[10] = 64
    odd = np.zeros((64, 18), np.uint8)
    big = np.zeros((8193, 48), np.uint8)
    P = abi.teaser_params(0.2)
    cases = [((cloud_of(t), cloud_of(s), bad_idx, idx), abi.MULLS_E_INVALID), ((cloud_of(t), cloud_of(s), idx, bad_idx), abi.MULLS_E_INVALID),
             ((cloud_of(odd, 18), cloud_of(s), None, None), abi.MULLS_E_INVALID), ((cloud_of(big), cloud_of(big), None, None), abi.MULLS_E_UNSUPPORTED),
             ((cloud_of(t), cloud_of(s), idx, None), abi.MULLS_E_INVALID)]
    for bad, code in cases:
        specs = [good, (cloud_of(t3), cloud_of(s3), None, None), bad, good]
        if bad[2] is not None and bad[3] is None:  # one index list without the other
            arr, bufs = raw_problems([good, specs[1], (bad[0], bad[1], None, None), good])
            arr[2].tgt_idx, arr[2].n_corr = idx.ctypes.data, 64
        else:
            arr, bufs = raw_problems(specs)
        res = (abi.TeaserResult * 4)()
        for r in res:
            r.status, r.clique_size = 5, 9
        assert L.mulls_coarse_reg_teaser_batch(ctx_auto.h, arr, 4, C.byref(P), 0, res) == code
        assert b"problem 2" in L.mulls_last_error(ctx_auto.h)
        for r in res:
            assert r.status == -1 and r.clique_size == 0 and np.array_equal(np.array(r.T[:]).reshape(4, 4), np.eye(4))
        assert (bufs == -7).all()
    for nb in (float("nan"), float("inf"), -0.5):
        arr, bufs = raw_problems([good, good])
        res = (abi.TeaserResult * 2)()
        res[1].status = 5
        assert L.mulls_coarse_reg_teaser_batch(ctx_auto.h, arr, 2, C.byref(abi.teaser_params(nb)), 0, res) == abi.MULLS_E_INVALID
        assert res[0].status == -1 and res[1].status == -1 and (bufs == -7).all()
    # a batch whose only trouble is upstream's early returns runs: the good problems are solved, the others' clique buffers are untouched
    arr, bufs = raw_problems([good, (cloud_of(t3), cloud_of(s3), None, None), (cloud_of(t), cloud_of(s, n=63), None, None), good])
    res = (abi.TeaserResult * 4)()
    assert L.mulls_coarse_reg_teaser_batch(ctx_auto.h, arr, 4, C.byref(P), 0, res) == abi.MULLS_OK
    want = fixture_case("size_64")
    for k in (0, 3):
        assert res[k].status == want["status"] and np.array_equal(bufs[k, :4], want["clique"][:4]) and (bufs[k, 4:] == -7).all()
    for k in (1, 2):
        assert res[k].status == -1 and res[k].clique_size == 0 and (bufs[k] == -7).all()
    (got,) = run_batch(ctx_auto, [(t, s)], 0.2)
    assert_same(got, want, "after refusals")


def test_the_same_batch_twice_and_a_small_one_after_a_large_one(ctx_auto, expected):
    """the grow-only scratch keeps nothing of the call before: the descriptor table, the stop words, the frozen marks and the weights are written anew"""
    names = ["exit_cost", "complete_300", "size_1025", "no_edge", "exit_mu", "size_33"]
    problems = [clouds(name) for name in names]
    a = run_batch(ctx_auto, problems, 0.2)
    small = run_batch(ctx_auto, [clouds("size_31"), clouds("exit_cost")], 0.2)
    b = run_batch(ctx_auto, problems, 0.2)
    check(a, names, 0.2, expected, "first")
    check(b, names, 0.2, expected, "second")
    check(small, ["size_31", "exit_cost"], 0.2, expected, "between")
    for x, y in zip(a, b):
        assert x["clique_nodes"] == y["clique_nodes"]
