"""GPU tests of mulls_coarse_reg_ransac_batch through mulls_amd/lib.py.  Every problem of a batch must come back with the BYTES of the matching single call
(mulls_coarse_reg_ransac, or mulls_coarse_reg_ransac_indexed when the problem carries index lists).  Every comparison is equality, 0 ulp; expectations
come from three sources:
  (a) tests/golden/ransac_cases.npz, where a case exists at the batch's noise_bound (tests/test_ransac.py keeps it equal to the restatement),
  (b) tests/ransac_restated.py's restate, computed here for small sets,
  (c) the single call on the same context: all 152 bytes of the result struct, and the inlier list.
The mixed batch runs at noise_bound 0.3 / max_iter_num 100: the smallest relative distance of any residual to its threshold there is 2.8e-3 (asserted below
against tests/test_ransac.py's guard of 1e-4), so the equality is not at the mercy of one rounding.

PCL is not available where these tests run: nothing here was compared with PCL itself."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ransac_restated as rr
from mulls_amd import abi, lib
from test_gpu_ransac import assert_same, cloud_of, fixture, strided
from test_ransac import GUARD, demo, fixture_case, input_sets

pytestmark = pytest.mark.gpu
MIX = ["half_3", "half_8", "half_64", "half_517", "noisy_64", "noisy_517", "sparse_517", "unrelated_300", "tiny_0", "tiny_2", "coincident_64", "collinear_200",
       "nan_src_517", "nan_tgt_517"]
MIX_BOUND, MIX_ITERS = 0.3, 100


def as_dict(res, inl):
    T = np.array(res.T[:], np.float64).reshape(4, 4).T.copy()
    return dict(status=res.status, iterations=res.iterations, best_iteration=res.best_iteration, refine_iterations=res.refine_iterations,
                n_inliers=res.n_inliers, inliers=inl.astype(np.int64), T=T, bytes=bytes(res))


@functools.lru_cache(maxsize=None)
def problem(name):
    """(tgt records, src records) of an input set"""
    t, s, _, _ = input_sets()[name]
    return rr.records(t), rr.records(s)


def run_batch(ctx, problems, P, limit=0):
    return [as_dict(r, inl) for r, inl in ctx.coarse_reg_ransac_batch(problems, P, limit)]


def run_single(ctx, prob, P):
    if not isinstance(prob, dict):
        prob = dict(zip(("tgt", "src", "tgt_idx", "src_idx"), prob))
    return as_dict(*ctx.coarse_reg_ransac(prob["tgt"], prob["src"], P, prob.get("cap"), prob.get("tgt_idx"), prob.get("src_idx")))


def assert_bytes(got, single, what):
    """(c): the result struct's bytes and the inlier list of the single call"""
    assert got["bytes"] == single["bytes"], (what, {k: (got[k], single[k]) for k in got if k not in ("bytes", "inliers", "T")})
    assert np.array_equal(got["inliers"], single["inliers"]), what


@functools.lru_cache(maxsize=None)
def mix_expected(refine):
    """(b): the restatement of every set of the mixed batch, computed once"""
    out = {}
    with np.errstate(all="ignore"):
        for name in MIX:
            t, s, _, _ = input_sets()[name]
            out[name] = rr.restate(t, s, MIX_BOUND, 8, MIX_ITERS, refine)
    return out


def check_mix(ctx, got, names, refine, what, singles=None):
    P = abi.ransac_params(MIX_BOUND, 8, MIX_ITERS, refine)
    Z = fixture()
    for g, name in zip(got, names):
        assert_same(g, mix_expected(refine)[name], (what, name, refine))
        if name.startswith("noisy_"):  # (a): the fixture has these sets at this bound
            assert_same(g, fixture_case(Z, rr.case_name(name, MIX_ITERS, refine), len(problem(name)[0])), (what, name, "fixture"))
        assert_bytes(g, singles[name] if singles else run_single(ctx, problem(name), P), (what, name, refine))


def test_the_mix_is_what_it_is_meant_to_be():
    """the outcomes the mixed batch is built for, by the restatement: refinements of 1, 2 and 4 rounds, failures, pass-through problems; and its margin"""
    r0, r1 = mix_expected(0), mix_expected(1)
    for name in ("half_8", "half_64", "half_517"):
        assert r1[name]["refine_iterations"] == 1 and r1[name]["iterations"] == 35
    assert r1["noisy_64"]["refine_iterations"] == 2 and r1["noisy_517"]["refine_iterations"] == 4 and r1["nan_tgt_517"]["refine_iterations"] == 1
    for name in ("half_3", "sparse_517", "unrelated_300"):
        assert r1[name]["refine_iterations"] == 1 and r1[name]["status"] == -1 and r1[name]["n_inliers"] == 0 and r1[name]["iterations"] == 101
    for name in ("tiny_0", "tiny_2", "coincident_64", "collinear_200", "nan_src_517"):
        for r in (r0[name], r1[name]):
            assert r["iterations"] == 0 and r["best_iteration"] == -1 and r["n_inliers"] == len(problem(name)[0])
    assert r0["unrelated_300"]["best_iteration"] >= 0 and r0["unrelated_300"]["n_inliers"] == 300  # fewer than three inliers: pass-through with a winner
    assert not any(r["oscillating"] for r in r1.values())
    margin = min(r["margin"] for rs in (r0, r1) for r in rs.values())
    assert 2.5e-3 < margin < 3e-3 and margin > 10 * GUARD


@pytest.mark.parametrize("refine", [0, 1])
def test_one_batch_mixes_every_outcome(ctx_auto, refine):
    """under refine = 1 the 2- and 4-round problems keep running after the others froze: their masks alternate while the frozen problems' must survive"""
    got = run_batch(ctx_auto, [problem(name) for name in MIX], abi.ransac_params(MIX_BOUND, 8, MIX_ITERS, refine))
    check_mix(ctx_auto, got, MIX, refine, "mix")


@pytest.mark.parametrize("refine", [0, 1])
def test_order_and_cuts_change_nothing(ctx_auto, refine):
    P = abi.ransac_params(MIX_BOUND, 8, MIX_ITERS, refine)
    singles = {name: run_single(ctx_auto, problem(name), P) for name in MIX}
    problems = [problem(name) for name in MIX]
    check_mix(ctx_auto, run_batch(ctx_auto, problems[::-1], P), MIX[::-1], refine, "reversed", singles)
    check_mix(ctx_auto, run_batch(ctx_auto, problems, P, 1), MIX, refine, "one problem per sub-batch", singles)
    # a limit that cuts the list in two: what the first seven running problems need (the planner's sum: tests/test_ransac_batch.py)
    def up(v):
        return -(-v // 256) * 256

    def need(n):
        return 2 * up(16 * n) + up(8 * n) + up(12 * 101) + up(48 * 101) + up(4 * 101) + 3 * up(n) + up(4 * n) + 256 + 512

    running = [len(problem(name)[0]) for name in MIX if len(problem(name)[0]) >= 3]
    assert len(running) == 12
    check_mix(ctx_auto, run_batch(ctx_auto, problems, P, sum(need(n) for n in running[:7])), MIX, refine, "two sub-batches", singles)


@pytest.mark.parametrize("refine", [0, 1])
def test_fixture_cases_large_beside_small(ctx_auto, refine):
    """bound 0.5: a problem of 65536 pairs beside small ones (offsets past 2^16 pairs), n_hyp = 101 (101 mod 16 = 5) and max_iter_num = 1 (n_hyp = 2)"""
    Z = fixture()
    for names, iters in ((["half_65536", "half_64", "sparse_517", "half_4097"], 100), (["half_65536", "half_64", "half_3", "half_4097"], 1)):
        got = run_batch(ctx_auto, [problem(name) for name in names], abi.ransac_params(0.5, 8, iters, refine))
        for g, name in zip(got, names):
            assert_same(g, fixture_case(Z, rr.case_name(name, iters, refine), len(problem(name)[0])), (name, iters, refine))


def test_full_hypothesis_list(ctx_auto):
    """max_iter_num 20000: sparse_517 runs all 20 001 hypotheses, half_2840 stops within tens, in one batch"""
    Z = fixture()
    names = ["sparse_517", "half_2840"]
    for refine in (0, 1):
        P = abi.ransac_params(0.5, 8, 20000, refine)
        got = run_batch(ctx_auto, [problem(name) for name in names], P)
        for g, name in zip(got, names):
            assert_same(g, fixture_case(Z, rr.case_name(name, 20000, refine), len(problem(name)[0])), (name, refine))
            assert_bytes(g, run_single(ctx_auto, problem(name), P), (name, refine))
        assert got[0]["iterations"] == 20001 and got[1]["iterations"] < 100


def test_indexed_and_plain_problems_mixed(ctx_auto):
    Z, D = fixture(), demo()
    kt, ks = D["kpts_0"], D["kpts_15"]
    for iters, refine in ((100, 1), (100, 0)):
        P = abi.ransac_params(1.0, 8, iters, refine)
        problems, wants = [], []
        for name in rr.DEMO_LISTS:
            pr = D[name + "_pairs"]
            want = fixture_case(Z, rr.case_name("demo_" + name, iters, refine), len(pr))
            problems += [dict(tgt=kt, src=ks, tgt_idx=pr[:, 0], src_idx=pr[:, 1]), (kt[pr[:, 0]], ks[pr[:, 1]])]  # indexed, and the same list pre-gathered
            wants += [want, want]
        pr = D["recip_0_15_pairs"][:2]  # fewer than three pairs: pass-through
        problems.append(dict(tgt=kt, src=ks, tgt_idx=pr[:, 0], src_idx=pr[:, 1]))
        got = run_batch(ctx_auto, problems, P)
        for k, (g, want) in enumerate(zip(got, wants)):
            assert_same(g, want, (k, iters, refine))
            assert_bytes(g, run_single(ctx_auto, problems[k], P), (k, iters, refine))
        last = got[-1]
        assert last["status"] == -1 and last["n_inliers"] == 2 and last["best_iteration"] == -1 and np.array_equal(last["inliers"], [0, 1])
        assert_bytes(last, run_single(ctx_auto, problems[-1], P), "two pairs")


# torch brings a HIP runtime of its own: a process takes one of the two, the one loaded first, so the tensors live in a child that imports torch first
TORCH_CHILD = r"""
import ctypes as C, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
torch.cuda.init()
assert torch.zeros(4, device="cuda:0").sum().item() == 0
import ransac_restated as rr
from mulls_amd import abi, lib
from test_ransac import FIXTURE, demo, fixture_case, input_sets
from test_gpu_ransac import assert_same, strided
from test_gpu_ransac_batch import assert_bytes, run_batch, run_single
Z = np.load(FIXTURE, allow_pickle=False)
ctx = lib.Context(0)
def cloud(x, n, stride=48):
    c = abi.Cloud()
    c.pts, c.n, c.stride = x.data_ptr(), n, stride
    return c
keep, problems, wants = [], [], []
for name in ("noisy_517", "noisy_64"):
    t, s, bound, _ = input_sets()[name]
    rt, rs = rr.records(t), rr.records(s)
    dev = {k: torch.from_numpy(raw.copy()).to("cuda:0") for k, raw in (("t", rt), ("s", rs))}
    pin = {k: torch.from_numpy(raw.copy()).pin_memory() for k, raw in (("t", rt), ("s", rs))}
    keep += [dev, pin]
    D = {k: cloud(x, len(x)) for k, x in dev.items()}
    H = {k: cloud(x, len(x)) for k, x in pin.items()}
    here = [(D["t"], rs), (rt, D["s"]), (H["t"], H["s"]), (D["t"], D["s"]), (H["t"], D["s"])]
    for stride in (16, 64):
        bt, ct = strided(rt, stride, stride)
        bs, cs = strided(rs, stride, stride + 1)
        keep += [bt, bs]
        here.append((ct, cs))
    problems += here
    wants += [name] * len(here)
torch.cuda.synchronize()
for rf in (0, 1):
    P = abi.ransac_params(0.3, 8, 100, rf)
    got = run_batch(ctx, problems, P)
    for g, name, prob in zip(got, wants, problems):
        assert_same(g, fixture_case(Z, rr.case_name(name, 100, rf), len(input_sets()[name][0])), (name, rf))
        assert_bytes(g, run_single(ctx, prob, P), (name, rf))
# no device-resident source: the same results (the path without the staging wait)
P = abi.ransac_params(0.3, 8, 100, 1)
for g, name in zip(run_batch(ctx, [p for p in problems if p[1] is not None and not isinstance(p[1], abi.Cloud)], P), ("noisy_517", "noisy_64")):
    assert_same(g, fixture_case(Z, rr.case_name(name, 100, 1), len(input_sets()[name][0])), name)
# indexed problems on device-resident key points, on either side
D0 = demo()
kt, ks = D0["kpts_0"], D0["kpts_15"]
dkt, dks = torch.from_numpy(kt.copy()).to("cuda:0"), torch.from_numpy(ks.copy()).to("cuda:0")
torch.cuda.synchronize()
P = abi.ransac_params(1.0, 8, 100, 1)
problems, wants = [], []
for name in rr.DEMO_LISTS:
    pr = D0[name + "_pairs"]
    for a, b in ((cloud(dkt, len(kt)), cloud(dks, len(ks))), (cloud(dkt, len(kt)), ks), (kt, cloud(dks, len(ks)))):
        problems.append(dict(tgt=a, src=b, tgt_idx=pr[:, 0], src_idx=pr[:, 1]))
        wants.append(fixture_case(Z, rr.case_name("demo_" + name, 100, 1), len(pr)))
for g, want, prob in zip(run_batch(ctx, problems, P), wants, problems):
    assert_same(g, want, "indexed")
    assert_bytes(g, run_single(ctx, prob, P), "indexed")
# a device cloud whose stride is not 48: refused, and the message names the problem
wide = torch.zeros((517, 64), dtype=torch.uint8, device="cuda:0")
torch.cuda.synchronize()
t, s, bound, _ = input_sets()["noisy_517"]
rt, rs = rr.records(t), rr.records(s)
good = cloud(torch.from_numpy(rs).to("cuda:0"), 517)
for where, bad in ((0, (cloud(wide, 517, 64), good)), (2, (good, cloud(wide, 517, 64)))):
    probs = [(rt, rs)] * 3
    probs[where] = bad
    try:
        ctx.coarse_reg_ransac_batch(probs, abi.ransac_params(0.3, 8, 100, 1))
        raise SystemExit("a device cloud of stride 64 was accepted")
    except lib.MullsError as e:
        assert e.args[1] == abi.MULLS_E_INVALID and ("problem %%d:" %% where) in e.args[0] and "stride" in e.args[0], e.args
(g,) = run_batch(ctx, [(rt, rs)], abi.ransac_params(0.3, 8, 100, 1))
assert_same(g, fixture_case(Z, "noisy_517_i100_r1", 517), "after the refusal")
ctx.close()
print("torch clouds ok")
"""


def test_clouds_homes_mixed_in_one_batch():
    """device-resident targets with host sources, host targets with device-resident sources, pinned clouds on both sides, host strides 16 and 64, in one
    batch; indexed problems on device-resident key points; a device cloud of stride 64 is refused with the problem's index"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", TORCH_CHILD % (root, os.path.join(root, "tests"))], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "torch clouds ok" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


def raw_problems(specs):
    """mulls_ransac_problem records by hand: (tgt cloud, src cloud, tgt_idx, src_idx) and an inlier buffer of four slots in eight, filled with -7, for each"""
    arr = (abi.RansacProblem * len(specs))()
    bufs = np.full((len(specs), 8), -7, np.int32)
    for k, (ct, cs, ti, si) in enumerate(specs):
        arr[k].tgt, arr[k].src = ct, cs
        if ti is not None:
            arr[k].tgt_idx, arr[k].n_corr = ti.ctypes.data, len(ti)
        if si is not None:
            arr[k].src_idx, arr[k].n_corr = si.ctypes.data, len(si)
        arr[k].inlier_cap, arr[k].inliers = 4, bufs[k].ctypes.data
    return arr, bufs


def test_refusals_reset_every_result_and_the_context_goes_on(ctx_auto):
    L = lib.load()
    t, s = problem("half_517")
    t2, s2 = problem("tiny_2")
    good, few = (cloud_of(t), cloud_of(s), None, None), (cloud_of(t2), cloud_of(s2), None, None)
    idx = np.arange(517, dtype=np.int32)
    bad_idx = idx.copy()
    bad_idx[100] = 517  # an index equal to n
    odd = np.zeros((517, 18), np.uint8)
    big = np.zeros((65537, 48), np.uint8)
    P = abi.ransac_params(MIX_BOUND, 8, MIX_ITERS, 1)
    cases = [((cloud_of(t), cloud_of(s, n=516), None, None), abi.MULLS_E_INVALID),  # unequal sizes
             ((cloud_of(t), cloud_of(s), bad_idx, idx), abi.MULLS_E_INVALID), ((cloud_of(t), cloud_of(s), idx, bad_idx), abi.MULLS_E_INVALID),
             ((cloud_of(t), cloud_of(s), idx, None), abi.MULLS_E_INVALID), ((cloud_of(t), cloud_of(s), None, idx), abi.MULLS_E_INVALID),  # one list without the other
             ((cloud_of(odd, 18), cloud_of(s), None, None), abi.MULLS_E_INVALID), ((cloud_of(t), cloud_of(odd, 18), None, None), abi.MULLS_E_INVALID),
             ((cloud_of(big), cloud_of(big), None, None), abi.MULLS_E_UNSUPPORTED)]

    def refused(arr, bufs, n, params, code, where):
        res = (abi.RansacResult * n)()
        for r in res:
            r.status, r.n_inliers, r.best_iteration = 5, 9, 3
        assert L.mulls_coarse_reg_ransac_batch(ctx_auto.h, arr, n, C.byref(params), 0, res) == code
        assert (b"mulls_coarse_reg_ransac_batch: problem %d:" % where) in L.mulls_last_error(ctx_auto.h), L.mulls_last_error(ctx_auto.h)
        for r in res:
            assert r.status == -1 and r.best_iteration == -1 and r.n_inliers == 0 and r.iterations == 0 and r.refine_iterations == 0
            assert np.array_equal(np.array(r.T[:]).reshape(4, 4), np.eye(4))
        assert (bufs == -7).all()

    for bad, code in cases:
        for where in (0, 2, 4):  # first, in the middle, last; a pass-through problem in front of it stays unwritten too
            specs = [good, few, good, good, good]
            specs[where] = bad
            arr, bufs = raw_problems(specs)
            refused(arr, bufs, 5, P, code, where)
    # the parameters refuse every problem: the first is named
    for params, code in ((abi.ransac_params(MIX_BOUND, 8, (1 << 20) + 1, 1), abi.MULLS_E_UNSUPPORTED), (abi.ransac_params(float("nan"), 8, 100, 1), abi.MULLS_E_INVALID),
                         (abi.ransac_params(float("inf"), 8, 100, 1), abi.MULLS_E_INVALID), (abi.ransac_params(float("-inf"), 8, 100, 1), abi.MULLS_E_INVALID)):
        arr, bufs = raw_problems([few, good, good])
        refused(arr, bufs, 3, params, code, 0)
    # the single calls' codes for the same offences (their messages carry no index)
    res = abi.RansacResult()
    for bad, code in cases:
        ct, cs, ti, si = bad
        if ti is None and si is None:
            rc = L.mulls_coarse_reg_ransac(ctx_auto.h, C.byref(ct), C.byref(cs), C.byref(P), C.byref(res), None, 0)
        else:
            rc = L.mulls_coarse_reg_ransac_indexed(ctx_auto.h, C.byref(ct), C.byref(cs), None if ti is None else ti.ctypes.data_as(C.c_void_p),
                                                   None if si is None else si.ctypes.data_as(C.c_void_p), 517, C.byref(P), C.byref(res), None, 0)
        assert rc == code
    # NULLs the call itself needs
    arr, bufs = raw_problems([good])
    assert L.mulls_coarse_reg_ransac_batch(ctx_auto.h, None, 1, C.byref(P), 0, (abi.RansacResult * 1)()) == abi.MULLS_E_INVALID
    assert L.mulls_coarse_reg_ransac_batch(ctx_auto.h, arr, 1, C.byref(P), 0, None) == abi.MULLS_E_INVALID
    assert L.mulls_coarse_reg_ransac_batch(ctx_auto.h, arr, 1, None, 0, (abi.RansacResult * 1)()) == abi.MULLS_E_INVALID
    arr[0].inliers = None  # a buffer the problem needs
    refused(arr, bufs, 1, P, abi.MULLS_E_INVALID, 0)
    # and the context goes on: the mixed batch
    got = run_batch(ctx_auto, [problem(name) for name in MIX], P)
    check_mix(ctx_auto, got, MIX, 1, "after refusals")


def test_caps_within_one_batch(ctx_auto):
    """inlier_cap 0, 1, n_inliers and n_inliers + 5 per problem (lib.py checks that the slot behind every cap is left alone)"""
    P = abi.ransac_params(MIX_BOUND, 8, MIX_ITERS, 1)
    problems, wants, caps = [], [], []
    for name in ("noisy_517", "half_64", "nan_tgt_517", "coincident_64"):  # (the last passes through: 64 inliers 0 .. 63)
        want = mix_expected(1)[name]
        assert want["n_inliers"] > 5
        for cap in (0, 1, want["n_inliers"], want["n_inliers"] + 5):
            t, s = problem(name)
            problems.append(dict(tgt=t, src=s, cap=cap))
            wants.append(want)
            caps.append(cap)
    got = run_batch(ctx_auto, problems, P)
    for k, (g, want, cap) in enumerate(zip(got, wants, caps)):
        assert_same(g, want, (k, cap), inliers=False)
        assert np.array_equal(g["inliers"], want["inliers"][:cap]), (k, cap)
        assert_bytes(g, run_single(ctx_auto, problems[k], P), (k, cap))


def test_batch_single_batch_single_then_a_larger_batch():
    """one context of its own: the grow-only scratch, shared by the single calls and the batch, keeps nothing between them"""
    ctx = lib.Context(0)
    try:
        Z = fixture()
        P = abi.ransac_params(MIX_BOUND, 8, MIX_ITERS, 1)
        small = ["noisy_64", "half_8", "sparse_517"]
        check_mix(ctx, run_batch(ctx, [problem(n) for n in small], P), small, 1, "first batch")
        t, s, bound, _ = input_sets()["noisy_517"]
        want = fixture_case(Z, "noisy_517_i20000_r1", 517)
        assert_same(run_single(ctx, problem("noisy_517"), abi.ransac_params(bound, 8, 20000, 1)), want, "single after a batch")
        check_mix(ctx, run_batch(ctx, [problem(n) for n in small[::-1]], P), small[::-1], 1, "second batch")
        assert_same(run_single(ctx, problem("noisy_517"), abi.ransac_params(bound, 8, 20000, 1)), want, "single after the second batch")
        check_mix(ctx, run_batch(ctx, [problem(n) for n in MIX + MIX[::-1]], P), MIX + MIX[::-1], 1, "a larger batch")
    finally:
        ctx.close()


def test_empty_and_all_pass_through(ctx_auto):
    assert ctx_auto.coarse_reg_ransac_batch([]) == []  # n_problems = 0: MULLS_OK
    assert lib.load().mulls_coarse_reg_ransac_batch(ctx_auto.h, None, 0, C.byref(abi.ransac_params()), 0, None) == abi.MULLS_OK
    names = ["tiny_0", "tiny_2", "coincident_64"]
    for refine in (0, 1):
        got = run_batch(ctx_auto, [problem(n) for n in names], abi.ransac_params(MIX_BOUND, 8, MIX_ITERS, refine))
        check_mix(ctx_auto, got, names, refine, "all pass-through")
        for g, n in zip(got, names):
            assert g["best_iteration"] == -1 and g["iterations"] == 0 and np.array_equal(g["inliers"], np.arange(len(problem(n)[0]))) and np.array_equal(g["T"], np.eye(4))
