"""GPU tests of mulls_coarse_reg_ransac / mulls_coarse_reg_ransac_indexed (coarse_reg_ransac, include/common/cregistration.hpp:605-661) through mulls_amd/lib.py,
against the numpy restatement of the library's definition (tests/ransac_restated.py) as tests/golden/ransac_cases.npz pins it (tests/test_ransac.py keeps the
two equal, and asserts that no residual of a winning or refined model lies within a relative 1e-4 of its threshold on any of these sets).

Every comparison is equality: status, iterations, best_iteration, refine_iterations, n_inliers, the inlier list — and the transform, in both modes.

Tolerance on T.  Without refinement T is the float matrix of the winning hypothesis: float and double expressions in a fixed order, no contraction, every
operation (+ - * / sqrt) correctly rounded on the device as in numpy: 0 ulp.  With refinement the centroids and H are double sums over up to 65 536 terms.  A
sum whose ORDER were free would differ between two evaluations by up to about n * 2^-53 relative to the sum of the magnitudes — after the decomposition and
the rounding to float (2^-24) that is at most 1 float ulp of an entry's magnitude, and only for entries whose double value sits within that distance of a float
rounding boundary.  The library does not leave the order free: it defines it (256 strided partial sums in ascending index, then a pairwise tree), the
restatement adds in that order, so the two double sums are the same bits and the allowance is 0 ulp here as well.  ULPS below states it.

PCL is not available where these tests run: nothing here was compared with PCL itself."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ransac_restated as rr
from mulls_amd import abi, lib, synth
from test_ransac import FIXTURE, demo, fixture_case, input_sets

pytestmark = pytest.mark.gpu
ULPS = 0  # see the module docstring
INT_FIELDS = ("status", "iterations", "best_iteration", "refine_iterations", "n_inliers")


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(FIXTURE, allow_pickle=False)


def device(ctx, t, s, bound, max_iter, refine, min_inlier=8, cap=None, **kw):
    res, inl = ctx.coarse_reg_ransac(rr.records(t) if isinstance(t, np.ndarray) and t.shape[1:] == (4,) else t,
                                     rr.records(s) if isinstance(s, np.ndarray) and s.shape[1:] == (4,) else s,
                                     abi.ransac_params(bound, min_inlier, max_iter, refine), cap, **kw)
    T = np.array(res.T[:], np.float64).reshape(4, 4).T.copy()
    return dict(status=res.status, iterations=res.iterations, best_iteration=res.best_iteration, refine_iterations=res.refine_iterations,
                n_inliers=res.n_inliers, inliers=inl.astype(np.int64), T=T)


def assert_same(got, want, what, inliers=True):
    for k in INT_FIELDS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    if inliers:
        assert np.array_equal(got["inliers"], want["inliers"]), what
    a, b = got["T"].astype(np.float32), np.asarray(want["T"]).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), got["T"])  # upstream's Matrix4f cast to double
    if ULPS == 0:
        assert np.array_equal(a, b), (what, np.abs(a - b).max())
    else:
        assert (np.abs(a - b) <= ULPS * np.spacing(np.maximum(np.abs(a), np.abs(b)))).all(), what


@pytest.mark.parametrize("name", sorted(rr.input_sets(None)) + ["demo_" + n for n in rr.DEMO_LISTS])
def test_device_equals_restatement(ctx_auto, name):
    """the synthetic families at N in {3, 8, 64, 517, 2840, 4097, 65536} x max_iter_num in {1, 100, 20000}, the edge families and the four demo pair lists,
    each with and without refinement"""
    t, s, bound, iters = input_sets()[name]
    Z = fixture()
    for it in iters:
        for rf in (0, 1):
            case = rr.case_name(name, it, rf)
            assert_same(device(ctx_auto, t, s, bound, it, rf), fixture_case(Z, case, len(t)), case)


def test_early_stop_and_full_run(ctx_auto):
    t, s, bound, _ = input_sets()["half_2840"]
    assert device(ctx_auto, t, s, bound, 20000, 1)["iterations"] < 100
    t, s, bound, _ = input_sets()["sparse_517"]
    assert device(ctx_auto, t, s, bound, 20000, 1)["iterations"] == 20001


def test_pass_through_and_failed_refinement(ctx_auto):
    for name in ("tiny_0", "tiny_1", "tiny_2", "coincident_64", "collinear_200", "nan_src_517"):
        t, s, bound, _ = input_sets()[name]
        for min_in, status in ((8, 1 if len(t) >= 16 else (0 if len(t) >= 8 else -1)), (40, 1 if len(t) >= 80 else (0 if len(t) >= 40 else -1))):
            r = device(ctx_auto, t, s, bound, 100, 1, min_inlier=min_in)
            assert r["status"] == status and r["best_iteration"] == -1 and r["n_inliers"] == len(t), name
            assert np.array_equal(r["inliers"], np.arange(len(t))) and np.array_equal(r["T"], np.eye(4)), name
    t, s, bound, _ = input_sets()["unrelated_300"]
    r = device(ctx_auto, t, s, bound, 100, 0)  # fewer than three inliers: everything passes, identity, but there was a winner
    assert r["best_iteration"] >= 0 and r["n_inliers"] == 300 and r["status"] == 1 and np.array_equal(r["T"], np.eye(4))
    r = device(ctx_auto, t, s, bound, 100, 1)  # the refinement selects nothing
    assert r["status"] == -1 and r["n_inliers"] == 0 and len(r["inliers"]) == 0 and np.array_equal(r["T"], np.eye(4))


def cloud_of(raw, stride=48, n=None):
    c = abi.Cloud()
    c.pts, c.n, c.stride = raw.ctypes.data, len(raw) if n is None else n, stride
    return c


def test_refusals(ctx_auto):
    L = lib.load()
    t, s, bound, _ = input_sets()["half_517"]
    rt, rs = rr.records(t), rr.records(s)
    res, inl = abi.RansacResult(), np.full(8, -7, np.int32)
    ip = inl.ctypes.data_as(C.c_void_p)

    def call(ct, cs, P):
        return L.mulls_coarse_reg_ransac(ctx_auto.h, C.byref(ct), C.byref(cs), C.byref(P), C.byref(res), ip, 4)

    good = abi.ransac_params(bound, 8, 100, 1)
    assert call(cloud_of(rt), cloud_of(rs, n=516), good) == abi.MULLS_E_INVALID  # unequal sizes
    for nb in (float("nan"), float("inf"), float("-inf")):
        assert call(cloud_of(rt), cloud_of(rs), abi.ransac_params(nb, 8, 100, 1)) == abi.MULLS_E_INVALID
    assert call(cloud_of(rt), cloud_of(rs), abi.ransac_params(bound, 8, (1 << 20) + 1, 1)) == abi.MULLS_E_UNSUPPORTED
    big = np.zeros((65537, 48), np.uint8)
    assert call(cloud_of(big), cloud_of(big), good) == abi.MULLS_E_UNSUPPORTED
    for stride in (12, 18, 50):
        buf = np.zeros((517, stride), np.uint8)
        assert call(cloud_of(buf, stride), cloud_of(rs), good) == abi.MULLS_E_INVALID
        assert call(cloud_of(rt), cloud_of(buf, stride), good) == abi.MULLS_E_INVALID
    assert L.mulls_coarse_reg_ransac(None, None, None, None, None, None, 0) == abi.MULLS_E_INVALID
    assert (inl == -7).all()
    # an index outside its cloud
    idx = np.arange(517, dtype=np.int32)
    bad = idx.copy()
    bad[100] = 517
    for a, b in ((bad, idx), (idx, bad)):
        rc = L.mulls_coarse_reg_ransac_indexed(ctx_auto.h, C.byref(cloud_of(rt)), C.byref(cloud_of(rs)), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), 517,
                                               C.byref(good), C.byref(res), ip, 4)
        assert rc == abi.MULLS_E_INVALID
    want = fixture_case(fixture(), "half_517_i100_r1", 517)  # and the context goes on
    assert_same(device(ctx_auto, t, s, bound, 100, 1), want, "after refusals")


def test_single_entry_points_at_their_own_edges(ctx_auto):
    """what only the single entry points define: the pass-through below three pairs (before the stride check, the indexed call with no pairs and NULL lists
    among them), the refusals without a message (a NULL cloud, one index list without the other) next to a NULL result and a capacity without a buffer, the
    order of two refusals — and the message of every refusal that sets one names the entry point that was called"""
    L = lib.load()
    t, s, bound, _ = input_sets()["half_517"]
    rt, rs = rr.records(t), rr.records(s)
    ct, cs = cloud_of(rt), cloud_of(rs)
    good = abi.ransac_params(bound, 8, 100, 1)
    res, inl = abi.RansacResult(), np.full(8, -7, np.int32)
    ip = inl.ctypes.data_as(C.c_void_p)
    idx = np.arange(517, dtype=np.int32)
    eye = np.eye(4)

    def vp(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def plain(a, b, P=good, result=res, inliers=ip, cap=4):
        return L.mulls_coarse_reg_ransac(ctx_auto.h, C.byref(a), C.byref(b), C.byref(P), result, inliers, cap)

    def indexed(ti, si, n, a=ct, b=cs, P=good, result=res, inliers=ip, cap=4):
        return L.mulls_coarse_reg_ransac_indexed(ctx_auto.h, C.byref(a), C.byref(b), vp(ti), vp(si), n, C.byref(P), result, inliers, cap)

    def T():
        return np.array(res.T[:]).reshape(4, 4)

    # the pass-through below three pairs
    res.status, res.n_inliers = 5, 9
    assert indexed(None, None, 0) == abi.MULLS_OK
    assert res.status == -1 and res.n_inliers == 0 and res.best_iteration == -1 and np.array_equal(T(), eye) and (inl == -7).all()
    for call in (lambda: indexed(idx, idx, 2, cap=1), lambda: plain(cloud_of(rt, n=2), cloud_of(rs, n=2), cap=1)):
        inl[:] = -7
        res.status, res.n_inliers = 5, 9
        assert call() == abi.MULLS_OK
        assert res.status == -1 and res.n_inliers == 2 and res.best_iteration == -1 and np.array_equal(T(), eye)
        assert inl[0] == 0 and (inl[1:] == -7).all()  # one slot was offered
    inl[:] = -7
    odd = np.zeros((517, 18), np.uint8)
    for n in (0, 1, 2):  # ... comes before the stride check
        assert plain(cloud_of(odd, 18, n=n), cloud_of(rs, n=n), cap=0) == abi.MULLS_OK and res.n_inliers == n
        assert indexed(idx, idx, n, a=cloud_of(odd, 18), cap=0) == abi.MULLS_OK and res.n_inliers == n

    def said(who):
        msg = L.mulls_last_error(ctx_auto.h) or b""
        assert msg.startswith(who + b":") and b"problem" not in msg, msg

    big, many, bad = np.zeros((65537, 48), np.uint8), np.zeros(65537, np.int32), idx.copy()
    bad[100] = 517
    inf, long_run = abi.ransac_params(float("inf"), 8, 100, 1), abi.ransac_params(bound, 8, (1 << 20) + 1, 1)
    one, two = b"mulls_coarse_reg_ransac", b"mulls_coarse_reg_ransac_indexed"
    for refuse, who, code in ((lambda: plain(ct, cs, P=inf), one, abi.MULLS_E_INVALID),
                              (lambda: plain(ct, cloud_of(rs, n=516)), one, abi.MULLS_E_INVALID),
                              (lambda: plain(cloud_of(big), cloud_of(big)), one, abi.MULLS_E_UNSUPPORTED),
                              (lambda: plain(ct, cs, P=long_run), one, abi.MULLS_E_UNSUPPORTED),
                              (lambda: plain(cloud_of(odd, 18), cs), one, abi.MULLS_E_INVALID),
                              (lambda: plain(ct, cloud_of(odd, 18)), one, abi.MULLS_E_INVALID),
                              (lambda: indexed(idx, idx, 517, P=inf), two, abi.MULLS_E_INVALID),
                              (lambda: indexed(many, many, 65537), two, abi.MULLS_E_UNSUPPORTED),
                              (lambda: indexed(idx, idx, 517, P=long_run), two, abi.MULLS_E_UNSUPPORTED),
                              (lambda: indexed(idx, idx, 517, a=cloud_of(odd, 18)), two, abi.MULLS_E_INVALID),
                              (lambda: indexed(bad, idx, 517), two, abi.MULLS_E_INVALID),
                              (lambda: indexed(idx, bad, 517), two, abi.MULLS_E_INVALID)):
        res.status, res.best_iteration, res.T[3] = 5, 7, 2.0
        assert refuse() == code
        said(who)
        assert res.status == -1 and res.best_iteration == -1 and np.array_equal(T(), eye) and (inl == -7).all()

    # the refusals without a message leave the last one standing
    assert plain(ct, cs, P=inf) == abi.MULLS_E_INVALID
    before = L.mulls_last_error(ctx_auto.h)
    said(one)
    gone = abi.Cloud()
    gone.pts, gone.n, gone.stride = None, 517, 48
    for quiet in (lambda: plain(gone, cs), lambda: plain(ct, gone), lambda: indexed(idx, idx, 517, a=gone), lambda: indexed(idx, None, 517),
                  lambda: indexed(None, idx, 517)):
        res.status = 5
        assert quiet() == abi.MULLS_E_INVALID
        assert L.mulls_last_error(ctx_auto.h) == before and res.status == -1 and (inl == -7).all()
    assert plain(ct, cs, result=None) == abi.MULLS_E_INVALID and indexed(idx, idx, 517, result=None) == abi.MULLS_E_INVALID
    assert plain(ct, cs, inliers=None) == abi.MULLS_E_INVALID and indexed(idx, idx, 517, inliers=None) == abi.MULLS_E_INVALID
    assert L.mulls_last_error(ctx_auto.h) == before

    # of two refusals the earlier one of the checks wins: unequal sizes come before too many iterations
    assert plain(ct, cloud_of(rs, n=516), P=long_run) == abi.MULLS_E_INVALID
    said(one)
    want = fixture_case(fixture(), "half_517_i100_r1", 517)  # and the context goes on
    assert_same(device(ctx_auto, t, s, bound, 100, 1), want, "after refusals")
    assert_same(device(ctx_auto, t, s, bound, 100, 1, tgt_idx=idx, src_idx=idx), want, "after refusals, indexed")


def strided(raw, stride, seed):
    n, w = len(raw), min(stride, 48)
    buf = np.random.default_rng(seed).integers(0, 256, (n, stride), dtype=np.uint8)
    buf[:, :w] = raw[:, :w]
    return buf, cloud_of(buf, stride)


def test_host_strides_and_cap(ctx_auto):
    t, s, bound, _ = input_sets()["noisy_517"]
    want = fixture_case(fixture(), "noisy_517_i20000_r1", 517)
    rt, rs = rr.records(t), rr.records(s)
    for stride in (16, 20, 36, 64):
        bt, ct = strided(rt, stride, stride)
        bs, cs = strided(rs, stride, stride + 1)
        for a, b in ((ct, cs), (ct, rs), (rt, cs)):
            assert_same(device(ctx_auto, a, b, bound, 20000, 1), want, stride)
    assert want["n_inliers"] > 20
    for cap in (0, 1, 20, want["n_inliers"], want["n_inliers"] + 5):
        got = device(ctx_auto, t, s, bound, 20000, 1, cap=cap)  # (lib.py checks that the slot behind cap is left alone)
        assert_same(got, want, cap, inliers=False)
        assert np.array_equal(got["inliers"], want["inliers"][:cap])


def test_indexed_equals_gathered(ctx_auto):
    Z = demo()
    kt, ks = Z["kpts_0"], Z["kpts_15"]
    for name in rr.DEMO_LISTS:
        pr = Z[name + "_pairs"]
        for it, rf in ((100, 1), (20000, 0)):
            want = fixture_case(fixture(), rr.case_name("demo_" + name, it, rf), len(pr))
            got = device(ctx_auto, kt, ks, 1.0, it, rf, tgt_idx=pr[:, 0], src_idx=pr[:, 1])
            assert_same(got, want, (name, it, rf))
            assert_same(device(ctx_auto, kt[pr[:, 0]], ks[pr[:, 1]], 1.0, it, rf), want, (name, it, rf, "gathered"))
    pr = Z["recip_0_15_pairs"][:2]  # fewer than three pairs
    got = device(ctx_auto, kt, ks, 1.0, 100, 1, tgt_idx=pr[:, 0], src_idx=pr[:, 1])
    assert got["n_inliers"] == 2 and got["status"] == -1 and got["best_iteration"] == -1


def test_two_calls_in_a_row_and_scratch_growth(ctx_auto):
    """one context: a small set, the largest, the small one again, each twice — the grow-only scratch keeps nothing of the call before"""
    Z = fixture()
    order = ["noisy_64", "half_65536", "noisy_64", "sparse_517", "noisy_4097", "noisy_64"]
    for name in order:
        t, s, bound, iters = input_sets()[name]
        want = fixture_case(Z, rr.case_name(name, max(iters), 1), len(t))
        a, b = device(ctx_auto, t, s, bound, max(iters), 1), device(ctx_auto, t, s, bound, max(iters), 1)
        assert_same(a, want, name)
        assert_same(b, want, name)
        assert a["T"].tobytes() == b["T"].tobytes()


def planted_key_point_pair(seed):
    """A synthetic scan pair 4 m and 20 degrees apart, and key points with NCC-style index lists: 40 % of the listed pairs are the same physical point seen from
    the two poses (5 cm of noise), the rest are unrelated."""
    src_c = {abi.GROUND: 600, abi.PILLAR: 300, abi.FACADE: 700, abi.BEAM: 150, abi.ROOF: 80}
    tgt_c = {abi.GROUND: 2500, abi.PILLAR: 900, abi.FACADE: 3000, abi.BEAM: 400, abi.ROOF: 300}
    motion = synth.se3(4.0, 1.0, 0.0, 0, 0, np.deg2rad(20))
    pair, T_gt = synth.make_pair(seed, n_beams=32, n_az=900, src_counts=src_c, tgt_counts=tgt_c, vertex_count=200, motion=motion)
    rng = np.random.default_rng(seed)
    tgt_kp = abi.records(pair.tgt[5]).copy()
    n = len(tgt_kp)
    xyz = rr.xyzw_of(tgt_kp)[:, :3].astype(np.float64)
    inv = np.linalg.inv(T_gt)
    moved = xyz @ inv[:3, :3].T + inv[:3, 3] + rng.normal(0, 0.05, (n, 3))
    good = rng.random(n) < 0.4
    moved[~good] = rng.uniform([-40, -40, -2], [40, 40, 8], (int((~good).sum()), 3))
    order = rng.permutation(n)  # the source key points are stored in another order than the target's
    src_xyzw = np.concatenate([moved, rng.uniform(0, 5, (n, 1))], 1).astype(np.float32)[order]
    src_kp = rr.records(src_xyzw)
    tgt_idx = rng.permutation(n).astype(np.int32)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    src_idx = pos[tgt_idx].astype(np.int32)  # pair k: target key point tgt_idx[k] and the source key point made from it
    return pair, T_gt, tgt_kp, src_kp, tgt_idx, src_idx, good


def test_end_to_end_guess_for_icp(ctx_auto):
    """index lists -> mulls_coarse_reg_ransac_indexed -> mulls_icp with the result as init_guess: code 1 within the tolerances tests/test_gpu_icp.py uses against
    a planted transform (5 cm, 2e-3 rad); from the identity the same pair does not get there"""
    pair, T_gt, tgt_kp, src_kp, tgt_idx, src_idx, good = planted_key_point_pair(21)
    got = device(ctx_auto, tgt_kp, src_kp, 0.5, 20000, 1, tgt_idx=tgt_idx, src_idx=src_idx)
    want = rr.restate(rr.xyzw_of(tgt_kp)[tgt_idx], rr.xyzw_of(src_kp)[src_idx], 0.5, 8, 20000, 1)
    assert_same(got, want, "planted key points")
    assert got["status"] == 1 and good[tgt_idx[got["inliers"]]].mean() > 0.95
    dt, dr = synth.pose_error(got["T"], T_gt)
    assert dt < 0.2 and dr < np.deg2rad(0.5)
    P = abi.kitti_params()
    pair.init_guess = got["T"]
    r = ctx_auto.icp(pair, P)[0]
    dt, dr = synth.pose_error(r.T_matrix(), T_gt)
    assert r.code == 1 and dt < 0.05 and dr < 2e-3
    pair.init_guess = np.eye(4)
    r0 = ctx_auto.icp(pair, P)[0]
    dt0, dr0 = synth.pose_error(r0.T_matrix(), T_gt)
    assert r0.code < 0 or dt0 > 1.0 or not np.isfinite(dt0)  # the guess matters


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
from test_gpu_ransac import assert_same, device
Z = np.load(FIXTURE, allow_pickle=False)
ctx = lib.Context(0)
def cloud(x, n, stride=48):
    c = abi.Cloud()
    c.pts, c.n, c.stride = x.data_ptr(), n, stride
    return c
for name, it in (("noisy_517", 20000), ("half_4097", 100)):
    t, s, bound, _ = input_sets()[name]
    rt, rs = rr.records(t), rr.records(s)
    dev = {k: torch.from_numpy(raw.copy()).to("cuda:0") for k, raw in (("t", rt), ("s", rs))}
    pin = {k: torch.from_numpy(raw.copy()).pin_memory() for k, raw in (("t", rt), ("s", rs))}
    torch.cuda.synchronize()
    D = {k: cloud(x, len(x)) for k, x in dev.items()}
    H = {k: cloud(x, len(x)) for k, x in pin.items()}
    for rf in (0, 1):
        want = fixture_case(Z, rr.case_name(name, it, rf), len(t))
        for a, b in ((D["t"], D["s"]), (D["t"], rs), (rt, D["s"]), (H["t"], H["s"]), (H["t"], D["s"]), (D["t"], H["s"])):
            assert_same(device(ctx, a, b, bound, it, rf), want, (name, rf))
# the indexed entry point on device-resident key points
D0 = demo()
kt, ks = D0["kpts_0"], D0["kpts_15"]
dkt, dks = torch.from_numpy(kt.copy()).to("cuda:0"), torch.from_numpy(ks.copy()).to("cuda:0")
torch.cuda.synchronize()
for name in rr.DEMO_LISTS:
    pr = D0[name + "_pairs"]
    want = fixture_case(Z, rr.case_name("demo_" + name, 20000, 1), len(pr))
    for a, b in ((cloud(dkt, len(kt)), cloud(dks, len(ks))), (cloud(dkt, len(kt)), ks), (kt, cloud(dks, len(ks)))):
        assert_same(device(ctx, a, b, 1.0, 20000, 1, tgt_idx=pr[:, 0], src_idx=pr[:, 1]), want, name)
# a device cloud whose stride is not 48
wide = torch.zeros((517, 64), dtype=torch.uint8, device="cuda:0")
torch.cuda.synchronize()
t, s, bound, _ = input_sets()["noisy_517"]
res = abi.RansacResult()
P = abi.ransac_params(bound, 8, 100, 1)
good = cloud(torch.from_numpy(rr.records(s)).to("cuda:0"), 517)
for a, b in ((cloud(wide, 517, 64), good), (good, cloud(wide, 517, 64))):
    assert lib.load().mulls_coarse_reg_ransac(ctx.h, C.byref(a), C.byref(b), C.byref(P), C.byref(res), None, 0) == abi.MULLS_E_INVALID
ctx.close()
print("torch clouds ok")
"""


def test_device_resident_and_pinned_clouds():
    """pairs in torch device tensors and pinned host tensors, on either side, and device-resident key points behind the indexed entry point: the results of the
    host clouds.  A device cloud with stride 64 is refused."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", TORCH_CHILD % (root, os.path.join(root, "tests"))], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "torch clouds ok" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


def test_mulls_reg_tool_with_global_registration(tmp_path, capsys):
    """tools/mulls_reg.py on the reference's two demo scans with its default --is_global_reg=true: NCC -> RANSAC -> mm_lls_icp runs to completion, and
    --teaser_on is answered with the RANSAC solver.  (The demo scans' own key-point pairs carry about 5 % inliers: tests/test_ransac.py — whether the guess is
    the true pose is not asserted.)"""
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mulls_reg_tool", os.path.join(root, "tools", "mulls_reg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    Z = np.load(os.path.join(root, "tests", "golden", "demo_pair.npz"))
    paths = []
    for k in (0, 15):
        s = Z["scan_%d" % k]
        path = str(tmp_path / ("scan%d.pcd" % k))
        lib.write_pcd(path, abi.make_points(s[:, :3], np.zeros_like(s[:, :3]), s[:, 3]))
        paths.append(path)
    for extra in ([], ["--teaser_on=true", "--reciprocal_corr_on=true"]):
        res, source = tool.main(["--point_cloud_1_path", paths[0], "--point_cloud_2_path", paths[1]] + extra)
        out = capsys.readouterr().out
        assert "global registration:" in out and "RANSAC status" in out and source in (1, 2)
        assert ("TEASER++ is not part of the library" in out) == bool(extra)
        assert isinstance(res.code, int) and res.iters >= 1
