"""GPU tests of mulls_coarse_reg_teaser / mulls_coarse_reg_teaser_indexed (coarse_reg_teaser, include/common/cregistration.hpp:664-759) through mulls_amd/lib.py,
against the numpy restatement of the library's definition (tests/teaser_restated.py) as tests/golden/teaser_cases.npz pins it (tests/test_teaser.py keeps the
two equal, and holds the product's host code against the same restatement on the CPU).

Every comparison is equality: status, n_edges, max_core, clique_size, clique_exact, gnc_iterations, both inlier counts, the clique list — and every bit of
cost and T.  Tolerance: none.  The definition is double arithmetic in a fixed order with + - * / sqrt only, built without contraction, and every one of
these operations is correctly rounded on the device as in numpy; the sums over up to C (C - 1) / 2 measurements have a defined order (4096 strided partial
sums, then a pairwise tree) that the restatement follows, so the sums are the same bits.  Every case has clique_exact == 1 (the restatement's exhaustive
enumeration is what the fixture holds).  clique_nodes, the search's effort, is not part of the definition: it is only required to repeat.

TEASER++ is not available where these tests run: nothing here was compared with TEASER++ itself."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import teaser_restated as tr
from mulls_amd import abi, lib
from test_teaser import INT_KEYS, demo, fixture_case, input_sets

pytestmark = pytest.mark.gpu


def device(ctx, t, s, nb, min_inlier=8, cap=None, budget=abi.TEASER_DEFAULT_NODE_BUDGET, **kw):
    def rec(x):
        return tr.records(x) if isinstance(x, np.ndarray) and x.ndim == 2 and x.shape[1] == 4 and x.dtype == np.float32 else x

    return as_dict(*ctx.coarse_reg_teaser(rec(t), rec(s), abi.teaser_params(nb, min_inlier, budget), cap, **kw))


def as_dict(res, clique):
    out = {k: int(getattr(res, k)) for k in INT_KEYS + ("clique_nodes",)}
    out.update(cost=float(res.cost), T=np.array(res.T[:], np.float64).reshape(4, 4).T.copy(), clique=clique.astype(np.int64))
    return out


def assert_same(got, want, what, clique=True):
    for k in INT_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    if clique:
        assert np.array_equal(got["clique"], want["clique"]), (what, got["clique"], want["clique"])
    assert np.float64(got["cost"]).tobytes() == np.float64(want["cost"]).tobytes(), (what, got["cost"], want["cost"])
    assert np.asarray(got["T"], np.float64).tobytes() == np.asarray(want["T"], np.float64).tobytes(), (what, got["T"], want["T"])


@pytest.mark.parametrize("name", sorted(tr.input_sets(None)) + ["demo_%s_nb%d" % (n, b) for n in tr.DEMO_LISTS for b in (25, 100)])
def test_device_equals_restatement(ctx_auto, name):
    """the word and wave edges N = 31 .. 65, 1023 .. 1025, 4097 and 8192 (a planted clique among sparse outliers), no edge, a single edge (M = 1), a complete
    graph of 300 (M = 44 850), two maximum cliques, each exit of the GNC loop, NaN and infinite coordinates, the planted sets and the demo pair lists"""
    t, s, nb = input_sets()[name]
    want = fixture_case(name)
    assert want["clique_exact"] == 1
    assert_same(device(ctx_auto, t, s, nb, tr.min_inlier(name)), want, name)


def cloud_of(raw, stride=48, n=None):
    c = abi.Cloud()
    c.pts, c.n, c.stride = raw.ctypes.data, len(raw) if n is None else n, stride
    return c


def test_outcomes_and_refusals(ctx_auto):
    L = lib.load()
    t, s, nb = input_sets()["size_64"]
    rt, rs = tr.records(t), tr.records(s)
    res, cl = abi.TeaserResult(), np.full(8, -7, np.int32)
    ip = cl.ctypes.data_as(C.c_void_p)

    def call(ct, cs, P):
        return L.mulls_coarse_reg_teaser(ctx_auto.h, C.byref(ct), C.byref(cs), C.byref(P), C.byref(res), ip, 4)

    good = abi.teaser_params(nb)
    for n in (0, 3):  # upstream: "too few correspondences", -1
        res.status = 5
        assert call(cloud_of(rt, n=n), cloud_of(rs, n=n), good) == abi.MULLS_OK
        assert res.status == -1 and res.clique_size == 0 and np.array_equal(np.array(res.T[:]).reshape(4, 4), np.eye(4)) and (cl == -7).all()
    res.status = 5
    assert call(cloud_of(rt), cloud_of(rs, n=63), good) == abi.MULLS_OK and res.status == -1 and (cl == -7).all()  # unequal sizes: upstream's -1
    t4, s4, _, _ = tr.planted(4, 4, 0.0)
    want = tr.restate(t4, s4, 0.2, 3)
    assert want["clique_size"] == 4 and want["n_rotation_inliers"] == 6 and want["status"] == 1
    assert_same(device(ctx_auto, t4, s4, 0.2, 3), want, "N = 4")
    big = np.zeros((8193, 48), np.uint8)
    assert call(cloud_of(big), cloud_of(big), good) == abi.MULLS_E_UNSUPPORTED
    for bad in (float("nan"), float("inf"), float("-inf"), -0.5):
        assert call(cloud_of(rt), cloud_of(rs), abi.teaser_params(bad)) == abi.MULLS_E_INVALID
    for stride in (12, 18, 50):
        buf = np.zeros((64, stride), np.uint8)
        assert call(cloud_of(buf, stride), cloud_of(rs), good) == abi.MULLS_E_INVALID
        assert call(cloud_of(rt), cloud_of(buf, stride), good) == abi.MULLS_E_INVALID
    assert L.mulls_coarse_reg_teaser(None, None, None, None, None, None, 0) == abi.MULLS_E_INVALID
    assert (cl == -7).all()
    idx = np.arange(64, dtype=np.int32)
    bad = idx.copy()
    bad[10] = 64
    for a, b in ((bad, idx), (idx, bad)):
        rc = L.mulls_coarse_reg_teaser_indexed(ctx_auto.h, C.byref(cloud_of(rt)), C.byref(cloud_of(rs)), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), 64,
                                               C.byref(good), C.byref(res), ip, 4)
        assert rc == abi.MULLS_E_INVALID
    assert_same(device(ctx_auto, t, s, nb), fixture_case("size_64"), "after refusals")  # and the context goes on
    z = device(ctx_auto, t, s, 0.0)  # a zero bound is allowed: only exactly equal distances are consistent
    assert z["status"] == -1 and z["clique_size"] <= 2


def test_single_entry_points_at_their_own_edges(ctx_auto):
    """what only the single entry points define: the indexed call's early returns (no pairs and NULL lists, three pairs), one index list without the other,
    a NULL result, a clique capacity without a buffer — and the message of every refusal that sets one names the entry point that was called"""
    L = lib.load()
    t, s, nb = input_sets()["size_64"]
    rt, rs = tr.records(t), tr.records(s)
    ct, cs = cloud_of(rt), cloud_of(rs)
    good = abi.teaser_params(nb)
    res, cl = abi.TeaserResult(), np.full(8, -7, np.int32)
    ip = cl.ctypes.data_as(C.c_void_p)
    idx = np.arange(64, dtype=np.int32)

    def vp(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def plain(a, b, P=good, result=res, clique=ip, cap=4):
        return L.mulls_coarse_reg_teaser(ctx_auto.h, C.byref(a), C.byref(b), C.byref(P), result, clique, cap)

    def indexed(ti, si, n, a=ct, b=cs, P=good, result=res, clique=ip, cap=4):
        return L.mulls_coarse_reg_teaser_indexed(ctx_auto.h, C.byref(a), C.byref(b), vp(ti), vp(si), n, C.byref(P), result, clique, cap)

    for ti, si, n in ((None, None, 0), (idx, idx, 3)):  # upstream: "too few correspondences", -1
        res.status, res.clique_size = 5, 9
        assert indexed(ti, si, n) == abi.MULLS_OK
        assert res.status == -1 and res.clique_size == 0 and np.array_equal(np.array(res.T[:]).reshape(4, 4), np.eye(4)) and (cl == -7).all()
    assert indexed(idx, None, 64) == abi.MULLS_E_INVALID and indexed(None, idx, 64) == abi.MULLS_E_INVALID
    assert plain(ct, cs, result=None) == abi.MULLS_E_INVALID and indexed(idx, idx, 64, result=None) == abi.MULLS_E_INVALID
    assert plain(ct, cs, clique=None) == abi.MULLS_E_INVALID and indexed(idx, idx, 64, clique=None) == abi.MULLS_E_INVALID

    def said(who):
        msg = L.mulls_last_error(ctx_auto.h) or b""
        assert msg.startswith(who + b":") and b"problem" not in msg, msg

    big, odd = np.zeros((8193, 48), np.uint8), np.zeros((64, 18), np.uint8)
    many, bad = np.zeros(8193, np.int32), idx.copy()
    bad[10] = 64
    nan = abi.teaser_params(float("nan"))
    for refuse, who, code in ((lambda: plain(cloud_of(big), cloud_of(big)), b"mulls_coarse_reg_teaser", abi.MULLS_E_UNSUPPORTED),
                              (lambda: plain(cloud_of(odd, 18), cs), b"mulls_coarse_reg_teaser", abi.MULLS_E_INVALID),
                              (lambda: plain(ct, cs, P=nan), b"mulls_coarse_reg_teaser", abi.MULLS_E_INVALID),
                              (lambda: indexed(many, many, 8193), b"mulls_coarse_reg_teaser_indexed", abi.MULLS_E_UNSUPPORTED),
                              (lambda: indexed(idx, idx, 64, a=cloud_of(odd, 18)), b"mulls_coarse_reg_teaser_indexed", abi.MULLS_E_INVALID),
                              (lambda: indexed(bad, idx, 64), b"mulls_coarse_reg_teaser_indexed", abi.MULLS_E_INVALID),
                              (lambda: indexed(idx, idx, 64, P=nan), b"mulls_coarse_reg_teaser_indexed", abi.MULLS_E_INVALID)):
        res.status = 5
        assert refuse() == code
        said(who)
        assert res.status == -1 and (cl == -7).all()
    assert_same(device(ctx_auto, t, s, nb, tgt_idx=idx, src_idx=idx), fixture_case("size_64"), "after refusals")


def test_batch_and_single_calls_share_one_scratch():
    """one context: a batch, a single call, a batch, a single call — the grow-only scratch carries nothing from one kind of call into the other"""
    ctx = lib.Context(0)
    try:
        def batch(names):
            sets = [input_sets()[name] for name in names]
            assert all(nb == 0.2 for _, _, nb in sets)
            got = ctx.coarse_reg_teaser_batch([(tr.records(t), tr.records(s)) for t, s, _ in sets], abi.teaser_params(0.2))
            for (res, clique), name in zip(got, names):
                assert_same(as_dict(res, clique), fixture_case(name), ("batch", name))

        def single(name):
            t, s, nb = input_sets()[name]
            assert_same(device(ctx, t, s, nb), fixture_case(name), ("single", name))

        batch(["size_1025", "complete_300", "no_edge"])
        single("size_31")
        batch(["exit_cost"])
        single("size_1025")
    finally:
        ctx.close()


def strided(raw, stride, seed):
    n, w = len(raw), min(stride, 48)
    buf = np.random.default_rng(seed).integers(0, 256, (n, stride), dtype=np.uint8)
    buf[:, :w] = raw[:, :w]
    return buf, cloud_of(buf, stride)


def test_host_strides_and_cap(ctx_auto):
    name = "demo_recip_0_15_nb25"
    t, s, nb = input_sets()[name]
    want = fixture_case(name)
    rt, rs = tr.records(t), tr.records(s)
    for stride in (16, 36, 48, 64):
        bt, ct = strided(rt, stride, stride)
        bs, cs = strided(rs, stride, stride + 1)
        for a, b in ((ct, cs), (ct, rs), (rt, cs)):
            assert_same(device(ctx_auto, a, b, nb), want, stride)
    for cap in (0, 1, 20, want["clique_size"], want["clique_size"] + 5):
        got = device(ctx_auto, t, s, nb, cap=cap)  # (lib.py checks that the slot behind cap is left alone)
        assert_same(got, want, cap, clique=False)
        assert np.array_equal(got["clique"], want["clique"][:cap])


def test_indexed_equals_gathered(ctx_auto):
    Z = demo()
    for name in tr.DEMO_LISTS:
        a, b = (0, 15) if name.endswith("0_15") else (15, 0)
        kt, ks, pr = Z["kpts_%d" % a], Z["kpts_%d" % b], Z[name + "_pairs"]
        for nb in (0.25, 1.0):
            want = fixture_case("demo_%s_nb%d" % (name, int(100 * nb)))
            assert_same(device(ctx_auto, kt, ks, nb, tgt_idx=pr[:, 0], src_idx=pr[:, 1]), want, (name, nb))
            assert_same(device(ctx_auto, kt[pr[:, 0]], ks[pr[:, 1]], nb), want, (name, nb, "gathered"))
    pr = Z["recip_0_15_pairs"][:3]  # three pairs: too few
    got = device(ctx_auto, Z["kpts_0"], Z["kpts_15"], 1.0, tgt_idx=pr[:, 0], src_idx=pr[:, 1])
    assert got["status"] == -1 and got["clique_size"] == 0


def test_small_call_after_the_largest_and_budget(ctx_auto):
    """one context: a small set, the largest, the small one again — the grow-only scratch keeps nothing of the call before; the search's effort repeats;
    a budget that ends the search gives clique_exact = 0 and the same clique on every run"""
    for name in ("size_31", "size_8192", "size_31", "complete_300", "single_edge", "demo_recip_15_0_nb100", "size_33"):
        t, s, nb = input_sets()[name]
        a, b = device(ctx_auto, t, s, nb), device(ctx_auto, t, s, nb)
        assert_same(a, fixture_case(name), name)
        assert_same(b, fixture_case(name), name)
        assert a["clique_nodes"] == b["clique_nodes"]
    t, s, nb = input_sets()["demo_recip_15_0_nb100"]
    a, b = device(ctx_auto, t, s, nb, budget=50), device(ctx_auto, t, s, nb, budget=50)
    assert a["clique_exact"] == 0 and a["clique_nodes"] == 51 and np.array_equal(a["clique"], b["clique"]) and a["T"].tobytes() == b["T"].tobytes()
    assert 2 <= a["clique_size"] <= fixture_case("demo_recip_15_0_nb100")["clique_size"]
    adj = tr.graph(t, s, nb)
    assert all(adj[i, j] for i in a["clique"] for j in a["clique"] if i != j)


# torch brings a HIP runtime of its own: a process takes one of the two, the one loaded first, so the tensors live in a child that imports torch first
TORCH_CHILD = r"""
import ctypes as C, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
torch.cuda.init()
assert torch.zeros(4, device="cuda:0").sum().item() == 0
import teaser_restated as tr
from mulls_amd import abi, lib
from test_teaser import demo, fixture_case, input_sets
from test_gpu_teaser import assert_same, device
ctx = lib.Context(0)
def cloud(x, n, stride=48):
    c = abi.Cloud()
    c.pts, c.n, c.stride = x.data_ptr(), n, stride
    return c
for name in ("size_65", "demo_fixed300_0_15_nb25"):
    t, s, nb = input_sets()[name]
    rt, rs = tr.records(t), tr.records(s)
    dev = {k: torch.from_numpy(raw.copy()).to("cuda:0") for k, raw in (("t", rt), ("s", rs))}
    pin = {k: torch.from_numpy(raw.copy()).pin_memory() for k, raw in (("t", rt), ("s", rs))}
    torch.cuda.synchronize()
    D = {k: cloud(x, len(x)) for k, x in dev.items()}
    H = {k: cloud(x, len(x)) for k, x in pin.items()}
    want = fixture_case(name)
    for a, b in ((D["t"], D["s"]), (D["t"], rs), (rt, D["s"]), (H["t"], H["s"]), (H["t"], D["s"]), (D["t"], H["s"])):
        assert_same(device(ctx, a, b, nb), want, name)
# the indexed entry point on device-resident key points
D0 = demo()
kt, ks = D0["kpts_0"], D0["kpts_15"]
dkt, dks = torch.from_numpy(kt.copy()).to("cuda:0"), torch.from_numpy(ks.copy()).to("cuda:0")
torch.cuda.synchronize()
pr = D0["recip_0_15_pairs"]
want = fixture_case("demo_recip_0_15_nb25")
for a, b in ((cloud(dkt, len(kt)), cloud(dks, len(ks))), (cloud(dkt, len(kt)), ks), (kt, cloud(dks, len(ks)))):
    assert_same(device(ctx, a, b, 0.25, tgt_idx=pr[:, 0], src_idx=pr[:, 1]), want, "indexed")
# a device cloud whose stride is not 48
wide = torch.zeros((65, 64), dtype=torch.uint8, device="cuda:0")
torch.cuda.synchronize()
t, s, nb = input_sets()["size_65"]
res, P = abi.TeaserResult(), abi.teaser_params(nb)
good = cloud(torch.from_numpy(tr.records(s)).to("cuda:0"), 65)
for a, b in ((cloud(wide, 65, 64), good), (good, cloud(wide, 65, 64))):
    assert lib.load().mulls_coarse_reg_teaser(ctx.h, C.byref(a), C.byref(b), C.byref(P), C.byref(res), None, 0) == abi.MULLS_E_INVALID
ctx.close()
print("torch clouds ok")
"""


def test_device_resident_and_pinned_clouds():
    """pairs in torch device tensors and pinned host tensors, on either side, and device-resident key points behind the indexed entry point: the results of the
    host clouds.  A device cloud with stride 64 is refused."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", TORCH_CHILD % (root, os.path.join(root, "tests"))], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "torch clouds ok" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


def test_mulls_reg_tool_with_the_teaser_solver(tmp_path, capsys):
    """tools/mulls_reg.py on the reference's two demo scans with --global_solver=teaser: NCC -> TEASER -> mm_lls_icp runs to completion"""
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
    res, source = tool.main(["--point_cloud_1_path", paths[0], "--point_cloud_2_path", paths[1], "--global_solver=teaser", "--reciprocal_corr_on=true"])
    out = capsys.readouterr().out
    assert "global registration:" in out and "TEASER status" in out and "RANSAC status" not in out and source in (1, 2)
    assert isinstance(res.code, int) and res.iters >= 1
