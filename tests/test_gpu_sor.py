"""GPU tests of mulls_sor_filter (CFilter::sor_filter, include/common/cfilter.hpp:204-247) through mulls_amd/lib.py, against the numpy restatement of the
library's definition (tests/sor_restated.py): computed here by brute force for the small and the edge families, read from tests/golden/sor_cases.npz for the
large cases (tests/test_sor.py keeps the fixture equal to the restatement).

Every comparison is equality: mean_dist bitwise; mean, stddev and threshold bitwise (two NaNs count as equal: the sign of the NaN a square root of a negative
variance produces is not part of the definition); the kept indices; the kept records byte for byte.  Nothing is left to a tolerance: the search is exact, the
distance expressions are correctly rounded operations in a fixed order without contraction, and the statistics' sums have a defined order.

PCL is not available where these tests run: nothing here was compared with PCL itself."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

import sor_restated as sr
from mulls_amd import abi, lib, synth
from test_sor import GOLDEN, fixture_case

pytestmark = pytest.mark.gpu


def records(xyz, seed=0):
    """48-byte records around the coordinates, every other byte random: what comes back must be these bytes"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    raw = np.random.default_rng(seed).integers(0, 256, (len(xyz), abi.POINT_BYTES), dtype=np.uint8)
    raw[:, :12] = xyz.view(np.uint8).reshape(len(xyz), 12)
    return raw


def same_double(a, b):
    a, b = np.float64(a), np.float64(b)
    return a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b))


def check(ctx, xyz, mean_k, std_mul, want, what, recs=None):
    """one device call against a restatement result (or a fixture case): every output"""
    recs = records(xyz, len(xyz)) if recs is None else recs
    kept, idx, rep, dist = ctx.sor_filter(recs, abi.sor_params(mean_k, std_mul), want_dist=True)
    if want.get("dist") is not None:
        bad = np.flatnonzero(dist.view(np.uint32) != want["dist"].view(np.uint32))
        assert len(bad) == 0, (what, len(bad), bad[:5], dist[bad[:5]], want["dist"][bad[:5]])
    if want.get("sha") is not None:
        assert hashlib.sha256(dist.tobytes()).digest() == want["sha"], what
    for k in ("mean", "stddev", "threshold"):
        assert same_double(getattr(rep, k), want[k]), (what, k, getattr(rep, k), want[k])
    assert np.array_equal(idx, want["kept_idx"]), what
    assert rep.n_in == len(recs) and rep.n_kept == len(idx) == len(kept)
    assert kept.tobytes() == recs[idx].tobytes(), what
    return rep, dist


@functools.lru_cache(maxsize=None)
def uniform_box(n):
    """(xyz, the 65 smallest squared distances of every point): one brute-force search serves every mean_k"""
    xyz = np.random.default_rng(n).uniform(-10, 10, (n, 3)).astype(np.float32)
    return xyz, sr.knn_brute(xyz, min(n, 65))


@pytest.mark.parametrize("n", [21, 22, 64, 1000, 4097, 30000])
def test_uniform_box(ctx_auto, n):
    """n x mean_k in {1, 8, 20, 64} wherever n > mean_k x std_mul in {-1, 0, 1, 2}"""
    xyz, d2 = uniform_box(n)
    recs, done = records(xyz, n), 0
    for mean_k in (1, 8, 20, 64):
        if n <= mean_k:
            continue
        for std_mul in (-1.0, 0.0, 1.0, 2.0):
            want = sr.restate(xyz, mean_k, std_mul, d2_sorted=np.ascontiguousarray(d2[:, : mean_k + 1]))
            check(ctx_auto, xyz, mean_k, std_mul, want, (n, mean_k, std_mul), recs)
            done += 1
    assert done >= 12


# ---------------------------------------------------------------------------------------------------------------- edge families
def edge_clouds():
    rng = np.random.default_rng(77)
    box = lambda n, s=5.0: rng.uniform(-s, s, (n, 3))  # noqa: E731
    out = {}
    out["exactly_k_plus_1"] = (box(21), 20)
    out["coincident"] = (np.tile(np.array([[1.5, -2.25, 0.75]]), (500, 1)), 20)
    c = box(3000)
    c[100:130] = c[100]  # 30 copies: more than mean_k + 1
    out["copies_inside"] = (c, 20)
    g = np.arange(14) * 0.25
    out["lattice"] = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), 20)
    p = box(2500)
    p[:, 2] = 0.5
    out["coplanar"] = (p, 20)
    t = rng.uniform(-30, 30, 1500)
    out["collinear"] = (np.stack([t, 0.5 * t + 1.0, -0.25 * t], -1), 8)
    out["within_1mm"] = (10.0 + rng.uniform(0, 1e-3, (800, 3)), 20)
    out["offset_1e5"] = (1e5 + box(4000, 3.0), 20)
    a, b = box(3000, 2.0), box(3000, 2.0) + np.array([5000.0, 0.0, 0.0])
    out["two_clusters_5km"] = (np.concatenate([a, b]), 20)
    out["one_far_point"] = (np.concatenate([box(5000, 3.0), [[1000.0, 0.0, 0.0]]]), 20)
    out["small_far_cluster"] = (np.concatenate([box(5000, 3.0), np.array([300.0, 200.0, 10.0]) + box(12, 0.05)]), 20)
    out["mean_k_64_far"] = (np.concatenate([box(3000, 3.0), np.array([80.0, 0.0, 0.0]) + box(40, 0.5)]), 64)
    return {k: (np.ascontiguousarray(v, np.float32), mk) for k, (v, mk) in out.items()}


@pytest.mark.parametrize("name", sorted(edge_clouds()))
def test_edge_families(ctx_auto, name):
    xyz, mean_k = edge_clouds()[name]
    d2 = sr.knn_brute(xyz, mean_k + 1)
    for std_mul in (0.0, 2.0):
        rep, _ = check(ctx_auto, xyz, mean_k, std_mul, sr.restate(xyz, mean_k, std_mul, d2_sorted=d2), (name, std_mul))
        if name in ("one_far_point", "small_far_cluster", "mean_k_64_far"):
            assert rep.n_fallback >= 1, name  # nothing within the ring budget of any level: answered by brute force, still exact
        if name == "coincident":
            assert rep.n_kept == len(xyz) and rep.mean == 0.0


# ---------------------------------------------------------------------------------------------------------------- large cases
@pytest.mark.parametrize("name", sorted(sr.LARGE_CASES))
def test_large_cases_equal_fixture(ctx_auto, name):
    """two synthetic scans, a real demo scan, a merged map of eight poses (about a million points): mean_k 20, std_mul 2.0, against tests/golden/sor_cases.npz"""
    xyz = sr.LARGE_CASES[name](GOLDEN)
    want = fixture_case(name)
    assert len(xyz) == want["n"]
    rep, _ = check(ctx_auto, xyz, 20, 2.0, want, name)
    assert rep.n_kept == want["n_kept"]


# ---------------------------------------------------------------------------------------------------------------- refusals and conventions
def raw_call(ctx, recs, mean_k=20, std_mul=2.0, stride=None, n=None, cap=None, idx_cap=None, out=True, idx=True, dist=True, report=True):
    recs = np.ascontiguousarray(recs)
    n = len(recs) if n is None else n
    c = abi.Cloud()
    c.pts, c.n, c.stride = (recs.ctypes.data if recs.size else None), n, recs.shape[1] if stride is None else stride
    cap = n if cap is None else cap
    idx_cap = n if idx_cap is None else idx_cap
    o = np.full((cap + 1, abi.POINT_BYTES), 0xA5, np.uint8)
    i = np.full(idx_cap + 1, -7, np.int32)
    d = np.full(n + 1, -3.0, np.float32)
    rep, n_out, p = abi.SorReport(), C.c_uint32(12345), abi.sor_params(mean_k, std_mul)
    rc = ctx.lib.mulls_sor_filter(ctx.h, C.byref(c), C.byref(p), o.ctypes.data_as(C.c_void_p) if out else None, cap if out else 0, C.byref(n_out),
                                  i.ctypes.data_as(C.c_void_p) if idx else None, idx_cap if idx else 0, d.ctypes.data_as(C.c_void_p) if dist else None,
                                  C.byref(rep) if report else None)
    assert (o[cap] == 0xA5).all() and i[idx_cap] == -7 and d[n] == -3.0  # nothing written past the capacities
    return rc, n_out.value, o[:cap], i[:idx_cap], d[:n], rep


def test_refusals(ctx_auto):
    xyz = np.random.default_rng(5).uniform(-5, 5, (400, 3)).astype(np.float32)
    recs = records(xyz)
    rc, n_out, _, _, _, rep = raw_call(ctx_auto, recs[:0])
    assert rc == abi.MULLS_OK and n_out == 0 and rep.n_kept == 0
    assert raw_call(ctx_auto, recs[:20])[0] == abi.MULLS_E_INVALID  # n == mean_k
    assert raw_call(ctx_auto, recs[:1])[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, mean_k=0)[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, mean_k=-3)[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, mean_k=65)[0] == abi.MULLS_E_UNSUPPORTED
    assert raw_call(ctx_auto, recs, mean_k=64)[0] == abi.MULLS_OK
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            x = xyz.copy()
            x[137, axis] = bad
            assert raw_call(ctx_auto, records(x))[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, std_mul=float("nan"))[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, std_mul=float("inf"))[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, stride=44)[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, stride=50)[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs)[0] == abi.MULLS_OK  # the context still works


def test_truncation_stride_and_null_outputs(ctx_auto):
    xyz = np.random.default_rng(6).uniform(-5, 5, (2000, 3)).astype(np.float32)
    recs = records(xyz)
    want = sr.restate(xyz, 20, 1.0)
    nk = int(want["keep"].sum())
    assert 100 < nk < len(xyz)
    rc, n_out, o, i, d, rep = raw_call(ctx_auto, recs, std_mul=1.0)
    assert rc == 0 and n_out == nk == rep.n_kept and np.array_equal(i[:nk], want["kept_idx"]) and o[:nk].tobytes() == recs[want["kept_idx"]].tobytes()
    assert d.tobytes() == want["dist"].tobytes() and rep.ms_total > 0
    # capacities below the kept count: truncated, the full count reported
    rc, n_out, o, i, _, rep = raw_call(ctx_auto, recs, std_mul=1.0, cap=50, idx_cap=7)
    assert rc == 0 and n_out == nk == rep.n_kept and np.array_equal(i, want["kept_idx"][:7]) and o.tobytes() == recs[want["kept_idx"][:50]].tobytes()
    # stride 64
    wide = np.random.default_rng(8).integers(0, 256, (len(recs), 64), dtype=np.uint8)
    wide[:, :48] = recs
    rc, n_out, o, i, d, _ = raw_call(ctx_auto, wide, std_mul=1.0)
    assert rc == 0 and n_out == nk and np.array_equal(i[:nk], want["kept_idx"]) and o[:nk].tobytes() == recs[want["kept_idx"]].tobytes()
    assert d.tobytes() == want["dist"].tobytes()
    # each output absent in turn
    for absent in ("out", "idx", "dist", "report"):
        rc, n_out, o, i, d, rep = raw_call(ctx_auto, recs, std_mul=1.0, **{absent: False})
        assert rc == 0 and n_out == nk, absent
        if absent != "out":
            assert o[:nk].tobytes() == recs[want["kept_idx"]].tobytes()
        if absent != "idx":
            assert np.array_equal(i[:nk], want["kept_idx"])
        if absent != "dist":
            assert d.tobytes() == want["dist"].tobytes()
        if absent != "report":
            assert same_double(rep.threshold, want["threshold"])


# ---------------------------------------------------------------------------------------------------------------- device-resident input
def test_device_resident_clouds(ctx_auto):
    """a LocalMap class cloud and a Block cloud give the result of the same cloud downloaded and passed from the host"""
    scene = synth.Scene(7)
    scan = synth.raycast(scene, synth.se3(0, 0, scene.sensor_height), 32, 900, seed=7)
    pts = abi.make_points(scan["xyz"], np.zeros_like(scan["xyz"]), scan["intensity"], scan["t"])
    X = abi.extract_params(ground=abi.ground_params(nonground_random_down_rate=1), classify=abi.classify_params(neighbor_k=20))
    b = ctx_auto.block().extract(pts, X)
    seen = 0
    for which in (abi.EX_GROUND, abi.EX_PILLAR + 2, abi.EX_VERTEX):
        host = b.download(which)
        if len(host) <= 20:
            continue
        seen += 1
        a = ctx_auto.sor_filter(b.cloud(which), want_dist=True)
        h = ctx_auto.sor_filter(host, want_dist=True)
        assert a[0].tobytes() == h[0].tobytes() and np.array_equal(a[1], h[1]) and a[3].tobytes() == h[3].tobytes()
        assert same_double(a[2].threshold, h[2].threshold) and a[2].n_kept == h[2].n_kept and 0 < a[2].n_kept < len(host)
        assert a[0].tobytes() == host[a[1]].tobytes()
    assert seen >= 2
    clouds = [abi.points_of(b.download(k)) for k in (abi.EX_GROUND, abi.EX_PILLAR, abi.EX_PILLAR + 2, abi.EX_PILLAR + 1, abi.EX_PILLAR + 3, abi.EX_VERTEX)]
    m = lib.LocalMap(ctx_auto, clouds, np.eye(4))
    for cls in (abi.GROUND, abi.FACADE):
        host = abi.records(m.download(cls))
        assert len(host) > 20
        a = ctx_auto.sor_filter(m.cloud(cls), want_dist=True)
        h = ctx_auto.sor_filter(host, want_dist=True)
        assert a[0].tobytes() == h[0].tobytes() and np.array_equal(a[1], h[1]) and a[3].tobytes() == h[3].tobytes() and same_double(a[2].threshold, h[2].threshold)
    m.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- reuse
def test_reuse(ctx_auto, pairs_small):
    """the same call twice: the same bits; a registration on the same context is not disturbed; a small cloud after a large one is still right"""
    P = abi.kitti_params(dis_thre_unit=2.4)
    pair = pairs_small[0][0]  # (pair, ground-truth transform)
    T0 = list(ctx_auto.icp(pair, P)[0].T[:])
    big = sr.synth_scan(3, 64, 1900)
    a = ctx_auto.sor_filter(records(big, 1), want_dist=True)
    b = ctx_auto.sor_filter(records(big, 1), want_dist=True)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[3].tobytes() == b[3].tobytes()
    assert all(same_double(getattr(a[2], k), getattr(b[2], k)) for k in ("mean", "stddev", "threshold")) and a[2].n_fallback == b[2].n_fallback
    assert np.array_equal(a[1], fixture_case("scan3")["kept_idx"])
    assert list(ctx_auto.icp(pair, P)[0].T[:]) == T0
    xyz, d2 = uniform_box(1000)
    check(ctx_auto, xyz, 20, 2.0, sr.restate(xyz, 20, 2.0, d2_sorted=np.ascontiguousarray(d2[:, :21])), "small after large")
    assert list(ctx_auto.icp(pair, P)[0].T[:]) == T0
