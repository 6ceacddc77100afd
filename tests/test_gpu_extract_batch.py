"""mulls_extract_features_batch on the device: every scan of a batch gets the bytes of its own mulls_extract_features_resident call — the fourteen counts, every
record of the twelve clouds a block holds, the status — whatever the batch size, the scan's position, its neighbours and the sub-batch cuts are.  The yardstick
is the single call on the same context type (Block.extract + Block.download of every cloud); for the synthetic scans pyoracle.extract_features is a second one.
The host side (layout, planner, bridge) is tested in tests/test_extract_batch.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from mulls_amd import abi, lib, synth
from oracle import pyoracle

import front_end_edges as fe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD = [k for k in range(abi.EX_COUNT) if k not in (abi.EX_RAW, abi.EX_DOWN)]  # the twelve clouds a block holds


def raw_scan(seed, n_beams=64, n_az=1900, tilt=0.0):
    """A synthetic scan in the sensor frame (z up, sensor 1.73 m above the ground), all returns, as 48-byte records (the recipe of tests/test_ground_filter.py)."""
    scene = synth.Scene(seed)
    pose = synth.se3(0, 0, scene.sensor_height, tilt, -tilt, 0.1 * seed)
    s = synth.raycast(scene, pose, n_beams, n_az, seed=seed)
    return abi.make_points(s["xyz"], np.zeros_like(s["xyz"]), s["intensity"], s["t"])


@functools.lru_cache(maxsize=None)
def scans():
    return {"s16": raw_scan(6, 16, 400), "s32": raw_scan(7, 32, 700), "s64": raw_scan(8, 64, 300), "seg1025": fe.segment_cloud(1025), "chain": fe.promotion_chain_cloud(),
            "classify": fe.classify_cloud(), "line": fe.line_cloud(), "onecell": fe.one_cell_cloud()}


NAMES = ["s16", "s32", "s64", "seg1025", "chain", "classify", "line", "onecell"]


def set_d(**kw):
    return abi.extract_params(**kw)


def set_k():
    return abi.extract_params(ground=abi.ground_params(estimate_ground_normal_method=3, fixed_num_downsampling=1, down_ground_fixed_num=300),
                              classify=abi.classify_params(fixed_num_downsampling=1, unground_down_fixed_num=3000, pillar_down_fixed_num=50, facade_down_fixed_num=200,
                                                           beam_down_fixed_num=50, roof_down_fixed_num=50),
                              apply_dist_filter=1, apply_scanner_filter=1)


SETS = {"D": set_d, "K": set_k}


def single(ctx, scan, X):
    """the yardstick: (rc, the fourteen counts, the twelve held clouds) of one mulls_extract_features_resident call"""
    blk = lib.Block(ctx)
    raw = abi.records(scan)
    nout = (C.c_uint32 * abi.EX_COUNT)()
    rc = ctx.lib.mulls_extract_features_resident(ctx.h, raw.ctypes.data_as(C.c_void_p) if len(raw) else None, len(raw), abi.POINT_BYTES, C.byref(X), blk.h, nout)
    clouds = {k: blk.download(k) for k in HELD}
    blk.close()
    return rc, list(nout), clouds


_SINGLE = {}


def single_of(ctx, name, set_name):
    """computed once per (scan, set) and shared"""
    key = (name, set_name)
    if key not in _SINGLE:
        _SINGLE[key] = single(ctx, scans()[name], SETS[set_name]())
    return _SINGLE[key]


def batch(ctx, scan_list, X, limit=0, blocks=None):
    blocks, results, stats = ctx.extract_features_batch(scan_list, X, blocks=blocks, scratch_limit_bytes=limit, check=False)
    out = [(r.status, list(r.n_out), {k: b.download(k) for k in HELD}, r.path) for b, r in zip(blocks, results)]
    return out, stats, ctx.last_batch_rc, blocks


def close(blocks):
    for b in blocks:
        b.close()


def assert_same(got, want, what, path=0):
    status, n_out, clouds, p = got
    rc, n_want, c_want = want
    assert status == rc, (what, status, rc)
    assert n_out == n_want, (what, n_out, n_want)
    assert p == path, (what, p)
    for k in HELD:
        assert clouds[k].shape == c_want[k].shape, (what, k, clouds[k].shape, c_want[k].shape)
        assert np.array_equal(clouds[k], c_want[k]), (what, k)
        if rc == abi.MULLS_OK:
            assert len(clouds[k]) == n_out[k], (what, k)
        else:
            assert len(clouds[k]) == 0, (what, k)  # a refused scan leaves its block with all sizes zero


def preconditions(ctx):
    """what makes the mixed batch worth running, asserted on the single path's sizes"""
    n = {(name, s): single_of(ctx, name, s)[1] for name in NAMES for s in SETS}
    P = abi.EX_PILLAR
    assert all(single_of(ctx, name, s)[0] == abi.MULLS_OK for name in NAMES for s in SETS)
    assert [name for name in NAMES if n[(name, "K")][abi.EX_UNGROUND] == 3000] == ["s64"] and n[("s64", "D")][abi.EX_UNGROUND] > 3000  # one scan thinned next to scans that are not
    assert all(n[(name, "K")][abi.EX_UNGROUND] < 3000 for name in NAMES if name != "s64")
    assert n[("s64", "D")][P] >= 10 and n[("s64", "D")][P + 1] >= 10 and n[("s64", "D")][P + 2] >= 10  # classes that go through the suppression ...
    assert n[("chain", "D")][P] == 0 and n[("seg1025", "D")][P:P + 4] == [0, 0, 0, 0] and 0 < min(n[("classify", "D")][P + 4:P + 8]) < 10  # ... next to classes that skip it
    assert n[("s16", "D")][P + 3] == 0 and n[("classify", "D")][P + 3] > 0  # roof clouds in some scans only
    assert n[("s16", "D")][abi.EX_VERTEX] == 0 and n[("s64", "D")][abi.EX_VERTEX] > 0 and n[("classify", "D")][abi.EX_VERTEX] > 0  # vertex clouds likewise
    assert n[("onecell", "K")][abi.EX_RAW] == 0  # empty after the pre-filter
    assert n[("line", "D")][abi.EX_GROUND] == 0 and n[("line", "D")][abi.EX_UNGROUND] == 0  # leaves the ground filter with nothing
    assert len(scans()["seg1025"]) == 1025 and n[("seg1025", "K")][abi.EX_RAW] < 1025  # one point past a 1 024-point segment; the pre-filter takes some
    assert n[("chain", "D")][P + 1] > 0 and n[("chain", "D")][P] == 0  # the promotion chain makes beams only
    assert [len(scans()[name]) for name in NAMES] == [6375, 22400, 19182, 1025, 964, 3125, 200, 500]
    return n


# ---------------------------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("set_name", ["D", "K"])
def test_mixed_batch_equals_single_calls(ctx_auto, set_name):
    """1: the eight scans side by side; the synthetic ones against the CPU oracle too.  2: reversed, and with s16 three times (nine scans)"""
    preconditions(ctx_auto)
    X = SETS[set_name]()
    got, stats, rc, blocks = batch(ctx_auto, [scans()[name] for name in NAMES], X)
    assert rc == abi.MULLS_OK and stats.n_subbatches == 1 and stats.n_lockstep == 8 and stats.n_single_path == 0
    for name, g in zip(NAMES, got):
        assert_same(g, single_of(ctx_auto, name, set_name), (set_name, name))
    for name in ("s16", "s32", "s64"):
        want = pyoracle.extract_features(scans()[name], X)
        g = got[NAMES.index(name)]
        assert g[1] == [len(w) for w in want], (set_name, name, g[1], [len(w) for w in want])
        for k in HELD:
            assert np.array_equal(g[2][k], want[k]), (set_name, name, k)
    close(blocks)
    # independence: the order reversed
    rev, _, rc, blocks = batch(ctx_auto, [scans()[name] for name in reversed(NAMES)], X)
    assert rc == abi.MULLS_OK
    for name, g in zip(reversed(NAMES), rev):
        assert_same(g, single_of(ctx_auto, name, set_name), (set_name, "reversed", name))
    close(blocks)
    # ... and s16 three times among the others: nine scans
    order = ["s16", "s32", "s16", "s64", "seg1025", "chain", "classify", "line", "s16"]
    nine, _, rc, blocks = batch(ctx_auto, [scans()[name] for name in order], X)
    assert rc == abi.MULLS_OK and len(nine) == 9
    for name, g in zip(order, nine):
        assert_same(g, single_of(ctx_auto, name, set_name), (set_name, "nine", name))
    copies = [g for name, g in zip(order, nine) if name == "s16"]
    for g in copies[1:]:
        assert g[1] == copies[0][1] and all(np.array_equal(g[2][k], copies[0][2][k]) for k in HELD)
    close(blocks)


# ---------------------------------------------------------------------------------------------------------------------------------- 3
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    from mulls_amd import build

    so = str(tmp_path_factory.mktemp("extract_batch_harness") / "extract_batch_harness.so")
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "include")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", rocm_inc,
                           os.path.join(ROOT, "tests", "extract_batch_harness.cpp"), "-o", so])
    L = C.CDLL(so)
    L.eb_head_bytes.restype = C.c_uint64
    L.eb_scan_cost.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    L.eb_cuts.restype = C.c_uint32
    return L


def scan_bytes(L, n, X):
    out = (C.c_uint64 * 3)()
    L.eb_scan_cost(n, int(bool(X.apply_dist_filter or X.apply_scanner_filter)), X.ground.estimate_ground_normal_method, X.classify.fixed_num_downsampling,
                   X.classify.unground_down_fixed_num, X.classify.neighbor_k, out)
    return int(out[2])


@pytest.mark.parametrize("set_name", ["D", "K"])
def test_sub_batch_cuts(ctx_auto, planner, set_name):
    """3: every scan alone, then a cut after the third scan — limits derived from the planner; the same bits"""
    X = SETS[set_name]()
    need = [scan_bytes(planner, len(scans()[name]), X) for name in NAMES]
    head = planner.eb_head_bytes()
    alone, stats, rc, blocks = batch(ctx_auto, [scans()[name] for name in NAMES], X, limit=1)
    assert rc == abi.MULLS_OK and stats.n_subbatches == 8
    for name, g in zip(NAMES, alone):
        assert_same(g, single_of(ctx_auto, name, set_name), (set_name, "alone", name))
    close(blocks)
    # a cut behind the third scan.  Under D the other five fit together: two sub-batches.  Under K every scan's search-grid tables (2 x 16 MiB) make the five
    # small scans dearer than the three large ones, so no limit gives 3 + 5: the first three fill the limit and the planner says how the rest is cut.
    limit = head + max(sum(need[:3]), sum(need[3:]))
    if set_name == "K":
        assert head + sum(need[:4]) <= limit
        limit = head + sum(need[:3])
    assert head + sum(need[:3]) <= limit < head + sum(need[:4])
    arr, cuts = (C.c_uint64 * 8)(*need), (C.c_uint32 * 10)()
    k = planner.eb_cuts(arr, 8, C.c_uint64(limit), cuts)
    assert list(cuts[:2]) == [0, 3] and cuts[k - 1] == 8
    if set_name == "D":
        assert k - 1 == 2
    cut, stats, rc, blocks = batch(ctx_auto, [scans()[name] for name in NAMES], X, limit=limit)
    assert rc == abi.MULLS_OK and stats.n_subbatches == k - 1
    for name, g in zip(NAMES, cut):
        assert_same(g, single_of(ctx_auto, name, set_name), (set_name, "cut", name))
    close(blocks)


# ---------------------------------------------------------------------------------------------------------------------------------- 4, 5
def test_lock_step_without_a_clock():
    """4: six copies of s16 under K cost the launches, waits and rounds of one copy: every step once per sub-batch"""
    X = set_k()
    counts = []
    for copies in (6, 1):
        ctx = lib.Context(0)
        got, stats, rc, blocks = batch(ctx, [scans()["s16"]] * copies, X)
        assert rc == abi.MULLS_OK and stats.n_subbatches == 1 and stats.n_lockstep == copies
        counts.append((stats.n_kernel_launches, stats.n_syncs, stats.promote_rounds, stats.nms_rounds))
        want = single(ctx, scans()["s16"], X)
        for g in got:
            assert_same(g, want, ("copies", copies))
        close(blocks)
        ctx.close()
    print("launches, waits, promotion rounds, suppression rounds:", counts)
    assert counts[0] == counts[1] and counts[0][0] > 0 and counts[0][1] > 0 and counts[0][2] > 0 and counts[0][3] > 0


def test_rounds_of_unequal_length(ctx_auto):
    """5: the promotion chain, which needs many rounds, next to a scan that needs few: the loop runs until the chain has settled"""
    X = set_d()
    rounds = []
    for names in (["chain"], ["chain", "s16"]):
        ctx = lib.Context(0)  # fresh: the first batch of rounds follows no earlier call
        got, stats, rc, blocks = batch(ctx, [scans()[n] for n in names], X)
        assert rc == abi.MULLS_OK
        for name, g in zip(names, got):
            assert_same(g, single_of(ctx_auto, name, "D"), ("rounds", name))
        rounds.append(stats.promote_rounds)
        close(blocks)
        ctx.close()
    print("promotion rounds launched: chain alone", rounds[0], "chain and s16", rounds[1])
    assert rounds[1] >= rounds[0] > 0


# ---------------------------------------------------------------------------------------------------------------------------------- 6
def refused_scans():
    s16 = scans()["s16"]
    far = abi.make_points(np.array([[450.0, 450.0, 0.0], [-450.0, 450.0, 0.0], [450.0, -450.0, 0.0], [-450.0, -450.0, 0.0]]), np.zeros((4, 3)), np.zeros(4), np.zeros(4))
    wide = np.concatenate([s16, far])
    nan_first = s16.copy()
    nan_first["x"][0] = np.nan
    # the first record is a low point: the ground filter decides about it before any classification sees it.  A NaN that does reach the classification: in the
    # first return above the ground threshold (mean height + 2 m; sensor frame, ground near z = -1.7) whose index the non-ground rate (3) keeps
    high = [j for j in range(0, len(s16), 3) if s16["z"][j] > 1.0][0]
    nan_high = s16.copy()
    nan_high["x"][high] = np.nan
    return {"wide": wide, "nan_first": nan_first, "nan_high": nan_high}


@pytest.mark.parametrize("which", ["wide", "nan_first", "nan_high"])
def test_a_refused_scan_in_the_middle(ctx_auto, which):
    """6: 360 x 360 cells at 2.5 m (refused by the ground filter) / a NaN x in the first record / a NaN x in a point that reaches the classification (refused
    there); scan 1 of 3 gets what its single call gets, scans 0 and 2 are served, and so is the next call.  The single call SERVES the scan whose first record
    has the NaN (the ground filter never hands that point on: measured, rc 0), so that variant pins the equality with the single call, not a refusal."""
    X = set_d()
    bad = refused_scans()[which]
    want_bad = single(ctx_auto, bad, X)
    if which == "wide":
        assert want_bad[0] == abi.MULLS_E_UNSUPPORTED  # the precondition: its single call refuses it
    if which == "nan_high":
        assert want_bad[0] == abi.MULLS_E_INVALID
    got, stats, rc, blocks = batch(ctx_auto, [scans()["s16"], bad, scans()["classify"]], X)
    assert rc == want_bad[0] and got[1][0] == want_bad[0]
    assert_same(got[1], want_bad, ("refused", which))
    if want_bad[0] != abi.MULLS_OK:
        assert b"scan 1" in ctx_auto.lib.mulls_last_error(ctx_auto.h)
        assert all(blocks[1].cloud(k).n == 0 for k in HELD)  # the refused scan's block is empty
    assert_same(got[0], single_of(ctx_auto, "s16", "D"), "before the refused scan")
    assert_same(got[2], single_of(ctx_auto, "classify", "D"), "behind the refused scan")
    close(blocks)
    again, _, rc, blocks = batch(ctx_auto, [scans()["classify"], scans()["s16"]], X)
    assert rc == abi.MULLS_OK
    assert_same(again[0], single_of(ctx_auto, "classify", "D"), "the next call")
    assert_same(again[1], single_of(ctx_auto, "s16", "D"), "the next call")
    close(blocks)


# ---------------------------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("case", ["voxels", "normals1", "normals2"])
def test_single_scan_path(ctx_auto, case):
    """7: the two parameter points whose scans run alone inside the call (path 1: a sub-batch of one scan each, with the two scan-local steps)"""
    X = {"voxels": lambda: set_d(vf_downsample_resolution=0.5), "normals1": lambda: set_d(ground=abi.ground_params(estimate_ground_normal_method=1)),
         "normals2": lambda: set_d(ground=abi.ground_params(estimate_ground_normal_method=2, min_grid_pt_num=6))}[case]()
    assert 2 * X.ground.min_grid_pt_num <= 64
    names = ["s16", "classify"]
    got, stats, rc, blocks = batch(ctx_auto, [scans()[n] for n in names], X)
    assert rc == abi.MULLS_OK and stats.n_single_path == 2 and stats.n_lockstep == 0
    for name, g in zip(names, got):
        want = single(ctx_auto, scans()[name], X)
        assert want[0] == abi.MULLS_OK and want[1][abi.EX_GROUND] > 0
        assert_same(g, want, (case, name), path=1)
    close(blocks)


# ---------------------------------------------------------------------------------------------------------------------------------- 8
def raw_batch(ctx, clouds, n, X, handles, results=True):
    res = (abi.ExtractBatchResult * max(n, 1))()
    return ctx.lib.mulls_extract_features_batch(ctx.h, clouds, n, C.byref(X), handles, 0, res if results else None, None), res


def test_abi_edges(ctx_auto):
    """8: the refusals that write nothing, the empty batch, a device-resident scan, records 64 bytes apart"""
    X = set_d()
    ctx = ctx_auto
    s16, cl = abi.records(scans()["s16"]), abi.records(scans()["classify"])
    blocks = [lib.Block(ctx).extract(scans()["s16"], X), lib.Block(ctx).extract(scans()["classify"], X)]
    before = [{k: b.download(k) for k in HELD} for b in blocks]

    def untouched():
        return all(np.array_equal(b.download(k), before[i][k]) for i, b in enumerate(blocks) for k in HELD)

    clouds = (abi.Cloud * 2)()
    clouds[0].pts, clouds[0].n, clouds[0].stride = s16.ctypes.data, len(s16), abi.POINT_BYTES
    clouds[1].pts, clouds[1].n, clouds[1].stride = cl.ctypes.data, len(cl), abi.POINT_BYTES
    ok = (C.c_void_p * 2)(blocks[0].h, blocks[1].h)
    assert raw_batch(ctx, clouds, 2, X, (C.c_void_p * 2)(blocks[0].h, None))[0] == abi.MULLS_E_INVALID and untouched()  # a null block
    assert raw_batch(ctx, clouds, 2, X, (C.c_void_p * 2)(blocks[0].h, blocks[0].h))[0] == abi.MULLS_E_INVALID and untouched()  # the same block twice
    assert raw_batch(ctx, None, 2, X, ok)[0] == abi.MULLS_E_INVALID and untouched()  # no scans
    clouds[1].stride = abi.POINT_BYTES - 4
    assert raw_batch(ctx, clouds, 2, X, ok)[0] == abi.MULLS_E_INVALID and untouched()  # records closer together than a record is long
    clouds[1].stride = abi.POINT_BYTES
    assert raw_batch(ctx, None, 0, X, None, results=False)[0] == abi.MULLS_OK and untouched()  # the empty batch
    # a scan of no points among the others: an empty block, MULLS_OK
    got, _, rc, bl = batch(ctx, [scans()["s16"], scans()["s16"][:0]], X)
    assert rc == abi.MULLS_OK and got[1][0] == abi.MULLS_OK and got[1][1] == [0] * abi.EX_COUNT and all(len(got[1][2][k]) == 0 for k in HELD)
    assert_same(got[0], single_of(ctx, "s16", "D"), "beside the empty scan")
    close(bl)
    # a device-resident cloud as a scan: the non-ground cloud of an earlier extraction, against the same records from the host
    dev_cloud = blocks[0].cloud(abi.EX_UNGROUND)
    host_copy = before[0][abi.EX_UNGROUND].copy()
    assert dev_cloud.n == len(host_copy) > 1000
    from_dev, _, rc, b1 = batch(ctx, [dev_cloud, scans()["classify"]], X)
    assert rc == abi.MULLS_OK
    want = single(ctx, host_copy, X)
    assert want[0] == abi.MULLS_OK and want[1][abi.EX_UNGROUND] > 0
    assert_same(from_dev[0], want, "device-resident scan")
    assert_same(from_dev[1], single_of(ctx, "classify", "D"), "beside the device-resident scan")
    close(b1)
    # records 64 bytes apart with random bytes between them
    wide = np.random.default_rng(5).integers(0, 256, (len(s16), 64), dtype=np.uint8)
    wide[:, :abi.POINT_BYTES] = s16
    strided = abi.Cloud()
    strided.pts, strided.n, strided.stride = wide.ctypes.data, len(wide), 64
    got, _, rc, b2 = batch(ctx, [scans()["classify"], strided], X)
    assert rc == abi.MULLS_OK
    assert_same(got[1], single_of(ctx, "s16", "D"), "stride 64")
    assert_same(got[0], single_of(ctx, "classify", "D"), "beside stride 64")
    close(b2)
    close(blocks)


# ---------------------------------------------------------------------------------------------------------------------------------- 9
def test_downstream_registration(ctx_auto):
    """9: the blocks of a batch call feed mulls_icp_batch as the single-extracted blocks do: the same mulls_result, field for field"""
    X = set_k()
    a, b = scans()["s32"], raw_scan(9, 32, 700)

    def register(blk_t, blk_s):
        arr = (abi.Pair * 1)()
        full, down = blk_t.class_clouds(down=False), blk_s.class_clouds(down=True)
        for c in range(abi.NCLASS):
            arr[0].tgt[c], arr[0].src[c] = full[c], down[c]
            arr[0].src_down[c] = abi.as_cloud(None)
        for k, v in enumerate([-200.0, -200.0, -50.0, 200.0, 200.0, 50.0]):
            arr[0].tgt_bound[k] = v
        for k in range(16):
            arr[0].init_guess[k] = 1.0 if k % 5 == 0 else 0.0
        res = abi.make_result_array(1)
        ctx_auto.icp_batch([None], abi.default_params(), marshalled=(arr, res))
        r = res[0]  # every field but the wall time
        return (r.code, r.iters, list(r.T), list(r.info), r.sigma, r.confidence, list(r.ncorr), list(r.nsrc0), list(r.ntgt0), r.singular, r.cropped, list(r.crop_box))

    blocks, results, _ = ctx_auto.extract_features_batch([a, b], X)
    got = register(blocks[0], blocks[1])
    singles = [lib.Block(ctx_auto).extract(a, X), lib.Block(ctx_auto).extract(b, X)]
    want = register(singles[0], singles[1])
    assert singles[1].n[abi.EX_GROUND_DOWN] > 100 and want[1] > 0 and sum(want[6]) > 100  # a registration that iterated on real correspondences
    assert got == want
    close(blocks)
    close(singles)


# ---------------------------------------------------------------------------------------------------------------------------------- 10
def test_single_entry_points_afterwards():
    """10: mulls_extract_features returns after a batch call what it returned before it (arenas, hints, the RANSAC table)"""
    ctx = lib.Context(0)
    for X in (set_d(), set_k()):
        before = ctx.extract_features(scans()["s16"], X)
        _, _, rc, blocks = batch(ctx, [scans()[n] for n in ("s64", "s16", "classify")], X)
        assert rc == abi.MULLS_OK
        after = ctx.extract_features(scans()["s16"], X)
        assert all(np.array_equal(p, q) for p, q in zip(before, after))
        close(blocks)
    ctx.close()
