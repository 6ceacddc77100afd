"""The single calls of the feature stage as batches of one (mulls_amd/csrc/extract_batch.cpp): mulls_extract_features_resident, mulls_extract_features,
mulls_ground_filter, mulls_classify_nground and mulls_voxel_downsample share one device arena, one pinned scratch, the round counters and the round hints with
mulls_extract_features_batch.  What is pinned here: no call leaves anything there that changes another's bytes; the two scan-local steps (voxel down-sampling, ground
normals by method 1 / 2) inside a batch; the host outputs at their capacities; return codes and messages of the refusals, as literals.
Scans: one synthetic scan (mulls_amd/synth.py) subsampled to 0, 9, 300, 4 097 (one point past a 4 096-point compaction segment) and 20 000 points; 9 is below the
10 points under which a class skips the suppression."""
import ctypes as C
import functools

import numpy as np
import pytest

from mulls_amd import abi, lib
from oracle import pyoracle

from test_gpu_extract_batch import HELD, assert_same, batch, close, raw_scan, single

pytestmark = pytest.mark.gpu

SIZES = [0, 9, 300, 4097, 20000]


@functools.lru_cache(maxsize=None)
def scan(n):
    """n returns of one 64 x 600 scan, evenly spread over it, as (n, 48) uint8 records"""
    full = abi.records(raw_scan(8, 64, 600))
    assert len(full) > 20000
    return np.ascontiguousarray(full[np.linspace(0, len(full) - 1, n).astype(np.int64)] if n else full[:0])


def thin_classify(**kw):
    """every fixed-number sampler of the classification has something to cut on the 4 097- and 20 000-point scans wherever the scan has the class at all
    (test_one_arena_many_callers asserts it; the synthetic scenes have no roofs, so the roof sampler sees an empty cloud)"""
    return abi.classify_params(fixed_num_downsampling=1, unground_down_fixed_num=500, pillar_down_fixed_num=4, beam_down_fixed_num=4, facade_down_fixed_num=8,
                               roof_down_fixed_num=4, **kw)


def thin_params():
    return abi.extract_params(ground=abi.ground_params(estimate_ground_normal_method=3, fixed_num_downsampling=1, down_ground_fixed_num=100), classify=thin_classify(),
                              apply_dist_filter=1, min_dist_used=5.0, max_dist_used=60.0)


def classify_strided(ctx, recs, P, stride=64):
    """mulls_classify_nground on host records `stride` bytes apart: (rc, sizes, the nine clouds, cloud_in as the call leaves it)"""
    n = len(recs)
    wide = np.full((max(n, 1), stride), 0xEE, np.uint8)
    wide[:n, : abi.POINT_BYTES] = recs
    outs = [np.zeros((max(n, 1), abi.POINT_BYTES), np.uint8) for _ in range(abi.CL_COUNT)]
    out_p = (C.c_void_p * abi.CL_COUNT)(*[o.ctypes.data for o in outs])
    cap = (C.c_uint32 * abi.CL_COUNT)(*([n] * abi.CL_COUNT))
    nout, after, n_after = (C.c_uint32 * abi.CL_COUNT)(), np.zeros((max(n, 1), abi.POINT_BYTES), np.uint8), C.c_uint32(0)
    rc = ctx.lib.mulls_classify_nground(ctx.h, wide.ctypes.data_as(C.c_void_p), n, stride, C.byref(P), out_p, cap, nout, after.ctypes.data_as(C.c_void_p), C.byref(n_after))
    return rc, list(nout), [outs[k][: nout[k]].copy() for k in range(abi.CL_COUNT)], after[: n_after.value].copy()


def same(a, b):
    """byte-for-byte equality of nested results (codes, size lists, record arrays)"""
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


# ------------------------------------------------------------------------------------------------------------------------------------ 1
def test_one_arena_many_callers():
    """Six calls of five entry points in a row on one context; every output equals the same call on a context of its own.  The order makes each call meet what
    a larger or differently shaped one left: the arena, the pinned words, the 64 round counters, the two round hints, the context-owned block."""
    X = thin_params()
    # the samplers have work: against the same chain with class numbers nothing reaches, every *_down cloud the two large scans have shrinks, and cloud_in is thinned
    loose = thin_params()
    loose.classify.pillar_down_fixed_num = loose.classify.beam_down_fixed_num = loose.classify.facade_down_fixed_num = loose.classify.roof_down_fixed_num = 100000
    for n in (4097, 20000):
        a, b = pyoracle.extract_features(scan(n), X), pyoracle.extract_features(scan(n), loose)
        assert len(a[abi.EX_UNGROUND]) == 500 and len(a[abi.EX_RAW]) < n
        down = range(abi.EX_PILLAR + abi.CL_PILLAR_DOWN, abi.EX_PILLAR + abi.CL_ROOF_DOWN + 1)
        assert all(len(b[k]) == 0 or len(a[k]) < len(b[k]) for k in down) and sum(len(b[k]) > 0 for k in down) == 3, [(len(a[k]), len(b[k])) for k in down]

    def calls(ctx):
        yield "resident 20000", lambda: single(ctx, scan(20000), X)
        yield "batch of five", lambda: batch_of_five(ctx)
        yield "classify 20000, stride 64", lambda: classify_strided(ctx, scan(20000), X.classify)
        yield "ground filter 300", lambda: ctx.ground_filter(abi.points_of(scan(300)), X.ground)
        yield "voxels 4097", lambda: ctx.voxel_downsample(scan(4097), 0.2)
        yield "host output 4097", lambda: ctx.extract_features(scan(4097), X)

    def batch_of_five(ctx):
        got, stats, rc, blocks = batch(ctx, [scan(n) for n in SIZES], X)
        close(blocks)
        return rc, [g[:3] for g in got], (stats.n_subbatches, stats.n_lockstep, stats.n_single_path)

    shared = lib.Context(0)
    try:
        in_a_row = [(name, fn()) for name, fn in calls(shared)]
    finally:
        shared.close()
    for i, (name, got) in enumerate(in_a_row):
        fresh = lib.Context(0)
        try:
            want = list(calls(fresh))[i][1]()
        finally:
            fresh.close()
        assert same(got, want), name
    rc, five, counts = in_a_row[1][1]
    assert rc == abi.MULLS_OK and counts == (1, 5, 0) and all(g[0] == abi.MULLS_OK for g in five)
    assert five[0][1] == [0] * abi.EX_COUNT and five[4][1] == in_a_row[0][1][1]  # the empty scan; the 20 000-point scan as its single call
    assert in_a_row[2][1][0] == abi.MULLS_OK and len(in_a_row[2][1][3]) == 500


# ------------------------------------------------------------------------------------------------------------------------------------ 2
def scan_local_params(case):
    return {"voxels": lambda: abi.extract_params(vf_downsample_resolution=0.2), "normals1": lambda: abi.extract_params(ground=abi.ground_params(estimate_ground_normal_method=1)),
            "normals2": lambda: abi.extract_params(ground=abi.ground_params(estimate_ground_normal_method=2, min_grid_pt_num=6))}[case]()


@pytest.mark.parametrize("case", ["voxels", "normals1", "normals2"])
def test_scan_local_steps_inside_a_batch(ctx_auto, case):
    """voxel down-sampling / ground normals by method 1 and 2 have no table form: every scan of such a batch is a sub-batch of its own (path 1).  An empty scan and
    a scan that is refused before anything is uploaded (500 001 points) sit between the two that run."""
    X = scan_local_params(case)
    too_many = np.zeros((500001, abi.POINT_BYTES), np.uint8)
    got, stats, rc, blocks = batch(ctx_auto, [scan(4097), scan(0), too_many, scan(300)], X)
    assert all(g[3] == 1 for g in got)
    assert stats.n_single_path == 4 and stats.n_lockstep == 0
    assert got[1][0] == abi.MULLS_OK and got[1][1] == [0] * abi.EX_COUNT and all(blocks[1].cloud(k).n == 0 for k in HELD)
    assert rc == abi.MULLS_E_UNSUPPORTED and got[2][0] == abi.MULLS_E_UNSUPPORTED and all(blocks[2].cloud(k).n == 0 for k in HELD)
    assert b"scan 2: mulls_ground_filter: more than 500000 points in one scan" in ctx_auto.lib.mulls_last_error(ctx_auto.h)
    for i, n in ((0, 4097), (3, 300)):
        want = single(ctx_auto, scan(n), X)
        assert want[0] == abi.MULLS_OK and want[1][abi.EX_GROUND] > 0
        assert_same(got[i], want, (case, n), path=1)
        oracle = pyoracle.extract_features(scan(n), X)
        assert got[i][1] == [len(o) for o in oracle], (case, n, got[i][1])
        for k in HELD:
            assert np.array_equal(got[i][2][k], oracle[k]), (case, n, k)
        if case == "voxels":
            assert got[i][1][abi.EX_DOWN] <= got[i][1][abi.EX_RAW] == n and (n == 300 or got[i][1][abi.EX_DOWN] < n)  # (the 300 returns lie a voxel and more apart)
    close(blocks)


# ------------------------------------------------------------------------------------------------------------------------------------ 3
def test_host_output_at_its_capacities(ctx_auto):
    """mulls_extract_features with the distance filter and the voxel grid ahead of the ground filter: RAW and DOWN come from where the chain has them, the other
    clouds from the context's block.  Capacities one below the size cut the records, not the sizes; cloud_in (UNGROUND) comes back whole or not at all."""
    X = abi.extract_params(apply_dist_filter=1, min_dist_used=5.0, max_dist_used=60.0, vf_downsample_resolution=0.2)
    recs = scan(4097)
    want = pyoracle.extract_features(recs, X)
    full = ctx_auto.extract_features(recs, X)
    for k in range(abi.EX_COUNT):
        assert np.array_equal(full[k], want[k]), k
    sizes = [len(w) for w in want]
    cut = (abi.EX_RAW, abi.EX_DOWN, abi.EX_GROUND, abi.EX_PILLAR)
    assert all(sizes[k] >= 2 for k in cut) and sizes[abi.EX_DOWN] < sizes[abi.EX_RAW] < 4097 and sizes[abi.EX_UNGROUND] >= 2
    for unground_cap in (sizes[abi.EX_UNGROUND], sizes[abi.EX_UNGROUND] - 1):
        caps = [s - 1 if k in cut else s for k, s in enumerate(sizes)]
        caps[abi.EX_UNGROUND] = unground_cap
        outs = [np.full((s + 1, abi.POINT_BYTES), 0xAB, np.uint8) for s in sizes]
        out_p = (C.c_void_p * abi.EX_COUNT)(*[o.ctypes.data for o in outs])
        nout = (C.c_uint32 * abi.EX_COUNT)()
        rc = ctx_auto.lib.mulls_extract_features(ctx_auto.h, recs.ctypes.data_as(C.c_void_p), len(recs), abi.POINT_BYTES, C.byref(X), out_p, (C.c_uint32 * abi.EX_COUNT)(*caps), nout)
        assert rc == abi.MULLS_OK and list(nout) == sizes  # the sizes in full
        for k in range(abi.EX_COUNT):
            written = caps[k] if k != abi.EX_UNGROUND or unground_cap == sizes[k] else 0
            assert np.array_equal(outs[k][:written], want[k][:written]), (k, unground_cap)
            assert np.all(outs[k][written:] == 0xAB), (k, unground_cap)  # nothing behind the capacity; a cloud_in that does not fit whole is not written


# ------------------------------------------------------------------------------------------------------------------------------------ 4
GRID = b"mulls_ground_filter: the grid has too many cells (more than 65536, or more than 64 M table entries: grid_resolution too fine for this scan's extent)"
NONFINITE = b"mulls_classify_nground: the cloud has non-finite coordinates"
NEIGHBOR_K = b"mulls_classify_nground: pca_down_rate >= 1, 1 <= neighbor_k <= 64 and a positive radius are required"
METHOD2 = b"mulls_ground_filter: normal method 2 searches 2 * min_grid_pt_num neighbours, at most 64"


def test_refusals_keep_their_codes_and_messages(ctx_auto):
    """one refusal and more per single entry point: the return code and the text of mulls_last_error, which name the stage that refuses, not the entry point"""
    L, h, recs = ctx_auto.lib, ctx_auto.h, scan(4097)
    p, n = recs.ctypes.data_as(C.c_void_p), len(recs)
    nout, n3, n_after = (C.c_uint32 * abi.EX_COUNT)(), (C.c_uint32 * 3)(), C.c_uint32(0)
    outs = [np.zeros((n, abi.POINT_BYTES), np.uint8) for _ in range(abi.EX_COUNT)]
    out_p, cap = (C.c_void_p * abi.EX_COUNT)(*[o.ctypes.data for o in outs]), (C.c_uint32 * abi.EX_COUNT)(*([n] * abi.EX_COUNT))
    vp = lambda k: outs[k].ctypes.data_as(C.c_void_p)  # noqa: E731
    blk = lib.Block(ctx_auto)
    fine = abi.extract_params(ground=abi.ground_params(grid_resolution=0.05))
    k65 = abi.extract_params(classify=abi.classify_params(neighbor_k=65))
    m2 = abi.ground_params(estimate_ground_normal_method=2, min_grid_pt_num=33)
    # a NaN that reaches the classification: every non-ground point is handed on (rate 1), and the point lies above the ground threshold
    every = abi.extract_params(ground=abi.ground_params(nonground_random_down_rate=1))
    nan = abi.points_of(recs).copy()
    nan["x"][int(np.argmax(nan["z"]))] = np.nan
    nan = abi.records(nan)
    pn = nan.ctypes.data_as(C.c_void_p)

    def resident(X, q=p):
        return L.mulls_extract_features_resident(h, q, n, abi.POINT_BYTES, C.byref(X), blk.h, nout)

    def host(X, q=p):
        return L.mulls_extract_features(h, q, n, abi.POINT_BYTES, C.byref(X), out_p, cap, nout)

    def ground(P):
        return L.mulls_ground_filter(h, p, n, abi.POINT_BYTES, C.byref(P), vp(1), n, vp(2), n, vp(3), n, n3)

    def classify(P, q=p):
        return L.mulls_classify_nground(h, q, n, abi.POINT_BYTES, C.byref(P), out_p, cap, nout, None, C.byref(n_after))

    for what, call, code, text in (("resident, grid", lambda: resident(fine), abi.MULLS_E_UNSUPPORTED, GRID), ("resident, NaN", lambda: resident(every, pn), abi.MULLS_E_INVALID, NONFINITE),
                                   ("resident, k 65", lambda: resident(k65), abi.MULLS_E_INVALID, NEIGHBOR_K), ("resident, method 2", lambda: resident(abi.extract_params(ground=m2)), abi.MULLS_E_UNSUPPORTED, METHOD2),
                                   ("host, grid", lambda: host(fine), abi.MULLS_E_UNSUPPORTED, GRID), ("host, NaN", lambda: host(every, pn), abi.MULLS_E_INVALID, NONFINITE),
                                   ("host, k 65", lambda: host(k65), abi.MULLS_E_INVALID, NEIGHBOR_K), ("ground filter, grid", lambda: ground(fine.ground), abi.MULLS_E_UNSUPPORTED, GRID),
                                   ("ground filter, method 2", lambda: ground(m2), abi.MULLS_E_UNSUPPORTED, METHOD2), ("classify, k 65", lambda: classify(k65.classify), abi.MULLS_E_INVALID, NEIGHBOR_K),
                                   ("classify, NaN", lambda: classify(every.classify, pn), abi.MULLS_E_INVALID, NONFINITE)):
        assert call() == code, what
        assert L.mulls_last_error(h) == text, (what, L.mulls_last_error(h))
        if what.startswith("resident"):
            assert all(blk.cloud(k).n == 0 for k in HELD), what  # a refused scan leaves its block at zero sizes
    assert resident(abi.extract_params()) == abi.MULLS_OK and nout[abi.EX_GROUND] > 0  # and the context serves the next call
    blk.close()
