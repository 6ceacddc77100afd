"""GPU tests of mulls_ncc_correspond_batch through mulls_amd/lib.py: results[b] and the pairs of problem b are the bits of the matching
mulls_ncc_correspond call.

Expected values never come from the batch path: they are the reference's own lines (tests/golden/ncc_demo.npz, ncc_edges.npz through
test_ncc.fixture_cases() / edge_cases()) or the numpy restatement (tests/ncc_restated.py), each computed once per (clouds, mode) and left unchanged; the
chain test's are the chained single calls.  A batch has one mulls_ncc_params, so fixture cases are grouped by (fixed_num_corr, corr_num, reciprocal_on).
Every comparison is equality of integer arrays (the chain: and of every bit of T), as in tests/test_gpu_ncc.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import ncc_restated
from mulls_amd import abi, lib
from test_gpu_teaser import assert_same, device as teaser_single
from test_ncc import FIXTURE, edge_cases, fixture_cases
from test_teaser import INT_KEYS

pytestmark = pytest.mark.gpu

RECIP, NN = (0, 2000, 1), (0, 2000, 0)
ALL_MODES = (RECIP, NN, (1, 300, 0))
MIXED_MODES = (RECIP, NN) + tuple((1, cn, 0) for cn in (1, 300, 2000, 65536))
# (10, 10) .. (63, 65): below a wave, a row block, a chunk; 255 .. 257 x 31 .. 33: the 256-row block and the 32-column floor of a table pass; 1023 .. 1025:
# the 1024 stride of the intensity fold and of the reciprocal compaction; the last two: several row blocks and column chunks
SHAPES = ((10, 10), (11, 64), (63, 65), (255, 31), (256, 32), (257, 33), (1023, 40), (1024, 40), (1025, 40), (1000, 3000), (4097, 513))
FAMILIES = ("plain", "quantised", "bigcodes")


def f32(raw):
    return raw.view(np.float32).reshape(len(raw), 12)


@functools.lru_cache(maxsize=None)
def kpts(seed, n, family="plain"):
    a = ncc_restated.random_kpts(seed, n, family)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def shape_clouds(k):
    nt, ns = SHAPES[k]
    return kpts(100 + k, nt, FAMILIES[k % 3]), kpts(200 + k, ns, FAMILIES[k % 3])


_want = {}


def want(t, s, mode):
    """(ok, pairs) of the restatement, once per (clouds, mode); the clouds are told apart by their bytes' address and size (they are kept alive by the caches)"""
    key = (t.ctypes.data, len(t), s.ctypes.data, len(s), mode)
    if key not in _want:
        _want[key] = (t, s, ncc_restated.restate(t, s, *mode))
    return _want[key][2]


def run(ctx, problems, mode, limit=0):
    return ctx.ncc_correspond_batch(problems, abi.ncc_params(*mode), limit)


def assert_problem(got, ok, pairs, what, cap=None):
    got_ok, ti, si, n = got
    assert got_ok == ok and n == len(pairs), (what, got_ok, n, len(pairs))
    w = len(pairs) if cap is None else min(cap, len(pairs))
    assert np.array_equal(np.stack([ti, si], 1).astype(np.int64), pairs[:w]), what


def check(ctx, clouds, mode, what, limit=0):
    got = run(ctx, clouds, mode, limit)
    assert len(got) == len(clouds)
    for b, (t, s) in enumerate(clouds):
        ok, pairs = want(t, s, mode)
        assert_problem(got[b], ok, pairs, (what, b, len(t), len(s), mode))


def test_fixtures_batched_per_parameter_group(ctx_auto):
    """the ten ncc_demo.npz cases and the 33 of ncc_edges.npz, one batch per (fixed_num_corr, corr_num, reciprocal_on), against the stored pairs"""
    groups, seen = {}, 0
    for name, t, s, fixed, cn, recip, ok, pairs, _ in fixture_cases():
        groups.setdefault((fixed, cn, recip), []).append((name, t, s, ok, pairs))
    assert sum(len(g) for g in groups.values()) == 10
    for name, t, s, fixed, cn, recip, ok, pairs in edge_cases():
        groups.setdefault((fixed, cn, recip), []).append((name, t, s, ok, pairs))
    assert sum(len(g) for g in groups.values()) == 43 and max(len(g) for g in groups.values()) > 4
    for mode, cases in groups.items():
        got = run(ctx_auto, [(c[1], c[2]) for c in cases], mode)
        for g, (name, _, _, ok, pairs) in zip(got, cases):
            assert_problem(g, ok, pairs, name)
            seen += 1
    assert seen == 43


@pytest.mark.parametrize("mode", MIXED_MODES, ids=lambda m: "recip" if m == RECIP else "nn" if m == NN else "fixed%d" % m[1])
def test_mixed_sizes_in_one_launch(ctx_auto, mode):
    """every shape in one launch of every kernel, forward and reversed; and with scratch_limit = 1: one problem per sub-batch"""
    clouds = [shape_clouds(k) for k in range(len(SHAPES))]
    assert [(len(t), len(s)) for t, s in clouds] == list(SHAPES)
    check(ctx_auto, clouds, mode, "forward")
    check(ctx_auto, clouds[::-1], mode, "reversed")
    check(ctx_auto, clouds, mode, "one per sub-batch", limit=1)


def state_batch():
    """ordinary problems around: a NaN target intensity at the last index; a constant target intensity; 9 targets; a table smaller than corr_num = 300 beside
    one that is not"""
    plain = [(kpts(301, 257), kpts(302, 33)), (kpts(303, 120, "quantised"), kpts(304, 90, "quantised")), (kpts(305, 63), kpts(306, 65))]
    nan_last = kpts(307, 300).copy()
    f32(nan_last)[-1, 8] = np.nan
    const = kpts(308, 500).copy()
    f32(const)[:, 8] = 7.0
    few = kpts(309, 9)
    small = (kpts(310, 10), kpts(311, 12))
    s = kpts(312, 400)
    for a in (nan_last, const):
        a.setflags(write=False)
    return [plain[0], (nan_last, s), plain[1], (const, s), (few, s), plain[2], small, (kpts(313, 63), kpts(314, 65))]


STATE = functools.lru_cache(maxsize=None)(state_batch)


@pytest.mark.parametrize("mode", ALL_MODES, ids=("recip", "nn", "fixed300"))
def test_per_problem_state_does_not_leak(ctx_auto, mode):
    clouds = STATE()
    # the properties this test is about, on the restatement
    for b in (1, 3):  # NaN range (the last target's intensity), collapsed range: every distance is a NaN
        t, s = clouds[b]
        lo, hi = ncc_restated.intensity_range(ncc_restated.fields(t)["inten"])
        dt = ncc_restated.table(ncc_restated.descriptors(t, lo, hi), ncc_restated.descriptors(s, lo, hi))
        assert np.isnan(dt).all()
        ok, pairs = want(t, s, mode)
        assert ok and (len(pairs) == 0 if mode[0] else np.array_equal(pairs, np.stack([np.arange(len(t)), np.zeros(len(t), np.int64)], 1)))
    ok, pairs = want(*clouds[4], mode)
    assert ok is False and len(pairs) == 0 and len(clouds[4][0]) == 9  # 9 targets in the middle of the batch: the reference's `false`
    assert len(clouds[6][0]) * len(clouds[6][1]) < 300 < len(clouds[7][0]) * len(clouds[7][1])
    check(ctx_auto, clouds, mode, "state")
    check(ctx_auto, clouds[::-1], mode, "state reversed")


def test_lock_step_mask(ctx_auto):
    """a problem that needs the flat-index levels beside problems that are done after the three distance levels, in both orders"""
    K = 300
    tied = (kpts(401, 120, "quantised"), kpts(402, 90, "quantised"))
    plains = [(kpts(403, 257), kpts(404, 100)), (kpts(405, 64), kpts(406, 700))]

    def rank_class(t, s):
        lo, hi = ncc_restated.intensity_range(ncc_restated.fields(t)["inten"])
        flat = ncc_restated.table(ncc_restated.descriptors(t, lo, hi), ncc_restated.descriptors(s, lo, hi)).reshape(-1)
        assert not np.isnan(flat).any() and len(flat) > K
        dK = np.partition(flat, K - 1)[K - 1]
        return K - int((flat < dK).sum()), int((flat == dK).sum())  # entries still to take at the rank-K distance, entries that have it

    left, ties = rank_class(*tied)
    assert 0 < left < ties, (left, ties)  # shared by more entries than fit: levels 3-5 decide
    for p in plains:
        left, ties = rank_class(*p)
        assert left == ties  # the whole class is taken: done after level 2
    mode = (1, K, 0)
    for clouds in ([plains[0], tied, plains[1]], [tied, plains[0], plains[1]], [plains[1], plains[0], tied], [tied, tied, plains[0], tied]):
        check(ctx_auto, clouds, mode, "lock-step")


def hip_runtime():
    """the HIP runtime the library brought into this process"""
    lib.load()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise AssertionError("libamdhip64 is not mapped")


def test_shared_and_mixed_memory(ctx_auto):
    s = kpts(501, 700)
    targets = [kpts(510 + k, n) for k, n in enumerate((300, 301, 1023, 1024, 1025, 64, 2000, 10))]
    for mode in ALL_MODES:  # one source cloud under eight targets, the same pointer
        got = run(ctx_auto, [(t, s) for t in targets], mode)
        for g, t in zip(got, targets):
            assert_problem(g, *want(t, s, mode), ("shared source", len(t), mode))
        got = run(ctx_auto, [(s, t) for t in targets], mode)  # ... and one target over eight sources
        for g, t in zip(got, targets):
            assert_problem(g, *want(s, t, mode), ("shared target", len(t), mode))
    # host clouds of strides 36, 48 and 64 beside a caller-owned device cloud and a pinned host cloud
    from test_gpu_ncc import strided

    t, u = kpts(520, 1500), kpts(521, 1100)
    hip = hip_runtime()
    dev, pin = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(t.nbytes)) == 0 and hip.hipHostMalloc(C.byref(pin), C.c_size_t(u.nbytes), C.c_uint(0)) == 0
    try:
        assert hip.hipMemcpy(dev, C.c_void_p(t.ctypes.data), C.c_size_t(t.nbytes), C.c_int(1)) == 0  # hipMemcpyHostToDevice
        C.memmove(pin, u.ctypes.data, u.nbytes)

        def cloud(ptr, n):
            c = abi.Cloud()
            c.pts, c.n, c.stride = ptr.value, n, 48
            return c

        D, P = cloud(dev, len(t)), cloud(pin, len(u))
        (b36, c36), (b64, c64) = strided(np.asarray(u), 36, 1), strided(np.asarray(t), 64, 2)
        problems = [(c64, c36), (D, u), (t, P), (D, P), (c64, u), (D, c36), (t, u)]
        for mode in ALL_MODES:
            ok, pairs = want(t, u, mode)
            got = run(ctx_auto, problems, mode)
            for b, g in enumerate(got):
                assert_problem(g, ok, pairs, ("mixed memory", b, mode))
            # a cap below the count: the full count reported, cap pairs written, nothing behind them (lib.py checks the slot behind cap)
            assert len(pairs) > 17
            got = run(ctx_auto, [dict(tgt=D, src=u, cap=17), dict(tgt=t, src=u), dict(tgt=c64, src=P, cap=0)], mode)
            assert_problem(got[0], ok, pairs, ("cap 17", mode), cap=17)
            assert_problem(got[1], ok, pairs, ("beside cap", mode))
            assert_problem(got[2], ok, pairs, ("cap 0", mode), cap=0)
            assert len(got[0][1]) == 17 and len(got[2][1]) == 0
    finally:
        assert hip.hipFree(dev) == 0 and hip.hipHostFree(pin) == 0


def test_refusals_leave_every_result_at_zero(ctx_auto):
    L = lib.load()
    t, s = kpts(601, 500), kpts(602, 400)
    bad = np.zeros((500, 50), np.uint8)

    def records(n, fill=None):
        arr, res, idx = (abi.NccProblem * max(n, 1))(), (abi.NccResult * max(n, 1))(), np.full((max(n, 1), 2, 8), -7, np.int32)
        for b in range(n):
            arr[b].tgt.pts, arr[b].tgt.n, arr[b].tgt.stride = t.ctypes.data, len(t), 48
            arr[b].src.pts, arr[b].src.n, arr[b].src.stride = s.ctypes.data, len(s), 48
            arr[b].tgt_idx, arr[b].src_idx, arr[b].cap = idx[b, 0].ctypes.data, idx[b, 1].ctypes.data, 8
            res[b].ret, res[b].n_corr = 7, 7
        return arr, res, idx

    def refused(arr, res, idx, n, P, code, names=None):
        assert L.mulls_ncc_correspond_batch(ctx_auto.h, arr, n, C.byref(P) if P is not None else None, 0, res) == code
        assert all(res[b].ret == 0 and res[b].n_corr == 0 for b in range(n)) and (idx == -7).all()
        if names is not None:
            assert ("problem %d" % names) in L.mulls_last_error(ctx_auto.h).decode()

    for mode in ALL_MODES:  # a bad stride in problem 3 of 5: the single call's MULLS_E_INVALID
        arr, res, idx = records(5)
        arr[3].tgt.pts, arr[3].tgt.stride = bad.ctypes.data, 50
        refused(arr, res, idx, 5, abi.ncc_params(*mode), abi.MULLS_E_INVALID, 3)
        n = C.c_uint32(9)
        assert L.mulls_ncc_correspond(ctx_auto.h, C.byref(arr[3].tgt), C.byref(arr[3].src), C.byref(abi.ncc_params(*mode)), arr[3].tgt_idx, arr[3].src_idx, 8,
                                      C.byref(n)) == abi.MULLS_E_INVALID
    arr, res, idx = records(4)
    refused(arr, res, idx, 4, abi.ncc_params(1, 65537, 0), abi.MULLS_E_UNSUPPORTED, 0)
    arr, res, idx = records(4)
    arr[2].src_idx = None  # a NULL index buffer with cap > 0
    refused(arr, res, idx, 4, abi.ncc_params(), abi.MULLS_E_INVALID, 2)
    arr, res, idx = records(3)
    refused(arr, res, idx, 3, None, abi.MULLS_E_INVALID)  # NULL params
    arr, res, idx = records(2)
    assert L.mulls_ncc_correspond_batch(ctx_auto.h, arr, 0, C.byref(abi.ncc_params()), 0, res) == abi.MULLS_OK  # n_problems = 0
    assert res[0].ret == 7 and ctx_auto.ncc_correspond_batch([]) == []
    # fixed-number mode with corr_num <= 0: the reference's `true` without a pair, per problem; the context goes on
    for cn in (0, -5):
        got = run(ctx_auto, [(t, s), (t[:9], s), (s, t)], (1, cn, 0))
        assert [(g[0], g[3], len(g[1])) for g in got] == [(True, 0, 0), (False, 0, 0), (True, 0, 0)]
    check(ctx_auto, [(t, s), (s, t)], RECIP, "after the refusals")


def test_repetition_on_one_context(ctx_auto):
    """the mixed batch, a batch of one small problem, the mixed batch again: the grow-only arena and the per-call clears of sel, hist and cand"""
    mixed = [shape_clouds(k) for k in (9, 2, 5, 8, 10, 0)]
    small = [(kpts(303, 120, "quantised"), kpts(304, 90, "quantised"))]
    for mode in ALL_MODES + ((1, 65536, 0),):
        check(ctx_auto, mixed, mode, "first")
        check(ctx_auto, small, mode, "small")
        check(ctx_auto, mixed, mode, "again")
        check(ctx_auto, small, mode, "small again")


def test_chain_into_the_teaser_batch(ctx_auto):
    """ncc_correspond_batch -> coarse_reg_teaser_batch on the demo key points (scans 0 / 15, both directions, twice) at the noise bound 0.25: every
    integer and every bit of T of the chained single calls ncc_correspond -> coarse_reg_teaser(tgt_idx=..., src_idx=...)"""
    Z = np.load(FIXTURE)
    a, b = Z["kpts_0"], Z["kpts_15"]
    clouds = [(a, b), (b, a), (a, b), (b, a)]
    for mode in (RECIP, (1, 300, 0)):
        singles = []
        for t, s in clouds[:2]:
            ok, ti, si, n = ctx_auto.ncc_correspond(t, s, abi.ncc_params(*mode))
            assert ok and n == len(ti) > 100
            singles.append((ti, si, teaser_single(ctx_auto, t, s, 0.25, tgt_idx=ti, src_idx=si)))
        lists = run(ctx_auto, clouds, mode)
        for k, (ok, ti, si, n) in enumerate(lists):
            assert ok and n == len(ti) and np.array_equal(ti, singles[k % 2][0]) and np.array_equal(si, singles[k % 2][1]), (mode, k)
        solved = ctx_auto.coarse_reg_teaser_batch([(t, s, ti, si) for (t, s), (_, ti, si, _) in zip(clouds, lists)], abi.teaser_params(0.25))
        for k, (res, clique) in enumerate(solved):
            got = {key: int(getattr(res, key)) for key in INT_KEYS}
            got.update(cost=float(res.cost), T=np.array(res.T[:], np.float64).reshape(4, 4).T.copy(), clique=clique.astype(np.int64))
            assert_same(got, singles[k % 2][2], (mode, k))
        assert singles[0][2]["status"] >= 0
