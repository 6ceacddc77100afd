"""GPU tests of mulls_ncc_correspond (find_feature_correspondence_ncc, include/common/cregistration.hpp:409-601) through mulls_amd/lib.py: the index
pairs against what the reference's own lines returned on its demo scans (fixture tests/golden/ncc_demo.npz) and against the numpy restatement
(tests/ncc_restated.py, equal to those lines on the fixture: tests/test_ncc.py) on seeded random key points.  Every comparison is equality of integer
arrays.

Below the first tests, the edges: what the reference's lines return on the synthetic sets of tests/golden/ncc_edges.npz; NaN / infinite / negative target
intensities around the 1024-thread stride of the intensity fold; the fixed-number selection's flat-index digits on tables of up to 2^31 - 2^16 entries
("far prefix" inputs, see far_prefix()); row and column counts around the 1024-row chunk of the reciprocal pass and the 32-column floor of a table pass;
host strides other than 48, caller-owned device memory and pinned host memory; the scratch after the largest table."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import ncc_restated
from mulls_amd import abi, lib
from test_ncc import FIXTURE, edge_cases, fixture_cases

pytestmark = pytest.mark.gpu

MODES = ((0, 2000, 1), (0, 2000, 0))  # (fixed_num_corr, corr_num, reciprocal_on): reciprocal nearest neighbour, nearest neighbour
CORR_NUMS = (1, 300, 2000, 65536)


def device_pairs(ctx, t, s, fixed, corr_num, recip, cap=None):
    ok, ti, si, n = ctx.ncc_correspond(t, s, abi.ncc_params(fixed, corr_num, recip), cap)
    assert n == len(ti) or cap is not None
    return ok, np.stack([ti, si], 1).astype(np.int64), n


def check(ctx, t, s, fixed, corr_num, recip, what):
    ok, want = ncc_restated.restate(t, s, fixed, corr_num, recip)
    got_ok, got, n = device_pairs(ctx, t, s, fixed, corr_num, recip)
    assert got_ok == ok and n == len(want), (what, n, len(want))
    assert np.array_equal(got, want), what
    return want


def test_fixture_device_equals_reference_lines(ctx_auto):
    seen = 0
    for name, t, s, fixed, cn, recip, ok, pairs, _ in fixture_cases():
        got_ok, got, n = device_pairs(ctx_auto, t, s, fixed, cn, recip)
        assert got_ok == ok and n == len(pairs), (name, n, len(pairs))
        assert np.array_equal(got, pairs), name
        seen += 1
    assert seen == 10


@pytest.mark.parametrize("family", ["plain", "quantised", "bigcodes"])
@pytest.mark.parametrize("nt,ns", [(10, 10), (11, 64), (63, 65), (257, 1000), (1000, 3000), (4097, 513)])
def test_random_key_points_against_restatement(ctx_auto, nt, ns, family):
    t, s = ncc_restated.random_kpts(1000 + nt, nt, family), ncc_restated.random_kpts(2000 + ns, ns, family)
    for fixed, cn, recip in MODES:
        check(ctx_auto, t, s, fixed, cn, recip, (nt, ns, family, "recip" if recip else "nn"))
    nums = list(CORR_NUMS) + ([nt * ns + 1] if nt * ns + 1 <= 65536 else [])  # ... and more than the table holds
    for cn in nums:
        want = check(ctx_auto, t, s, 1, cn, 1, (nt, ns, family, "fixed", cn))
        assert len(want) <= min(cn, nt * ns)
    if family == "quantised" and nt * ns >= 4095:
        # equal distances are the rule here: this is what pins "lowest j" and "lowest flat index"
        imin, imax = ncc_restated.intensity_range(ncc_restated.fields(t)["inten"])
        dt = ncc_restated.table(ncc_restated.descriptors(t, imin, imax), ncc_restated.descriptors(s, imin, imax))
        assert ((dt == dt.min(1)[:, None]).sum(1) > 1).mean() > 0.4 and len(np.unique(dt)) < 100


def test_large_table_is_never_stored(ctx_auto):
    """16 384 x 12 288 key points in the two nearest-neighbour modes: 201 M distances, the column range split over workgroups"""
    t, s = ncc_restated.random_kpts(31, 16384), ncc_restated.random_kpts(32, 12288)
    for fixed, cn, recip in MODES:
        check(ctx_auto, t, s, fixed, cn, recip, ("large", recip))


def test_degenerate_inputs_and_refusals(ctx_auto):
    t, s = ncc_restated.random_kpts(41, 500), ncc_restated.random_kpts(42, 400)
    for a, b in ((t[:9], s), (t, s[:9])):
        for fixed in (0, 1):
            ok, got, n = device_pairs(ctx_auto, a, b, fixed, 300, 1)
            assert ok is False and n == 0 and len(got) == 0  # the reference's `false`
    const = t.copy()
    const.view(np.float32).reshape(len(const), 12)[:, 8] = 7.0  # constant target intensity: every distance is a NaN
    ok, got, n = device_pairs(ctx_auto, const, s, 0, 2000, 1)
    assert ok and np.array_equal(got, np.stack([np.arange(500), np.zeros(500, np.int64)], 1))
    ok, got, n = device_pairs(ctx_auto, const, s, 1, 2000, 0)
    assert ok and n == 0
    for cn in (0, -5):
        ok, got, n = device_pairs(ctx_auto, t, s, 1, cn, 0)
        assert ok and n == 0
    # cap below the count: the full count reported, cap pairs written, nothing past them (lib.py checks the slot behind cap)
    for fixed, cn, recip in ((0, 2000, 0), (0, 2000, 1), (1, 300, 0)):
        _, want = ncc_restated.restate(t, s, fixed, cn, recip)
        ok, got, n = device_pairs(ctx_auto, t, s, fixed, cn, recip, cap=17)
        assert ok and n == len(want) > 17 and np.array_equal(got, want[:17])
        ok, got, n = device_pairs(ctx_auto, t, s, fixed, cn, recip, cap=0)
        assert ok and n == len(want) and len(got) == 0
    # refusals
    L, n = lib.load(), C.c_uint32(9)
    ct, cs, P = abi.Cloud(), abi.Cloud(), abi.ncc_params(1, 65537, 0)
    ct.pts, ct.n, ct.stride = t.ctypes.data, len(t), 48
    cs.pts, cs.n, cs.stride = s.ctypes.data, len(s), 48
    idx = np.zeros(8, np.int32)
    ip = idx.ctypes.data_as(C.c_void_p)
    assert L.mulls_ncc_correspond(ctx_auto.h, C.byref(ct), C.byref(cs), C.byref(P), ip, ip, 4, C.byref(n)) == abi.MULLS_E_UNSUPPORTED and n.value == 0
    big_t, big_s = np.zeros((65536, 48), np.uint8), np.zeros((32768, 48), np.uint8)  # 2^31 table entries: one more than upstream's int index holds
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.ncc_correspond(big_t, big_s, abi.ncc_params(1, 300, 0), cap=4)
    assert e.value.args[1] == abi.MULLS_E_UNSUPPORTED
    P = abi.ncc_params()
    for args in ((None, C.byref(cs), C.byref(P), ip, ip, 4, C.byref(n)), (C.byref(ct), None, C.byref(P), ip, ip, 4, C.byref(n)),
                 (C.byref(ct), C.byref(cs), None, ip, ip, 4, C.byref(n)), (C.byref(ct), C.byref(cs), C.byref(P), None, ip, 4, C.byref(n)),
                 (C.byref(ct), C.byref(cs), C.byref(P), ip, None, 4, C.byref(n)), (C.byref(ct), C.byref(cs), C.byref(P), ip, ip, 4, None)):
        assert L.mulls_ncc_correspond(ctx_auto.h, *args) == abi.MULLS_E_INVALID
    assert L.mulls_ncc_correspond(None, C.byref(ct), C.byref(cs), C.byref(P), ip, ip, 4, C.byref(n)) == abi.MULLS_E_INVALID
    null = abi.Cloud()
    null.pts, null.n, null.stride = None, 100, 48
    assert L.mulls_ncc_correspond(ctx_auto.h, C.byref(null), C.byref(cs), C.byref(P), ip, ip, 4, C.byref(n)) == abi.MULLS_E_INVALID


def test_device_resident_key_points(ctx_auto):
    """the demo scan through mulls_extract_features_resident: its MULLS_EX_VERTEX block cloud on either side gives the pairs of the downloaded cloud"""
    Z = np.load(os.path.join(os.path.dirname(FIXTURE), "demo_pair.npz"))
    X = ncc_restated.demo_extract_params()
    blocks, hosts = [], []
    for k in (0, 15):
        a = Z["scan_%d" % k]
        b = ctx_auto.block().extract(abi.make_points(a[:, :3], None, a[:, 3], None), X)
        blocks.append(b)
        hosts.append(b.download(abi.EX_VERTEX))
    assert len(hosts[0]) > 1000 and len(hosts[1]) > 1000
    for fixed, cn, recip in MODES + ((1, 2000, 0),):
        want = check(ctx_auto, hosts[0], hosts[1], fixed, cn, recip, ("resident, host copy", fixed, recip))
        for t, s in ((blocks[0].cloud(abi.EX_VERTEX), blocks[1].cloud(abi.EX_VERTEX)), (blocks[0].cloud(abi.EX_VERTEX), hosts[1]),
                     (hosts[0], blocks[1].cloud(abi.EX_VERTEX))):
            ok, got, n = device_pairs(ctx_auto, t, s, fixed, cn, recip)
            assert ok and n == len(want) and np.array_equal(got, want), (fixed, recip)
    for b in blocks:
        b.close()


def test_scratch_reuse_and_interleaving(ctx_auto, pairs_small):
    big = ncc_restated.random_kpts(51, 3000), ncc_restated.random_kpts(52, 2500)
    small = ncc_restated.random_kpts(53, 120, "quantised"), ncc_restated.random_kpts(54, 90, "quantised")
    P = abi.kitti_params(dis_thre_unit=2.4)
    first = {}
    for rep in range(3):
        for tag, (t, s) in (("big", big), ("small", small)):
            for fixed, cn, recip in MODES + ((1, 300, 0),):
                ok, got, n = device_pairs(ctx_auto, t, s, fixed, cn, recip)
                key = (tag, fixed, recip)
                if rep == 0:
                    first[key] = got
                    assert np.array_equal(got, ncc_restated.restate(t, s, fixed, cn, recip)[1]), key
                assert ok and np.array_equal(got, first[key]), (rep, key)
        if rep == 0:
            r0 = ctx_auto.icp(pairs_small[0][0], P)[0]
            T0 = list(r0.T[:])
        else:
            assert list(ctx_auto.icp(pairs_small[0][0], P)[0].T[:]) == T0  # and the registration is not disturbed either


# ---- the edges ------------------------------------------------------------------------------------------------------------------------------------

ALL_MODES = MODES + ((1, 300, 0),)


def f32(raw):
    """the 12 floats of (n, 48) uint8 records, a view: writes go to the records"""
    return raw.view(np.float32).reshape(len(raw), 12)


def test_edges_fixture_device_equals_reference_lines(ctx_auto):
    seen = 0
    for name, t, s, fixed, cn, recip, ok, pairs in edge_cases():
        got_ok, got, n = device_pairs(ctx_auto, t, s, fixed, cn, recip)
        assert got_ok == ok and n == len(pairs), (name, n, len(pairs))
        assert np.array_equal(got, pairs), name
        seen += 1
    assert seen == 33


def odd_sources(seed, n=300):
    """sources with NaN and infinite curvatures (normal[3]) and heights (data[3]) among ordinary rows"""
    s = ncc_restated.random_kpts(seed, n)
    f32(s)[3::29, 7] = np.nan
    f32(s)[5::31, 7] = np.inf
    f32(s)[7::37, 3] = np.nan
    f32(s)[11::41, 3] = np.inf
    f32(s)[13::43, 3] = -np.inf
    return s


def nan_positions(n):
    sets = [(0,), (1023,), (1024,), (n - 2,), (n - 1,), (0, n - 1), tuple(np.random.default_rng(n).choice(n, 12, replace=False))]
    return [tuple(p for p in at) for at in sets if all(p < n for p in at)]


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049, 5000])
def test_nan_intensity_fold_at_the_stride(ctx_auto, n):
    """k_ncc_minmax: the fold restarts behind the last NaN target intensity, returns NaN when the last point is it, and clamps to FLT_MAX / 0 only without one"""
    s = odd_sources(3000 + n)
    plain = ncc_restated.random_kpts(4000 + n, n)
    sets = nan_positions(n)
    assert len(sets) == (5 if n == 1023 else 6 if n == 1024 else 7)
    ranges = set()
    for at in sets:
        t = plain.copy()
        f32(t)[list(at), 8] = np.nan
        lo, hi = ncc_restated.intensity_range(ncc_restated.fields(t)["inten"])
        rest = ncc_restated.fields(t)["inten"][max(at) + 1:]
        assert (np.isnan(lo) and np.isnan(hi)) if max(at) == n - 1 else (lo == rest.min() and hi == rest.max())
        ranges.add((float(lo), float(hi)))
        for fixed, cn, recip in ALL_MODES:
            check(ctx_auto, t, s, fixed, cn, recip, (n, at, fixed, recip))
    assert len(ranges) >= 4  # the positions really move the range
    # the clamp: negative intensities leave intensity_max at 0; equal ones too; a NaN in front of them removes the clamp (the range collapses: NaN distances)
    for tag, inten in (("negative", -1.0 - ncc_restated.fields(plain)["inten"]), ("equal negative", np.full(n, -5.0, np.float32))):
        t = plain.copy()
        f32(t)[:, 8] = inten
        assert ncc_restated.intensity_range(ncc_restated.fields(t)["inten"])[1] == 0
        for fixed, cn, recip in ALL_MODES:
            check(ctx_auto, t, s, fixed, cn, recip, (n, tag, fixed, recip))
        f32(t)[0, 8] = np.nan
        assert ncc_restated.intensity_range(ncc_restated.fields(t)["inten"])[1] < 0
        for fixed, cn, recip in ALL_MODES:
            check(ctx_auto, t, s, fixed, cn, recip, (n, tag, "behind a NaN", fixed, recip))
    for tag, at, v in (("+inf", (n // 2,), np.inf), ("-inf", (n // 3,), -np.inf), ("both", (5, n - 3), None), ("+inf last", (n - 1,), np.inf), ("every +inf", None, np.inf)):
        t = plain.copy()
        if at is None:
            f32(t)[:, 8] = v
        elif v is None:
            f32(t)[at[0], 8], f32(t)[at[1], 8] = np.inf, -np.inf
        else:
            f32(t)[list(at), 8] = v
        for fixed, cn, recip in ALL_MODES:
            check(ctx_auto, t, s, fixed, cn, recip, (n, "intensity", tag, fixed, recip))


def test_infinite_distances_are_selected_after_the_finite_ones(ctx_auto):
    """corr_num beyond the number of finite distances: +inf entries are selectable (NaN ones never), in flat-index order behind every finite one"""
    t, s = ncc_restated.random_kpts(61, 12), ncc_restated.random_kpts(62, 15)
    f32(s)[::3, 3] = np.inf  # 5 columns of +inf
    f32(s)[1, 7] = np.nan  # and one of NaN
    imin, imax = ncc_restated.intensity_range(ncc_restated.fields(t)["inten"])
    dt = ncc_restated.table(ncc_restated.descriptors(t, imin, imax), ncc_restated.descriptors(s, imin, imax))
    assert np.isposinf(dt).sum() == 60 and np.isnan(dt).sum() == 12 and np.isfinite(dt).sum() == 108
    for cn in (100, 108, 109, 120, 168, 169, 180, 181, 65536):
        want = check(ctx_auto, t, s, 1, cn, 0, ("inf", cn))
        picked_inf = [(i, j) for i, j in want if np.isposinf(dt[i, j])]
        assert not any(np.isnan(dt[i, j]) for i, j in want)
        if cn == 108:
            assert not picked_inf
    # seven uses per point end the finite walk early (9 finite columns: 63 pairs at most), the infinite columns then take the targets that are left
    want = check(ctx_auto, t, s, 1, 168, 0, ("inf", "all"))
    assert any(np.isposinf(dt[i, j]) for i, j in want)
    for fixed, cn, recip in MODES:
        check(ctx_auto, t, s, fixed, cn, recip, ("inf", "nn", recip))
    # a larger table, the rank inside the infinite class: levels 3-5 on the +inf pattern
    t, s = ncc_restated.random_kpts(63, 700), odd_sources(64, 500)
    for cn in (300, 65536):
        check(ctx_auto, t, s, 1, cn, 0, ("inf large", cn))
    t, s = ncc_restated.random_kpts(65, 40), odd_sources(66, 60)
    f32(s)[::2, 3] = np.inf
    _, want = ncc_restated.restate(t, s, 1, 65536, 0)
    check(ctx_auto, t, s, 1, 65536, 0, ("inf small", 65536))


@functools.lru_cache(maxsize=None)
def far_prefix(nt, ns, live):
    """Deep ties at high flat indices.  A `quantised` target whose rows, all but the last `live`, have 4096 added to data[3]: descriptor entry 10 (30 * data[3])
    alone then puts every entry of those prefix rows beyond any tail distance, so the K smallest entries of the whole nt x ns table are the K smallest of the
    tail rows' table, at flat indices (nt - live) * ns and up, and the expected result is the restatement of the tail against the source with the target
    indices shifted.  -> (target, source, tail distance table)"""
    t, s = ncc_restated.random_kpts(7000 + nt, nt, "quantised"), ncc_restated.random_kpts(8000 + ns, ns, "quantised")
    f32(t)[:nt - live, 3] += np.float32(4096.0)
    f32(t)[nt - live:nt - live + 2, 8] = (0, 256)
    inten = ncc_restated.fields(t)["inten"]
    imin, imax = ncc_restated.intensity_range(inten)
    assert (imin, imax) == ncc_restated.intensity_range(inten[nt - live:]) == (0, 256)  # the tail alone gives the same descriptors
    T, S = ncc_restated.descriptors(t, imin, imax), ncc_restated.descriptors(s, imin, imax)
    assert np.array_equal(T[nt - live:], ncc_restated.descriptors(t[nt - live:], imin, imax))
    tail = ncc_restated.table(T[nt - live:], S)
    # d(i, j) is a float sum of eleven non-negative terms, the last of them |T[i, 10] - S[j, 10]|: rounding is monotone, so d(i, j) is at least that term
    smallest_prefix = T[:nt - live, 10].min() - S[:, 10].max()
    assert np.isfinite(tail).all() and smallest_prefix > tail.max(), (smallest_prefix, tail.max())
    return t, s, tail


def far_prefix_expected(nt, ns, live, K):
    """-> (target, source, expected pairs), with the preconditions that make the case say something about the index digits asserted"""
    t, s, tail = far_prefix(nt, ns, live)
    flat = tail.reshape(-1)
    k = min(K, len(flat))
    assert k == K  # the tail alone holds K entries
    dK = np.partition(flat, k - 1)[k - 1]
    below, tie = int((flat < dK).sum()), np.nonzero(flat == dK)[0]
    left = k - below
    assert 0 < left < len(tie), (K, left, len(tie))  # more entries at the rank-K distance than remain to be taken: levels 3-5 run
    rank_index = int(tie[left - 1]) + (nt - live) * ns
    assert rank_index >= 0.9 * nt * ns
    _, pairs = ncc_restated.restate(t[nt - live:], s, 1, K, 0)
    want = pairs + np.array([nt - live, 0])
    if K == 1:
        assert len(want) == 1 and tuple(want[-1]) == divmod(rank_index, ns)  # the boundary entry itself is in the output
    return t, s, want, rank_index


FAR_SHAPES = ((4097, 513, 200), (16384, 12288, 512), (65536, 32767, 512), (65536, 32767, 24))


@pytest.mark.parametrize("nt,ns,live", FAR_SHAPES)
def test_fixed_number_ties_at_high_flat_indices(ctx_auto, nt, ns, live):
    """k_ncc_hist<3..5> / k_ncc_pick: the rank-K key's flat index i * Ns + j in digits of 11 / 10 / 10 bits, up to 65536 x 32767 = 2^31 - 2^16 entries"""
    top = set()
    for K in (1, 300, 4096, 65536):
        t, s, want, rank_index = far_prefix_expected(nt, ns, live, K)
        ok, got, n = device_pairs(ctx_auto, t, s, 1, K, 0)
        assert ok and n == len(want), (K, n, len(want))
        assert np.array_equal(got, want), (K, rank_index)
        top.add(rank_index >> 20)
    if nt == 65536:
        assert nt * ns == 2 ** 31 - 2 ** 16 and max(top) == (2047 if live == 24 else 2032)  # the top index digit: at its largest value with 24 live rows
    if nt == 4097:  # small enough for the whole table: the construction itself against the full restatement
        for K in (1, 300, 4096, 65536):
            t, s, want, _ = far_prefix_expected(nt, ns, live, K)
            assert np.array_equal(ncc_restated.restate(t, s, 1, K, 0)[1], want), K


def test_fixed_number_on_the_large_plain_table(ctx_auto):
    """16 384 x 12 288 plain key points, fixed-number mode: the whole 201 M-entry table restated (row chunks of 1024 rows)"""
    t, s = ncc_restated.random_kpts(31, 16384), ncc_restated.random_kpts(32, 12288)
    keep = ncc_restated.CHUNK_ENTRIES
    try:
        ncc_restated.CHUNK_ENTRIES = 1024 * 12288
        want = check(ctx_auto, t, s, 1, 2000, 0, ("large", "fixed", 2000))
    finally:
        ncc_restated.CHUNK_ENTRIES = keep
    assert 1000 < len(want) <= 2000


@pytest.mark.parametrize("family", ["plain", "quantised"])
def test_shapes_at_the_chunk_boundaries(ctx_auto, family):
    """target sizes around k_ncc_recip's chunks of 1024 rows; tables of 10 x 100 000 and 100 000 x 10 (ncc_chunk's 32-column floor, workgroups that leave
    ncc_sweep at once); sources of 31 and 33 columns"""
    kp = lambda seed, n: ncc_restated.random_kpts(seed, n, family)
    shapes = [(nt, 700) for nt in (1023, 1024, 1025, 2048, 2049)] + [(10, 100000), (100000, 10), (600, 33), (600, 31), (33, 600), (31, 600)]
    for nt, ns in shapes:
        t, s = kp(5000 + nt, nt), kp(6000 + ns, ns)
        for fixed, cn, recip in ALL_MODES + ((1, 65536, 0),):
            want = check(ctx_auto, t, s, fixed, cn, recip, (family, nt, ns, fixed, cn, recip))
            if not fixed and not recip:
                assert len(want) == nt


def strided(raw, stride, seed):
    """the records' first min(stride, 48) bytes every `stride` bytes, random bytes between them -> (buffer, abi.Cloud)"""
    n, w = len(raw), min(stride, 48)
    buf = np.random.default_rng(seed).integers(0, 256, (n, stride), dtype=np.uint8)
    buf[:, :w] = raw[:, :w]
    c = abi.Cloud()
    c.pts, c.n, c.stride = buf.ctypes.data, n, stride
    return buf, c


def test_host_strides(ctx_auto):
    """pack_live walks the cloud's own stride (any multiple of 4 from 36: the last live float, intensity, ends at byte 36)"""
    t, s = ncc_restated.random_kpts(71, 1500), ncc_restated.random_kpts(72, 1100)
    want = {m: ncc_restated.restate(t, s, *m)[1] for m in ALL_MODES}
    for m in ALL_MODES:
        ok, got, n = device_pairs(ctx_auto, t, s, *m)
        assert ok and np.array_equal(got, want[m]), m
    for stride in (36, 40, 52, 64):
        bt, ct = strided(t, stride, stride)
        bs, cs = strided(s, stride, stride + 1)
        for a, b in ((ct, cs), (ct, s), (t, cs)):
            for m in ALL_MODES:
                ok, got, n = device_pairs(ctx_auto, a, b, *m)
                assert ok and n == len(want[m]) and np.array_equal(got, want[m]), (stride, m)
    # refusals: MULLS_E_INVALID, *n_corr = 0, nothing written
    L = lib.load()
    idx = np.zeros(8, np.int32)
    ip = idx.ctypes.data_as(C.c_void_p)
    good = abi.Cloud()
    good.pts, good.n, good.stride = s.ctypes.data, len(s), 48
    (b32, c32), (b50, c50) = strided(t, 32, 1), strided(t, 50, 2)
    for fixed in (0, 1):
        P = abi.ncc_params(fixed, 300, 0)
        for c in (c32, c50):
            for args in ((c, good), (good, c)):
                n = C.c_uint32(9)
                rc = L.mulls_ncc_correspond(ctx_auto.h, C.byref(args[0]), C.byref(args[1]), C.byref(P), ip, ip, 4, C.byref(n))
                assert rc == abi.MULLS_E_INVALID and n.value == 0, (c.stride, fixed)
    assert not idx.any()


# torch brings a HIP runtime of its own: a process takes one of the two, the one loaded first, so the tensors live in a child that imports torch first
TORCH_CHILD = r"""
import ctypes as C, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
torch.cuda.init()
assert torch.zeros(4, device="cuda:0").sum().item() == 0
import ncc_restated
from mulls_amd import abi, lib
MODES = ((0, 2000, 1), (0, 2000, 0), (1, 300, 0))
t, s = ncc_restated.random_kpts(71, 1500), ncc_restated.random_kpts(72, 1100)
ctx = lib.Context(0)
def pairs(a, b, m):
    ok, ti, si, n = ctx.ncc_correspond(a, b, abi.ncc_params(*m))
    assert ok and n == len(ti)
    return np.stack([ti, si], 1).astype(np.int64)
def cloud(x, n, stride=48):
    c = abi.Cloud()
    c.pts, c.n, c.stride = x.data_ptr(), n, stride
    return c
want = {m: ncc_restated.restate(t, s, *m)[1] for m in MODES}
for m in MODES:
    assert np.array_equal(pairs(t, s, m), want[m]), m  # host clouds
dev = {k: torch.from_numpy(raw.copy()).to("cuda:0") for k, raw in (("t", t), ("s", s))}
pin = {k: torch.from_numpy(raw.copy()).pin_memory() for k, raw in (("t", t), ("s", s))}
torch.cuda.synchronize()
assert all(x.is_cuda for x in dev.values()) and all(x.is_pinned() for x in pin.values())
D = {k: cloud(x, len(x)) for k, x in dev.items()}
H = {k: cloud(x, len(x)) for k, x in pin.items()}
for a, b in ((D["t"], D["s"]), (D["t"], s), (t, D["s"]), (H["t"], H["s"]), (H["t"], s), (t, H["s"]), (H["t"], D["s"]), (D["t"], H["s"])):
    for m in MODES:
        assert np.array_equal(pairs(a, b, m), want[m]), m
# a device cloud whose stride is not 48: MULLS_E_INVALID, *n_corr = 0, nothing written
wide = torch.zeros((len(t), 64), dtype=torch.uint8, device="cuda:0")
torch.cuda.synchronize()
L, idx = lib.load(), np.zeros(8, np.int32)
ip = idx.ctypes.data_as(C.c_void_p)
good = abi.Cloud()
good.pts, good.n, good.stride = s.ctypes.data, len(s), 48
bad = cloud(wide, len(t), 64)
for fixed in (0, 1):
    P = abi.ncc_params(fixed, 300, 0)
    for a, b in ((bad, good), (good, bad), (bad, D["s"])):
        n = C.c_uint32(9)
        assert L.mulls_ncc_correspond(ctx.h, C.byref(a), C.byref(b), C.byref(P), ip, ip, 4, C.byref(n)) == abi.MULLS_E_INVALID and n.value == 0
assert not idx.any()
for m in MODES:
    assert np.array_equal(pairs(D["t"], D["s"], m), want[m]), m  # and the context goes on
ctx.close()
print("torch clouds ok")
"""


def test_caller_owned_device_and_pinned_memory():
    """key points in a torch device tensor and in a pinned host tensor, on either side: neither is the library's own block memory, hipPointerGetAttributes
    tells them apart; both give the pairs of the host cloud.  A device cloud with stride 64 is refused."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", TORCH_CHILD % (root, os.path.join(root, "tests"))], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "torch clouds ok" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


def test_scratch_after_the_largest_table(ctx_auto, pairs_small):
    """the grow-only scratch after 65536 x 32767: a small case and a registration repeat what they gave before it"""
    small = ncc_restated.random_kpts(53, 120, "quantised"), ncc_restated.random_kpts(54, 90, "quantised")
    mid = ncc_restated.random_kpts(55, 1025), ncc_restated.random_kpts(56, 700)
    P = abi.kitti_params(dis_thre_unit=2.4)
    before = {}
    for tag, (t, s) in (("small", small), ("mid", mid)):
        for m in ALL_MODES:
            before[tag, m] = check(ctx_auto, t, s, *m, (tag, m))
    T0 = list(ctx_auto.icp(pairs_small[0][0], P)[0].T[:])
    nt, ns, live = FAR_SHAPES[2]
    t, s, want, _ = far_prefix_expected(nt, ns, live, 300)
    big = None
    for rep in range(2):
        ok, got, n = device_pairs(ctx_auto, t, s, 1, 300, 0)
        assert ok and np.array_equal(got, want)
        for fixed, cn, recip in MODES:  # the largest nearest-neighbour table too: repeatable (its restatement would take minutes)
            ok, got, n = device_pairs(ctx_auto, t, s, fixed, cn, recip)
            big = big or {}
            assert ok and np.array_equal(got, big.setdefault((fixed, cn, recip), got))
        for tag, (a, b) in (("small", small), ("mid", mid)):
            for m in ALL_MODES:
                ok, got, n = device_pairs(ctx_auto, a, b, *m)
                assert ok and np.array_equal(got, before[tag, m]), (rep, tag, m)
        assert list(ctx_auto.icp(pairs_small[0][0], P)[0].T[:]) == T0


def test_single_call_equals_a_batch_of_one(ctx_auto):
    """mulls_ncc_correspond against mulls_ncc_correspond_batch on that one problem, on one context: the smallest table, a row block plus one row, and one
    column past the 32-column chunk floor, in the three modes — equal return value, n_corr and both index lists.  A refused single call (a device cloud
    with a stride of 49; fixed-number mode with corr_num 70 000) leaves the caller's index buffers alone and *n_corr at 0, and names itself."""
    from test_gpu_ncc_batch import hip_runtime

    for nt, ns in ((10, 10), (257, 1000), (1025, 33)):
        t, s = ncc_restated.random_kpts(9000 + nt, nt), ncc_restated.random_kpts(9100 + ns, ns)
        for m in ALL_MODES:
            ok, ti, si, n = ctx_auto.ncc_correspond(t, s, abi.ncc_params(*m))
            (b_ok, b_ti, b_si, b_n), = ctx_auto.ncc_correspond_batch([(t, s)], abi.ncc_params(*m))
            assert (ok, n) == (b_ok, b_n) and ok is True and n > 0, (nt, ns, m)
            assert np.array_equal(ti, b_ti) and np.array_equal(si, b_si), (nt, ns, m)
    L, hip = lib.load(), hip_runtime()
    good = abi.Cloud()
    good.pts, good.n, good.stride = s.ctypes.data, len(s), 48
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(49 * len(t))) == 0
    try:
        bad = abi.Cloud()
        bad.pts, bad.n, bad.stride = dev.value, len(t), 49
        for a, b, m, code, why in ((bad, good, ALL_MODES[0], abi.MULLS_E_INVALID, "stride"), (good, bad, ALL_MODES[2], abi.MULLS_E_INVALID, "stride"),
                                   (good, good, (1, 70000, 0), abi.MULLS_E_UNSUPPORTED, "corr_num <= 65536")):
            idx, n = np.full((2, 8), -7, np.int32), C.c_uint32(9)
            rc = L.mulls_ncc_correspond(ctx_auto.h, C.byref(a), C.byref(b), C.byref(abi.ncc_params(*m)), idx[0].ctypes.data_as(C.c_void_p),
                                        idx[1].ctypes.data_as(C.c_void_p), 8, C.byref(n))
            assert rc == code and n.value == 0 and (idx == -7).all(), (m, rc, n.value)
            text = L.mulls_last_error(ctx_auto.h).decode()
            assert text.startswith("mulls_ncc_correspond: ") and why in text, text
    finally:
        assert hip.hipFree(dev) == 0
