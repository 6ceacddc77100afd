"""GPU tests of mulls_ncc_correspond (find_feature_correspondence_ncc, include/common/cregistration.hpp:409-601) through mulls_amd/lib.py: the index
pairs against what the reference's own lines returned on its demo scans (fixture tests/golden/ncc_demo.npz) and against the numpy restatement
(tests/ncc_restated.py, equal to those lines on the fixture: tests/test_ncc.py) on seeded random key points.  Every comparison is equality of integer
arrays."""
import ctypes as C
import os

import numpy as np
import pytest

import ncc_restated
from mulls_amd import abi, lib
from test_ncc import FIXTURE, fixture_cases

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
