"""mulls_ground_filter and mulls_classify_nground at the capacities and segment boundaries their kernels are built around (k_ground.hip,
k_ground_normals.hip, k_classify.hip): the inputs of tests/front_end_edges.py — tests/test_front_end_edges.py shows on any machine which boundary
each one crosses — on the device, every output record byte for byte against the oracle; the refusals one step beyond a capacity; the C ABI's
contract by raw calls; and the class labels against a float64 numpy PCA that does not go through the oracle."""
import ctypes as C

import numpy as np
import pytest

from mulls_amd import abi
from oracle import pyoracle

import front_end_edges as fe

pytestmark = pytest.mark.gpu

GROUND = {name: (cloud, P) for name, cloud, P in fe.ground_cases()}
CLASSIFY = {name: (cloud, P) for name, cloud, P in fe.classify_cases()}


def same_ground(a, b, what):
    for k, cloud in enumerate(("ground", "ground_down", "unground")):
        assert a[k].shape == b[k].shape, (what, cloud, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), (what, cloud)


def same_classes(a, a_in, b, b_in, what):
    for k in range(abi.CL_COUNT):
        assert a[k].shape == b[k].shape, (what, abi.CL_NAMES[k], a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), (what, abi.CL_NAMES[k])
    assert a_in.shape == b_in.shape and np.array_equal(a_in, b_in), (what, "cloud_in")  # cloud_in as the function leaves it


def raw_ground_filter(ctx, pts, P, stride=abi.POINT_BYTES, caps=None, padding_seed=None):
    """mulls_ground_filter straight through the C ABI.  Returns (rc, n_out, the three receive buffers, the input buffer as sent and as it is afterwards);
    every receive buffer has one guard record of 0xCD bytes past its capacity."""
    recs = abi.records(pts)
    n = len(recs)
    wide = np.zeros((max(n, 1), stride), np.uint8)
    if padding_seed is not None:
        wide[:] = np.random.default_rng(padding_seed).integers(0, 256, wide.shape, dtype=np.uint8)
    wide[:n, :abi.POINT_BYTES] = recs
    sent = wide.copy()
    caps = [n, n, n] if caps is None else list(caps)
    outs = [np.full((c + 1, abi.POINT_BYTES), 0xCD, np.uint8) for c in caps]
    n_out = (C.c_uint32 * 3)(7, 7, 7)
    rc = ctx.lib.mulls_ground_filter(ctx.h, wide.ctypes.data_as(C.c_void_p), n, stride, C.byref(P), outs[0].ctypes.data_as(C.c_void_p), caps[0],
                                     outs[1].ctypes.data_as(C.c_void_p), caps[1], outs[2].ctypes.data_as(C.c_void_p), caps[2], n_out)
    return rc, list(n_out), outs, sent, wide


def refused(ctx, pts, P, code):
    rc, _, outs, sent, wide = raw_ground_filter(ctx, pts, P)
    assert rc == code, (rc, code)
    assert len(ctx.lib.mulls_last_error(ctx.h) or b"") > 0
    assert all((o == 0xCD).all() for o in outs) and np.array_equal(sent, wide)  # nothing written on the way to the refusal


# ---------------------------------------------------------------------------------------------------------------------------- A. ground filter
@pytest.mark.parametrize("name", list(GROUND))
def test_ground_filter_equals_oracle(ctx_auto, name):
    """A.1 segment and wave boundaries, A.2 cell ids above 32767 and exactly 65536 cells, A.3 the border wrap, A.5 the second staging round and the
    largest scan, A.6 zero rows and a single cell, A.7 the normal methods at their limits"""
    cloud, P = GROUND[name]
    same_ground(pyoracle.ground_filter(cloud(), P), ctx_auto.ground_filter(cloud(), P), name)


def test_one_cell_more_is_refused(ctx_auto):
    """A.4: 257 x 256 cells; the context serves the next call"""
    for m in (0, 3):
        refused(ctx_auto, fe.one_cell_more_cloud(), fe.fine_params(0.25, m), abi.MULLS_E_UNSUPPORTED)
    assert b"cells" in ctx_auto.lib.mulls_last_error(ctx_auto.h)
    cloud, P = GROUND["fine-200x200-m0"]
    same_ground(pyoracle.ground_filter(cloud(), P), ctx_auto.ground_filter(cloud(), P), "after the refusal")


def test_one_point_more_is_refused(ctx_auto):
    """A.5: 500 001 points"""
    refused(ctx_auto, fe.staging_cloud(fe.GF_MAX_POINTS + 1), abi.ground_params(), abi.MULLS_E_UNSUPPORTED)
    cloud, P = GROUND["segment-n1025-m0"]
    same_ground(pyoracle.ground_filter(cloud(), P), ctx_auto.ground_filter(cloud(), P), "after the refusal")


def test_normal_methods_beyond_their_limits_are_refused(ctx_auto):
    """A.7: method 2 with 66 neighbours; method 1 with 1025 ground points within the radius of one of them"""
    refused(ctx_auto, fe.k64_cloud(), abi.ground_params(grid_resolution=3.0, min_grid_pt_num=33, estimate_ground_normal_method=2), abi.MULLS_E_UNSUPPORTED)
    refused(ctx_auto, fe.patch_cloud(fe.PATCH_N_OVER_CAP), fe.patch_params(1, normal_estimation_radius=fe.PATCH_RADIUS), abi.MULLS_E_UNSUPPORTED)
    assert b"1024" in ctx_auto.lib.mulls_last_error(ctx_auto.h)
    # the same cloud is served with a radius that holds fewer, and by the k-nearest search
    for P in (fe.patch_params(1, normal_estimation_radius=0.4), fe.patch_params(2, min_grid_pt_num=10)):
        same_ground(pyoracle.ground_filter(fe.patch_cloud(fe.PATCH_N_OVER_CAP), P), ctx_auto.ground_filter(fe.patch_cloud(fe.PATCH_N_OVER_CAP), P), "after the refusal")


def test_ground_filter_abi_contract(ctx_auto):
    """A.8: records 64 bytes apart with random bytes between them; each capacity below its cloud's size (the prefix written, the full sizes reported,
    the record past the capacity untouched); capacities of zero with NULL outputs; the input left as it was"""
    cloud = fe.abi_cloud()
    for m in (0, 3, 1):
        P = fe.segment_params(m)
        want = pyoracle.ground_filter(cloud, P)
        sizes = [len(x) for x in want]
        for caps in (fe.ABI_CAPS, sizes, [sizes[0], 0, fe.ABI_CAPS[2]]):
            rc, n_out, outs, sent, wide = raw_ground_filter(ctx_auto, cloud, P, stride=64, caps=caps, padding_seed=5)
            assert rc == abi.MULLS_OK and n_out == sizes, (m, caps, rc, n_out)
            for k in range(3):
                kept = min(caps[k], sizes[k])
                assert np.array_equal(outs[k][:kept], want[k][:kept]), (m, caps, k)
                assert (outs[k][kept:] == 0xCD).all(), (m, caps, k)
            assert np.array_equal(sent, wide)
        n_out = (C.c_uint32 * 3)()
        recs = abi.records(cloud)
        rc = ctx_auto.lib.mulls_ground_filter(ctx_auto.h, recs.ctypes.data_as(C.c_void_p), len(recs), abi.POINT_BYTES, C.byref(P), None, 0, None, 0, None, 0, n_out)
        assert rc == abi.MULLS_OK and list(n_out) == sizes


def test_ground_filter_parameter_refusals(ctx_auto):
    """A.8: gf_check's refusals one by one; the context then serves the next call"""
    cloud = fe.abi_cloud()
    bad = [dict(estimate_ground_normal_method=-1), dict(estimate_ground_normal_method=4), dict(estimate_ground_normal_method=1, normal_estimation_radius=0.0),
           dict(min_grid_pt_num=0), dict(grid_resolution=0.0), dict(grid_resolution=float("nan")), dict(ground_random_down_rate=0),
           dict(ground_random_down_down_rate=0), dict(nonground_random_down_rate=0), dict(distance_weight_downsampling_method=3)]
    for kw in bad:
        refused(ctx_auto, cloud, abi.ground_params(**kw), abi.MULLS_E_INVALID)
    recs, out, n_out = abi.records(cloud), np.full((len(cloud), abi.POINT_BYTES), 0xCD, np.uint8), (C.c_uint32 * 3)()
    rc = ctx_auto.lib.mulls_ground_filter(ctx_auto.h, recs.ctypes.data_as(C.c_void_p), len(recs) - 1, abi.POINT_BYTES - 4, C.byref(fe.segment_params(0)),
                                          out.ctypes.data_as(C.c_void_p), len(out), None, 0, None, 0, n_out)
    assert rc == abi.MULLS_E_INVALID and (out == 0xCD).all()  # records closer together than a record is long
    for m in (0, 3):
        same_ground(pyoracle.ground_filter(cloud, fe.segment_params(m)), ctx_auto.ground_filter(cloud, fe.segment_params(m)), "after the refusals")


# ------------------------------------------------------------------------------------------------------------------------------ B. classifier
@pytest.mark.parametrize("name", list(CLASSIFY))
def test_classify_equals_oracle(ctx_auto, name):
    """B.1 the prune of the candidate buffer with ties at rank K and the suppression's overflowing lists, B.2 the coarsened search grid, B.4 index
    order along x, B.5 sizes around a block of queries: all nine clouds and cloud_in"""
    cloud, P = CLASSIFY[name]
    a, a_in = pyoracle.classify_nground(cloud(), P)
    b, b_in = ctx_auto.classify_nground(cloud(), P, with_cloud_in=True)
    same_classes(a, a_in, b, b_in, name)


@pytest.mark.parametrize("K", [24, 40])
def test_device_labels_equal_a_float64_pca(ctx_auto, K):
    """B.3, the one check that does not go through the oracle: the device's labels against numpy's float64 PCA of the same neighbourhoods
    (neighbours by (distance, index), np.linalg.eigh, the six thresholds).  A point within 1e-4 of a threshold is skipped; at most 1 % may be."""
    cloud = fe.classify_cloud()
    out = ctx_auto.classify_nground(cloud, abi.classify_params(neighbor_k=K, sharpen_with_nms=0, extract_vertex_points_method=0))
    want, checked = fe.float64_labels(cloud, K)
    got = fe.classify_labels(cloud, out)
    print("K", K, "checked", int(checked.sum()), "skipped", int((~checked).sum()), "wrong", int((got[checked] != want[checked]).sum()))
    assert int((~checked).sum()) <= len(cloud) // 100
    assert np.array_equal(got[checked], want[checked]), np.nonzero(checked & (got != want))[0][:10]
