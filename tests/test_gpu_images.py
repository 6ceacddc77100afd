"""mulls_cloud_centre, mulls_map_image_2d, mulls_range_image and mulls_scan_images_batch on the device against tests/images_restated.py: every comparison is
equality of bytes.  Sizes at the edges of MULLS_SCAN_CHUNK and of MULLS_NDT_TREE, both forms of the counting pass, contention on one pixel, every edge case of
the definition, host against device-resident input, the batch against the single calls, and every refusal with its outputs left untouched."""
import ctypes as C
import math

import numpy as np
import pytest

import images_restated as ir
from mulls_amd import abi, lib, synth
from test_gpu_scanprep import DevBuf

pytestmark = pytest.mark.gpu
CH = abi.SCAN_CHUNK
GUARD = lib.Context.GUARD
FORMS = (0, 1, 2)


def with_form(p, form):
    q = abi.Image2dParams.from_buffer_copy(p)
    q.count_form = form
    return q


def check_map(ctx, cloud, p, host=None, forms=FORMS):
    """cloud: what the call takes; host: the same records on the host when cloud is device-resident"""
    want_img, want_cnt, info = ir.map_image(cloud if host is None else host, p)
    for form in forms:
        img, cnt, rep = ctx.map_image_2d(cloud, with_form(p, form), want_counts=True)
        assert np.array_equal(cnt, want_cnt), form
        assert np.array_equal(img, want_img), form
        assert np.array(rep.centre[:]).tobytes() == info["centre"].tobytes()
        assert (rep.n_counted, rep.n_skipped_height, rep.n_skipped_frame) == (info["n_counted"], info["n_skipped_height"], info["n_skipped_frame"])
    return want_img, want_cnt


def check_range(ctx, cloud, p, host=None):
    want = ir.range_image(cloud if host is None else host, p)
    assert np.array_equal(ctx.range_image(cloud, p), want)
    return want


@pytest.mark.parametrize("n", [0, 1, CH - 1, CH, CH + 1, 3000])
def test_images_equal_restatement(ctx_auto, n):
    """the per-frame pictures of test/mulls_slam.cpp:722-733 and an export-like map with the shift, at the chunk's edge and over several workgroups"""
    cloud = ir.make_scan(200 + n, n, offset=(3.3, -4.4, 0.5))
    img, cnt = check_map(ctx_auto, cloud, abi.bev_params())
    assert n < CH - 1 or cnt.sum() > 0
    check_map(ctx_auto, cloud, abi.image2d_params(m2pix=0.5, map_width=96, map_height=64, min_points_in_pix=1, max_points_in_pix=9))
    rng_img = check_range(ctx_auto, cloud, abi.range_image_params())  # the upstream size
    assert n < 2 or np.count_nonzero(rng_img) > n // 4
    check_range(ctx_auto, cloud, abi.range_image_params(width=1800, height=16, f_up_deg=15.0, f_down_deg=15.0, max_distance=100.0))


def test_empty_cloud_gives_the_empty_pictures(ctx_auto):
    empty = np.zeros((0, abi.POINT_BYTES), np.uint8)
    img, cnt, rep = ctx_auto.map_image_2d(empty, abi.bev_params(min_points_in_pix=0), want_counts=True)
    assert (img == 255).all() and (cnt == 0).all() and list(rep.centre) == [0.0, 0.0, 0.0]
    img, _ = ctx_auto.map_image_2d(empty, abi.bev_params(min_points_in_pix=-1, max_points_in_pix=1))  # count 0 is (0 + 1) * -127.5 + 255 = 127.5 -> 128
    assert (img == 128).all()
    assert (ctx_auto.range_image(empty) == 0).all() and list(ctx_auto.cloud_centre(empty)) == [0.0, 0.0, 0.0]


def test_contention_and_runs(ctx_auto):
    """5 000 points in ONE pixel (one long run per wave, every add on one word) followed by 5 000 alternating between two pixels (no run longer than one),
    then runs of every length 1 .. 70 across wave and chunk edges"""
    one = np.tile([(0.3, 0.2, 0.0)], (5000, 1))
    alt = np.tile([(2.3, 0.2, 0.0), (3.3, 0.2, 0.0)], (2500, 1))
    runs = np.concatenate([np.tile([(-7.5 + (k % 15), 5.5 - (k % 11), 0.0)], (k, 1)) for k in range(1, 71)])
    cloud = ir.cloud_of(np.concatenate([one, alt, runs]))
    p = abi.image2d_params(**dict(ir.EDGE_MAP, min_points_in_pix=10, max_points_in_pix=5200))
    _, cnt = check_map(ctx_auto, cloud, p)
    assert cnt[5, 8] >= 5000 and cnt[5, 10] >= 2500 and cnt[5, 11] >= 2500 and cnt.sum() == len(cloud)


def test_every_edge_case(ctx_auto):
    """the CPU list (dx = -0.5, -1.0, width; a NaN z; heights equal to a point's z and just beyond) plus +-inf / NaN / huge coordinates, in one cloud"""
    cloud = ir.edge_cloud()
    _, cnt = check_map(ctx_auto, cloud, abi.image2d_params(**ir.EDGE_MAP))
    assert cnt[6, 0] == 2 and cnt[0, 8] == 1 and cnt[6, 8] >= 3
    check_map(ctx_auto, cloud, abi.image2d_params(**dict(ir.EDGE_MAP, shift=1)))  # +inf and -inf: a NaN centre, every point outside the frame
    check_map(ctx_auto, cloud, abi.image2d_params(**dict(ir.EDGE_MAP, m2pix=math.inf, min_height=-math.inf, max_height=math.inf)))
    check_map(ctx_auto, cloud, abi.image2d_params(**dict(ir.EDGE_MAP, min_points_in_pix=5, max_points_in_pix=0)))  # max below min: the picture inverted
    for rp in (abi.range_image_params(), abi.range_image_params(width=36, height=8), abi.range_image_params(f_up_deg=10.0, f_down_deg=-10.0)):  # f_up + f_down = 0
        check_range(ctx_auto, cloud, rp)
    # the 8-bit tie: min 0 and max 2 give a = -127.5, count 1 -> 127.5 -> 128; count >= max -> 0
    img, cnt, _ = ctx_auto.map_image_2d(ir.cloud_of([(0.5, 0, 0)] + [(1.5, 0, 0)] * 2 + [(2.5, 0, 0)] * 5), abi.image2d_params(**ir.EDGE_MAP), want_counts=True)
    assert list(cnt[6, 8:11]) == [1, 2, 5] and list(img[6, 7:11]) == [255, 128, 0, 0]


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_centre_and_shift(ctx_auto, n):
    """the later trips of a lane and the tree of the strided partials; the centre moves points across pixel borders"""
    cloud = ir.make_scan(300 + n, n, r_lo=1.0, r_hi=30.0, offset=(12.3, -7.7, 1.0))
    want = ir.centre(cloud)
    assert ctx_auto.cloud_centre(cloud).tobytes() == want.tobytes() and abs(want[0] - 12.3) < 1.0
    p = abi.image2d_params(m2pix=2.0, map_width=150, map_height=130, min_points_in_pix=0, max_points_in_pix=6)
    shifted, _ = check_map(ctx_auto, cloud, p, forms=(0,))
    plain, _ = check_map(ctx_auto, cloud, with_form(abi.image2d_params(m2pix=2.0, map_width=150, map_height=130, min_points_in_pix=0, max_points_in_pix=6, shift=0), 0), forms=(0,))
    assert not np.array_equal(shifted, plain)


def test_centre_sum_order(ctx_auto):
    """values that cancel tell the strided tree from any other order: lane 0 absorbs 3 / n into 1e30 / n before the tree meets -1e30 / n"""
    x = np.zeros(4097, np.float32)
    x[0], x[2048], x[4096], x[1] = 1e30, -1e30, 3.0, 5.0
    cloud = ir.cloud_of(np.stack([x, x[::-1], x * 0], 1))
    want = ir.centre(cloud)
    assert ctx_auto.cloud_centre(cloud).tobytes() == want.tobytes() and want[0] == float(np.float32(5.0) / np.float32(4097))
    assert np.isnan(ctx_auto.cloud_centre(ir.cloud_of([(math.inf, 1, 1), (-math.inf, 1, 1)]))[0])


def test_range_image_last_index_wins(ctx_auto):
    """2 000 points forced into 3 pixels with shuffled distances: the highest index decides, whatever its distance; index 0 with value 0 and alone"""
    rng = np.random.default_rng(8)
    az = np.deg2rad(np.array([0.0, 90.0, -120.0]))[rng.integers(0, 3, 2000)]
    d = rng.uniform(0.1, 80.0, 2000)
    cloud = ir.cloud_of(np.stack([d * np.cos(az), d * np.sin(az), np.zeros(2000)], 1))
    p = abi.range_image_params(width=90, height=8)
    want = check_range(ctx_auto, cloud, p)
    assert np.count_nonzero(want) <= 3
    i0 = int(np.flatnonzero(az == 0.0)[-1])  # azimuth 0, elevation 0: the middle column, row 0 of 8 (v = (1 - 3 / 28) * 8 = 7.14)
    assert want[0, 45] == int(255.0 * min(1.0, float(np.float32(d[i0]) / np.float32(70.0))))
    near = ir.cloud_of([(0.1, 0.0, 0.0)])  # index 0, value 0: the pixel reads as an empty one
    assert check_range(ctx_auto, near, p).sum() == 0
    assert np.count_nonzero(check_range(ctx_auto, ir.cloud_of([(35.0, 0.0, 0.0)]), p)) == 1  # index 0 with a value
    assert np.count_nonzero(check_range(ctx_auto, ir.cloud_of([(35.0, 0.0, 0.0), (0.1, 0.0, 0.0)]), p)) == 0  # a later value 0 overwrites


def test_device_resident_input(ctx_auto):
    """a device allocation of the caller's gives the bytes of the host path and is left as it was"""
    cloud = ir.make_scan(41, 3 * CH + 7, offset=(-2.0, 6.0, 0.0))
    buf = DevBuf(cloud)
    try:
        check_map(ctx_auto, buf.cloud(), abi.bev_params(shift=1), host=cloud)
        check_range(ctx_auto, buf.cloud(), abi.range_image_params(), host=cloud)
        assert ctx_auto.cloud_centre(buf.cloud()).tobytes() == ir.centre(cloud).tobytes()
        assert np.array_equal(buf.download(), cloud)
    finally:
        buf.free()


def test_mapper_cloud_is_imaged_where_it_lies(ctx_auto):
    """a mulls_mapper filled with two small frames, through mulls_mapper_cloud: the picture of the export (test/mulls_slam.cpp:1016-1025)"""
    prep = abi.scan_prep_params(dist_filter_on=1, min_dist=2.0, max_dist=60.0, downsample_ratio=2)
    m = ctx_auto.mapper(4000)
    try:
        m.add([(ir.make_scan(51, 1500), np.eye(4)), (ir.make_scan(52, 1700), synth.se3(4.0, -3.0, 0.1, 0.0, 0.0, 0.3))], prep)
        host = m.download()
        assert 500 < len(host) < 3200
        p = abi.image2d_params(m2pix=1.5, map_width=192, map_height=108, min_points_in_pix=1, max_points_in_pix=5)
        check_map(ctx_auto, m.cloud(), p, host=host)
        assert np.array_equal(m.download(), host)
    finally:
        m.close()


@pytest.mark.parametrize("count", [1, 3, 9])
def test_batch_equals_single_calls(ctx_auto, count):
    """scans of unequal sizes, one of them empty, host and device-resident ones mixed: every scan gets the bytes of its single calls"""
    sizes = [2 * CH + 5, 0, 1, CH, 3000, CH - 1, 700, CH + 1, 1234][:count]
    if count == 1:
        sizes = [3000]
    clouds = [ir.make_scan(600 + k, n, offset=(1.5 * k, -0.7 * k, 0.2)) for k, n in enumerate(sizes)]
    bufs = {k: DevBuf(clouds[k]) for k in range(count) if k % 4 == 2}
    scans = [bufs[k].cloud() if k in bufs else clouds[k] for k in range(count)]
    rp, bp = abi.range_image_params(), abi.bev_params(shift=1)
    try:
        ranges, bevs, reps = ctx_auto.scan_images_batch(scans, rp, bp)
        for k in range(count):
            img, rep = ctx_auto.map_image_2d(scans[k], bp)
            assert np.array_equal(bevs[k], img) and np.array_equal(ranges[k], ctx_auto.range_image(scans[k], rp)), k
            assert bytes(reps[k])[:36] == bytes(rep)[:36]  # everything but ms_total
        assert np.array_equal(bevs[count - 1], ir.map_image(clouds[count - 1], bp)[0]) and np.array_equal(ranges[0], ir.range_image(clouds[0], rp))
        only_r = ctx_auto.scan_images_batch(scans, rp, None)
        only_b = ctx_auto.scan_images_batch(scans, None, bp)
        assert only_r[1] is None and only_b[0] is None and all(np.array_equal(a, b) for a, b in zip(only_r[0] + only_b[1], ranges + bevs))
    finally:
        for b in bufs.values():
            b.free()
    assert ctx_auto.scan_images_batch([], rp, bp) == ([], [], [])  # n_scans = 0: MULLS_OK


def test_refusals_leave_the_outputs_untouched(ctx_auto):
    L, h = ctx_auto.lib, ctx_auto.h
    raw = ir.make_scan(71, 300)
    good = abi.Cloud()
    good.pts, good.n, good.stride = raw.ctypes.data, len(raw), abi.POINT_BYTES
    img = np.full(64 * 64 + 1, GUARD, np.uint8)
    cnt = np.full(64 * 64 + 1, -7, np.int32)
    rep = abi.Image2dReport()
    rep.n_counted = 12345
    ok = dict(map_width=64, map_height=64)

    def untouched():
        return (img == GUARD).all() and (cnt == -7).all() and rep.n_counted == 12345

    def call_map(cloud, p, image=img):
        return L.mulls_map_image_2d(h, C.byref(cloud), C.byref(p), image.ctypes.data_as(C.c_void_p) if image is not None else None, cnt.ctypes.data_as(C.c_void_p), C.byref(rep))

    for kw in (dict(max_points_in_pix=20), dict(map_width=0), dict(map_height=0), dict(map_width=-5), dict(map_width=8193, map_height=8192), dict(m2pix=math.nan),
               dict(min_height=math.nan), dict(max_height=math.nan), dict(count_form=3)):
        assert call_map(good, abi.image2d_params(**dict(ok, **kw))) == abi.MULLS_E_INVALID and untouched(), kw
    bad = abi.Cloud.from_buffer_copy(good)
    bad.stride = 64
    assert call_map(bad, abi.image2d_params(**ok)) == abi.MULLS_E_INVALID and untouched()
    assert call_map(good, abi.image2d_params(**ok), image=None) == abi.MULLS_E_INVALID and untouched()
    big = abi.Cloud.from_buffer_copy(good)
    big.n = abi.SCAN_MAX_POINTS + 1  # refused before a record is read
    assert call_map(big, abi.image2d_params(**ok)) == abi.MULLS_E_UNSUPPORTED and untouched()
    c = np.full(4, 7.5)
    assert L.mulls_cloud_centre(h, C.byref(big), c.ctypes.data_as(C.POINTER(C.c_double))) == abi.MULLS_E_UNSUPPORTED
    assert L.mulls_cloud_centre(h, C.byref(bad), c.ctypes.data_as(C.POINTER(C.c_double))) == abi.MULLS_E_INVALID and (c == 7.5).all()

    def call_range(cloud, p, image=img):
        return L.mulls_range_image(h, C.byref(cloud), C.byref(p), image.ctypes.data_as(C.c_void_p) if image is not None else None)

    okr = dict(width=64, height=64)
    for kw in (dict(width=0), dict(height=-1), dict(width=1 << 14, height=(1 << 12) + 1), dict(f_up_deg=math.nan), dict(f_down_deg=math.inf), dict(max_distance=0.0),
               dict(max_distance=-70.0), dict(max_distance=math.nan)):
        assert call_range(good, abi.range_image_params(**dict(okr, **kw))) == abi.MULLS_E_INVALID and untouched(), kw
    assert call_range(bad, abi.range_image_params(**okr)) == abi.MULLS_E_INVALID and untouched()
    assert call_range(good, abi.range_image_params(**okr), image=None) == abi.MULLS_E_INVALID and untouched()
    assert call_range(big, abi.range_image_params(**okr)) == abi.MULLS_E_UNSUPPORTED and untouched()
    # a batch: one scan's refusal, or one missing image, and no output of the call is written
    scans = (abi.Cloud * 3)(good, good, good)
    imgs = [np.full(64 * 64 + 1, GUARD, np.uint8) for _ in range(6)]
    rptr, bptr = (C.c_void_p * 3)(*[a.ctypes.data for a in imgs[:3]]), (C.c_void_p * 3)(*[a.ctypes.data for a in imgs[3:]])
    reps = (abi.Image2dReport * 3)()
    reps[0].n_counted = 777
    rp, bp = abi.range_image_params(**okr), abi.image2d_params(**ok)

    def batch():
        return L.mulls_scan_images_batch(h, scans, 3, C.byref(rp), C.byref(bp), rptr, bptr, reps)

    scans[2] = big
    assert batch() == abi.MULLS_E_UNSUPPORTED and all((a == GUARD).all() for a in imgs) and reps[0].n_counted == 777
    scans[2] = bad
    assert batch() == abi.MULLS_E_INVALID and all((a == GUARD).all() for a in imgs)
    scans[2] = good
    bptr[1] = None
    assert batch() == abi.MULLS_E_INVALID and all((a == GUARD).all() for a in imgs)
    bptr[1] = imgs[4].ctypes.data
    bp.max_points_in_pix = bp.min_points_in_pix
    assert batch() == abi.MULLS_E_INVALID and all((a == GUARD).all() for a in imgs) and reps[0].n_counted == 777
    bp = abi.image2d_params(**ok)
    assert batch() == abi.MULLS_OK and all(a[64 * 64] == GUARD and (a[:64 * 64] != GUARD).any() for a in imgs) and reps[0].n_counted != 777
    assert L.mulls_scan_images_batch(h, None, 0, C.byref(rp), C.byref(bp), None, None, None) == abi.MULLS_OK
