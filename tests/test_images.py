"""mulls_cloud_centre / mulls_map_image_2d / mulls_range_image on the CPU: hand-computed cases of the definition as tests/images_restated.py restates it; the
product's arithmetic (mulls_amd/csrc/image_math.h) built into tests/images_harness.cpp with -fsanitize=address,undefined and held against the restatement,
byte for byte; the ABI mirror, the defaults, the PGM writer, the committed fixture.  The device runs in tests/test_gpu_images.py."""
import ctypes as C
import importlib.util
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import images_restated as ir
from mulls_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "images_cases.npz")
CH = abi.SCAN_CHUNK
F32 = np.float32


# ---- hand-computed cases of the restatement ----------------------------------------------------------------------------------------------------------
def small_map(**kw):
    return abi.image2d_params(**dict(ir.EDGE_MAP, **kw))


def counts_of(xyz, **kw):
    return ir.map_image(ir.cloud_of(xyz), small_map(**kw))


def test_truncation_toward_zero_keeps_the_column_zero_quirk():
    """width 16: dx = x + 8.  dx = -0.5 lands in column 0, dx = -1.0 and dx = 16 exactly are outside; rows likewise with dy = -y + 6"""
    _, counts, info = counts_of([(-8.5, 0, 0), (-9.0, 0, 0), (8.0, 0, 0), (7.5, 0, 0), (0, 6.5, 0), (0, 7.0, 0), (0, -6.0, 0), (0, -5.5, 0)])
    want = np.zeros((12, 16), np.int32)
    want[6, 0] = want[6, 15] = want[0, 8] = want[11, 8] = 1
    assert np.array_equal(counts, want)
    assert (info["n_counted"], info["n_skipped_height"], info["n_skipped_frame"]) == (4, 0, 4)


def test_height_limits_and_nan_z():
    """z < min or z > max skips; z equal to a limit stays; a NaN z passes both comparisons and is counted"""
    below, above = np.nextafter(F32(-1), F32(-2)), np.nextafter(F32(2), F32(3))
    _, counts, info = counts_of([(0, 0, math.nan), (0, 0, -1.0), (0, 0, 2.0), (0, 0, below), (0, 0, above)])
    assert counts[6, 8] == 3 and counts.sum() == 3 and info["n_skipped_height"] == 2


def test_non_finite_and_huge_coordinates_are_outside_the_frame():
    _, counts, info = counts_of([(math.inf, 0, 0), (-math.inf, 0, 0), (math.nan, 0, 0), (0, math.nan, 0), (1e30, 0, 0), (0, -3e38, 0)])
    assert counts.sum() == 0 and info["n_skipped_frame"] == 6


def test_8_bit_conversion():
    """min 0 and max 2: a = -127.5; count 0 -> 255, count 1 -> 127.5, a tie, -> 128 (to even), count 2 -> 0, more -> 0.  min 2: counts below it -> 255"""
    image, counts, _ = counts_of([(0.5, 0, 0)] + [(1.5, 0, 0)] * 2 + [(2.5, 0, 0)] * 5)
    assert list(counts[6, 8:11]) == [1, 2, 5] and list(image[6, 7:11]) == [255, 128, 0, 0]
    image, _, _ = counts_of([(0.5, 0, 0)] + [(1.5, 0, 0)] * 2 + [(2.5, 0, 0)] * 3 + [(3.5, 0, 0)] * 4, min_points_in_pix=2, max_points_in_pix=4)
    assert list(image[6, 7:12]) == [255, 255, 255, 128, 0]  # counts 0 and 1 are below min; 2 -> 255; 3 -> 127.5 -> 128; 4 -> 0
    # the other tie parity: a = -1, counts 0 .. 3 give 255 .. 252, and with max - min = 510 a = -0.5: count 1 -> 254.5 -> 254 (to even), count 3 -> 253.5 -> 254
    p = small_map(max_points_in_pix=510)
    assert list(ir.to_8_bits(np.array([0, 1, 2, 3]), p)) == [255, 254, 254, 254]
    p = small_map(min_points_in_pix=5, max_points_in_pix=0)  # max below min: a = +51, the picture inverted
    assert list(ir.to_8_bits(np.array([0, 4, 5, 6]), p)) == [0, 204, 255, 255]


def test_shift_is_the_centre_rounded_to_float():
    xyz = np.array([(10.0, 20.0, 0.0), (11.0, 21.0, 0.0), (13.5, 22.0, 0.0)])
    c = ir.centre(ir.cloud_of(xyz))
    third = [F32(v) / F32(3) for v in (10.0, 11.0, 13.5)]
    assert c[0] == (float(third[0]) + float(third[2])) + float(third[1])  # three lanes: the tree adds lane 2 to lane 0 (w = 2), then lane 1 (w = 1)
    _, counts, info = counts_of(xyz, shift=1)
    sx, sy = F32(c[0]), F32(c[1])
    for x, y, _ in xyz:
        px, py = math.trunc(float(F32(x) - sx) + 8), math.trunc(float(-(F32(y) - sy)) + 6)
        assert counts[py, px] >= 1
    assert info["n_counted"] == 3 and np.array_equal(info["centre"], c)


def test_centre_order_is_the_strided_tree():
    """4097 points: lane 0 adds points 0 and 4096, the tree pairs lane l with l + 2048 first — told apart from a left-to-right sum by values that cancel"""
    n = 4097
    x = np.zeros(n, np.float32)
    x[0], x[2048], x[4096], x[1] = 1e30, -1e30, 3.0, 5.0
    c = ir.centre(ir.cloud_of(np.stack([x, x * 0, x * 0], 1)))
    t = lambda v: float(F32(v) / F32(n))  # noqa: E731
    assert c[0] == ((t(1e30) + t(3.0)) + t(-1e30)) + t(5.0) and c[0] == t(5.0)  # 3 / n is absorbed by 1e30 / n before the tree cancels it
    assert list(ir.centre(ir.cloud_of(np.zeros((0, 3))))) == [0.0, 0.0, 0.0]
    assert np.isnan(ir.centre(ir.cloud_of([(math.inf, 1, 1), (-math.inf, 1, 1)]))[0])


def test_range_image_cases():
    p = abi.range_image_params()
    assert ir.range_image(ir.cloud_of([(0, 0, 0)]), p).sum() == 0  # the origin: z / d = 0 / 0, skipped
    img = ir.range_image(ir.cloud_of([(1.0, 0.0, 100.0)]), p)  # v above the rows: clamped to r = height - 1, written at row 0
    assert img[0, 450] == 255 and np.count_nonzero(img) == 1
    img = ir.range_image(ir.cloud_of([(1.0, 0.0, -100.0)]), p)  # below: r = 0, written at the last row
    assert img[63, 450] == 255 and np.count_nonzero(img) == 1
    # azimuth 0 is the middle column; elevation 0: v = (1 - 3 / 28) * 64 = 57.14 -> r = 57 -> row 6; 35 m of 70: 255 * 0.5 = 127.5 -> 127 (truncated)
    img = ir.range_image(ir.cloud_of([(35.0, 0.0, 0.0)]), p)
    assert img[6, 450] == 127 and np.count_nonzero(img) == 1
    # two points in one pixel: the later one wins even when nearer
    img = ir.range_image(ir.cloud_of([(35.0, 0.0, 0.0), (7.0, 0.0, 0.0)]), p)
    assert img[6, 450] == 25
    img = ir.range_image(ir.cloud_of([(7.0, 0.0, 0.0), (35.0, 0.0, 0.0)]), p)
    assert img[6, 450] == 127
    # azimuth +pi lands in column 0, -pi clamps to the last column
    img = ir.range_image(ir.cloud_of([(-70.0, 0.0, 0.0), (-35.0, -0.0, 0.0)]), p)
    assert img[6, 0] == 255 and img[6, 899] == 127


def test_refusals_of_the_restatement():
    cloud = ir.cloud_of([(1, 2, 3)])
    for kw in (dict(max_points_in_pix=0), dict(map_width=0), dict(map_height=-3), dict(map_width=8193, map_height=8192), dict(m2pix=math.nan),
               dict(min_height=math.nan), dict(max_height=math.nan), dict(count_form=3)):
        with pytest.raises(ir.Refused):
            ir.map_image(cloud, small_map(**kw))
    ir.map_image(cloud, small_map(m2pix=math.inf, min_height=-math.inf, max_height=math.inf))  # infinite values are arithmetic, not refusals
    for kw in (dict(width=0), dict(height=0), dict(width=1 << 14, height=(1 << 12) + 1), dict(f_up_deg=math.nan), dict(f_down_deg=math.inf), dict(max_distance=0.0),
               dict(max_distance=-1.0), dict(max_distance=math.nan)):
        with pytest.raises(ir.Refused):
            ir.range_image(cloud, abi.range_image_params(**kw))


def test_vectorised_counts_equal_the_loop():
    cloud = ir.make_scan(5, 3000)
    for p in (abi.bev_params(), abi.image2d_params(m2pix=0.25, map_width=33, map_height=17, min_points_in_pix=3, max_points_in_pix=40)):
        a, b = ir.map_image(cloud, p), ir.map_image(cloud, p, vectorised=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].sum() > 100


# ---- the product's arithmetic on the CPU --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("images_harness")
    exe = str(d / "images_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "images_harness.cpp"), "-o", exe])
    return exe, str(d)


def run_harness(harness, cloud, bp, rp):
    """-> dict(rc_map, rc_range, centre, tally, counts, image, range): what tests/images_harness.cpp computes with image_math.h"""
    exe, d = harness
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    raw = abi.records(cloud)
    with open(fin, "wb") as f:
        f.write(struct.pack("<II", len(raw), 0) + bytes(bp) + bytes(rp) + raw.tobytes())
    subprocess.check_call([exe, "run", fin, fout])
    blob = open(fout, "rb").read()
    rc_map, rc_range = struct.unpack_from("<ii", blob, 0)
    out = dict(rc_map=rc_map, rc_range=rc_range, centre=np.frombuffer(blob, np.float64, 3, 8), tally=tuple(np.frombuffer(blob, np.uint32, 3, 32)))
    off = 48
    if rc_map == 0:
        npix = bp.map_width * bp.map_height
        out["counts"] = np.frombuffer(blob, np.int32, npix, off).reshape(bp.map_height, bp.map_width)
        out["image"] = np.frombuffer(blob, np.uint8, npix, off + 4 * npix).reshape(bp.map_height, bp.map_width)
        off += 5 * npix
    if rc_range == 0:
        out["range"] = np.frombuffer(blob, np.uint8, rp.width * rp.height, off).reshape(rp.height, rp.width)
        off += rp.width * rp.height
    assert off == len(blob)
    return out


def check_harness(harness, cloud, bp, rp):
    got = run_harness(harness, cloud, bp, rp)
    image, counts, info = ir.map_image(cloud, bp)
    assert got["rc_map"] == got["rc_range"] == 0
    assert got["centre"].tobytes() == info["centre"].tobytes()
    assert got["tally"] == (info["n_counted"], info["n_skipped_height"], info["n_skipped_frame"])
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["image"], image)
    assert np.array_equal(got["range"], ir.range_image(cloud, rp))
    return got


@pytest.mark.parametrize("n", [0, 1, CH - 1, CH, CH + 1, 3000, 4095, 4096, 4097, 8193])
def test_harness_equals_restatement(harness, n):
    cloud = ir.make_scan(100 + n, n, offset=(3.3, -4.4, 0.5))
    check_harness(harness, cloud, abi.bev_params(shift=1, map_width=200, map_height=120), abi.range_image_params())
    check_harness(harness, cloud, abi.image2d_params(m2pix=0.7, map_width=61, map_height=47, min_points_in_pix=1, max_points_in_pix=7),
                  abi.range_image_params(width=1800, height=16, f_up_deg=15.0, f_down_deg=15.0, max_distance=100.0))


def test_harness_on_the_edge_cloud(harness):
    got = check_harness(harness, ir.edge_cloud(), small_map(), abi.range_image_params(width=36, height=8))
    assert got["counts"][6, 0] == 2 and got["counts"][0, 8] == 1 and got["tally"] == (13, 6, 10)
    check_harness(harness, ir.edge_cloud(), small_map(shift=1), abi.range_image_params())  # a NaN centre: every point outside the frame


def test_harness_refusals(harness):
    cloud = ir.cloud_of([(1, 2, 3)])
    for kw in (dict(max_points_in_pix=0), dict(map_width=0), dict(map_width=8193, map_height=8192), dict(m2pix=math.nan), dict(max_height=math.nan), dict(count_form=-1)):
        assert run_harness(harness, cloud, small_map(**kw), abi.range_image_params())["rc_map"] == abi.MULLS_E_INVALID
    for kw in (dict(height=0), dict(f_up_deg=math.nan), dict(max_distance=0.0), dict(max_distance=math.inf)):
        assert run_harness(harness, cloud, small_map(), abi.range_image_params(**kw))["rc_range"] == abi.MULLS_E_INVALID


def test_fixture_is_the_restatement_and_the_harness_meets_it(harness):
    """tests/golden/images_cases.npz (make_images_golden.py): inputs from seeds, images of the restatement as it stood when the fixture was made — the
    restatement still gives them, byte for byte, and the product's arithmetic meets them"""
    spec = importlib.util.spec_from_file_location("make_images_golden", os.path.join(ROOT, "tests", "golden", "make_images_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 400 << 10
    for name, (cloud, bp, rp) in mk.cases().items():
        assert np.array_equal(z[name + "_in"], cloud)
        image, counts, info = ir.map_image(cloud, bp)
        assert np.array_equal(z[name + "_image"], image) and np.array_equal(z[name + "_counts"], counts) and np.array_equal(z[name + "_range"], ir.range_image(cloud, rp))
        assert z[name + "_centre"].tobytes() == info["centre"].tobytes()
        got = run_harness(harness, cloud, bp, rp)
        assert np.array_equal(got["image"], z[name + "_image"]) and np.array_equal(got["counts"], z[name + "_counts"]) and np.array_equal(got["range"], z[name + "_range"])
        assert got["centre"].tobytes() == z[name + "_centre"].tobytes() and list(got["tally"]) == list(z[name + "_tally"])


# ---- the drop-in boundary -------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_layout_matches_header():
    fields = {"mulls_image2d_params": abi.Image2dParams, "mulls_image2d_report": abi.Image2dReport, "mulls_range_image_params": abi.RangeImageParams}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){"]
    for cname, ct in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog.append('printf("pixels %u\\ntree %u\\n", MULLS_IMAGE_MAX_PIXELS, MULLS_NDT_TREE);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    for cname, ct in fields.items():
        assert int(got[cname]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(ct, f).offset, (cname, f)
    assert int(got["pixels"]) == abi.IMAGE_MAX_PIXELS == ir.MAX_PIXELS and int(got["tree"]) == ir.TREE


def test_exports_and_defaults():
    L = lib.load()
    for name in ("mulls_image2d_default_params", "mulls_range_image_default_params", "mulls_cloud_centre", "mulls_map_image_2d", "mulls_range_image",
                 "mulls_scan_images_batch", "mulls_io_write_pgm"):
        assert hasattr(L, name) and name in lib.EXPORTS
    p, r = abi.Image2dParams(), abi.RangeImageParams()
    L.mulls_image2d_default_params(C.byref(p))
    L.mulls_range_image_default_params(C.byref(r))
    assert bytes(p) == bytes(abi.image2d_params()) and bytes(r) == bytes(abi.range_image_params())
    flt_max = float(np.finfo(np.float32).max)
    # test/mulls_slam.cpp:1018 and cfilter.hpp:2717-2721
    assert (p.m2pix, p.map_width, p.map_height, p.min_points_in_pix, p.max_points_in_pix, p.min_height, p.max_height, p.shift, p.count_form) == \
        (1.0, 1920, 1080, 20, 1000, -flt_max, flt_max, 1, 0)
    assert (r.width, r.height, r.f_up_deg, r.f_down_deg, r.max_distance) == (900, 64, 3.0, 25.0, 70.0)
    b = abi.bev_params()  # :731
    assert (b.m2pix, b.map_width, b.map_height, b.min_points_in_pix, b.max_points_in_pix, b.min_height, b.max_height, b.shift) == (4.0, 400, 400, 2, 50, -5.0, 15.0, 0)


def test_pgm_writer_bytes(tmp_path):
    img = (np.arange(7 * 5, dtype=np.uint32) * 37 % 256).astype(np.uint8).reshape(5, 7)
    path = str(tmp_path / "a.pgm")
    lib.write_pgm(path, img)
    assert open(path, "rb").read() == b"P5\n7 5\n255\n" + img.tobytes()
    L = lib.load()
    assert L.mulls_io_write_pgm(path.encode(), None, 7, 5) == abi.MULLS_E_INVALID
    assert L.mulls_io_write_pgm(path.encode(), img.ctypes.data_as(C.c_void_p), 0, 5) == abi.MULLS_E_INVALID
    assert L.mulls_io_write_pgm(str(tmp_path / "no" / "dir.pgm").encode(), img.ctypes.data_as(C.c_void_p), 7, 5) == abi.MULLS_E_IO
    assert open(path, "rb").read() == b"P5\n7 5\n255\n" + img.tobytes()  # the refusals wrote nothing
