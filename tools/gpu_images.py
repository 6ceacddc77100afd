"""The pictures of a cloud (mulls_map_image_2d, mulls_range_image, mulls_scan_images_batch) on one MI355X: wall time per call of the C entry points, arrays
marshalled once, medians after a warm-up call; every timed result is first checked against tests/images_restated.py, byte for byte.
usage: gpu_images.py [--batch 1,8,64] [--reps N] [--out profiles/images.txt]
  1. the export's picture (1 m per pixel, 1920 x 1080, 20 .. 1000 points, shifted) of a device-resident mapper of about 8 M points, in both forms of the
     counting pass, the two alternating call by call
  2. the same picture by the route a caller had before: mulls_mapper_download and the vectorised numpy restatement on the host
  3. the per-frame pictures (range image 900 x 64 and the 400 x 400 bird's-eye view) of B scans in one mulls_scan_images_batch call against B x 2 single
     calls, host scans and device-resident scans"""
import ctypes as C
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
warnings.filterwarnings("ignore")
import numpy as np  # noqa: E402

import images_restated as ir  # noqa: E402
from gpu_mapper import DevBuf  # noqa: E402
from mulls_amd import abi, lib, synth  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternating_ms(fns, reps, warm=2):
    """the functions called in turn, reps rounds after warm rounds: the median of each"""
    t = [[] for _ in fns]
    for k in range(warm + reps):
        for j, fn in enumerate(fns):
            ms = timed(fn)
            if k >= warm:
                t[j].append(ms)
    return [float(np.median(v)) for v in t], [(float(np.min(v)), float(np.max(v))) for v in t]


def main():
    batches = [int(b) for b in arg("--batch", "1,8,64").split(",")]
    reps = int(arg("--reps", "15"))
    out_path = arg("--out", os.path.join(ROOT, "profiles", "images.txt"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    scene = synth.Scene(3)
    s = synth.raycast(scene, synth.se3(0, 0, scene.sensor_height), 64, 1900, seed=3)
    scan = abi.records(abi.make_points(s["xyz"], np.zeros_like(s["xyz"]), s["intensity"], s["t"] * 100.0)).copy()
    n = len(scan)
    ctx = lib.Context(0)
    L, h = ctx.lib, ctx.h
    say("# tools/gpu_images.py on one MI355X, a box shared with other work: wall time per call (the C calls themselves, arrays marshalled once), medians of %d" % reps)
    say("# after 2 warm-up calls [min .. max]; every timed result equals tests/images_restated.py byte for byte.  One 64-beam synthetic scan: %d points." % n)

    # ---- 1. and 2.: the merged map ----
    frames = 64
    m = ctx.mapper(frames * n)
    prep = abi.scan_prep_params()
    dev = DevBuf(scan)
    m.add([(dev.cloud(), synth.se3(0.9 * k, 0.05 * k, 0.0, 0.0, 0.0, 0.01 * k)) for k in range(frames)], prep)
    cloud = m.cloud()
    p = [abi.image2d_params(count_form=f) for f in (1, 2)]
    npix = p[0].map_width * p[0].map_height
    img = [np.zeros(npix, np.uint8) for _ in p]
    cnt = np.zeros(npix, np.int32)
    rep = abi.Image2dReport()

    def map_call(k, counts=None):
        rc = L.mulls_map_image_2d(h, C.byref(cloud), C.byref(p[k]), img[k].ctypes.data_as(C.c_void_p), counts, C.byref(rep))
        assert rc == 0, (rc, L.mulls_last_error(h))

    host = m.download()
    want_img, want_cnt, info = ir.map_image(host, p[0], vectorised=True)
    for k in (0, 1):
        map_call(k, cnt.ctypes.data_as(C.c_void_p))
        assert np.array_equal(img[k], want_img.reshape(-1)) and np.array_equal(cnt, want_cnt.reshape(-1)), "form %d differs from the restatement" % (k + 1)
        assert np.array(rep.centre[:]).tobytes() == info["centre"].tobytes() and rep.n_counted == info["n_counted"]
    say("")
    say("1. mulls_map_image_2d, the export's picture (1 m per pixel, 1920 x 1080, 20 .. 1000, shifted) of a device-resident mapper of %d points" % cloud.n)
    say("   (%d counted, %d outside the frame; the fullest pixel holds %d points, %d pixels hold one at least):" % (rep.n_counted, rep.n_skipped_frame, want_cnt.max(), (want_cnt > 0).sum()))
    med, span = alternating_ms([lambda: map_call(0), lambda: map_call(1)], reps)
    for k, name in enumerate(("form 1, one atomic add per point", "form 2, runs of equal pixels folded in the wave")):
        say("   %-50s %8.3f ms [%.3f .. %.3f]" % (name, med[k], span[k][0], span[k][1]))
    c3 = np.zeros(3)
    med_c, span_c = alternating_ms([lambda: L.mulls_cloud_centre(h, C.byref(cloud), c3.ctypes.data_as(C.POINTER(C.c_double)))], reps)
    say("   %-50s %8.3f ms [%.3f .. %.3f]  (the centre's passes are part of either form's call)" % ("mulls_cloud_centre alone", med_c[0], span_c[0][0], span_c[0][1]))

    buf = np.zeros((cloud.n, abi.POINT_BYTES), np.uint8)
    got_n = C.c_uint32(0)
    t_down, t_numpy = [], []
    for _ in range(3):
        t_down.append(timed(lambda: L.mulls_mapper_download(h, m.h, 0, buf.ctypes.data_as(C.c_void_p), cloud.n, C.byref(got_n))))
        t_numpy.append(timed(lambda: ir.map_image(buf, p[0], vectorised=True)))
    say("2. the same picture the way a caller had it before: mulls_mapper_download %.1f ms (%.0f MB) + the vectorised numpy restatement %.1f ms = %.1f ms" % (
        np.median(t_down), buf.nbytes / 1e6, np.median(t_numpy), np.median(t_down) + np.median(t_numpy)))
    say("   (medians of 3; numpy on one host thread, no OpenCV here to compare with)")
    m.close()

    # ---- 3. the per-frame pictures ----
    rp, bp = abi.range_image_params(), abi.bev_params()
    rpix, bpix = rp.width * rp.height, bp.map_width * bp.map_height
    want_r, want_b = ir.range_image(scan, rp), ir.map_image(scan, bp, vectorised=True)[0]
    say("")
    say("3. mulls_scan_images_batch, the per-frame pictures (range image %d x %d and bird's-eye view %d x %d at %g pixels per metre) of B scans of %d points:" % (
        rp.width, rp.height, bp.map_width, bp.map_height, bp.m2pix, n))
    B_max = max(batches)
    r_out, b_out = [np.zeros(rpix, np.uint8) for _ in range(B_max)], [np.zeros(bpix, np.uint8) for _ in range(B_max)]
    rptr, bptr = (C.c_void_p * B_max)(*[a.ctypes.data for a in r_out]), (C.c_void_p * B_max)(*[a.ctypes.data for a in b_out])
    reps_arr = (abi.Image2dReport * B_max)()
    host_cloud = abi.Cloud()
    host_cloud.pts, host_cloud.n, host_cloud.stride = scan.ctypes.data, n, abi.POINT_BYTES
    for label, one in (("host scans", host_cloud), ("device-resident scans", dev.cloud())):
        scans = (abi.Cloud * B_max)(*[one] * B_max)

        def batch(B):
            rc = L.mulls_scan_images_batch(h, scans, B, C.byref(rp), C.byref(bp), rptr, bptr, reps_arr)
            assert rc == 0, rc

        def singles(B):
            for k in range(B):
                rc = L.mulls_range_image(h, C.byref(scans[k]), C.byref(rp), r_out[k].ctypes.data_as(C.c_void_p))
                rc |= L.mulls_map_image_2d(h, C.byref(scans[k]), C.byref(bp), b_out[k].ctypes.data_as(C.c_void_p), None, None)
                assert rc == 0, rc

        for B in batches:
            for fn in (batch, singles):
                for a in r_out + b_out:
                    a[:] = 1
                fn(B)
                assert all(np.array_equal(r_out[k], want_r.reshape(-1)) and np.array_equal(b_out[k], want_b.reshape(-1)) for k in range(B)), (label, B, fn.__name__)
            med, span = alternating_ms([lambda: batch(B), lambda: singles(B)], reps)
            say("   %-22s B = %2d: one call %8.3f ms [%.3f .. %.3f] = %.3f ms per scan; %3d single calls %8.3f ms [%.3f .. %.3f] = %.3f ms per scan (ratio %.3f)" % (
                label, B, med[0], span[0][0], span[0][1], med[0] / B, 2 * B, med[1], span[1][0], span[1][1], med[1] / B, med[0] / med[1]))
    # the two forms of the counting pass on the per-frame bird's-eye views alone (64 device-resident scans, one call)
    scans = (abi.Cloud * B_max)(*[dev.cloud()] * B_max)
    bps = [abi.bev_params(count_form=f) for f in (1, 2)]

    def bev_batch(k):
        rc = L.mulls_scan_images_batch(h, scans, B_max, None, C.byref(bps[k]), None, bptr, reps_arr)
        assert rc == 0 and np.array_equal(b_out[B_max - 1], want_b.reshape(-1)), rc

    med, span = alternating_ms([lambda: bev_batch(0), lambda: bev_batch(1)], reps)
    say("   bird's-eye views alone, %d device-resident scans in one call: form 1 %.3f ms [%.3f .. %.3f], form 2 %.3f ms [%.3f .. %.3f]" % (
        B_max, med[0], span[0][0], span[0][1], med[1], span[1][0], span[1][1]))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
    print(out_path)


if __name__ == "__main__":
    main()
