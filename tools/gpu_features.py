"""Feature extraction on the device vs the CPU oracle, one 64-beam scan: fast_ground_filter + classify_nground_pts.  usage gpu_features.py
[--batch 1,8,64 [--repeats R] [--out profiles/features_batch.txt]: mulls_extract_features_batch against as many mulls_extract_features_resident calls, 121 k-return
scans of the synthetic drive under the KITTI parameter shape — for each B the median over R alternating repeats (after a warm-up of the same shape) of one batch
call of B scans and of B single calls, the same process, the same context; the launch / wait / round counts of the batch call; one check that the bits agree]
[--single-rows [--calls N]: every single entry point of the feature stage and batches of 1, 8 and 64, on 121 k-return scans and on their 4 097-point subsamples,
KITTI parameter shape, one row each in the format tools/gpu_ab_single_calls.py parses (profiles/features_single_as_batch.txt)]"""
import ctypes as C
import os, sys, time, warnings
sys.path.insert(0, "."); warnings.filterwarnings("ignore")
import numpy as np
from mulls_amd import abi, lib, synth
from oracle import pyoracle


def one_scan_report():
    scene = synth.Scene(3)
    s = synth.raycast(scene, synth.se3(0, 0, scene.sensor_height), 64, 1900, seed=3)
    pts = abi.make_points(s["xyz"], np.zeros_like(s["xyz"]), s["intensity"], s["t"])
    ctx = lib.Context(0)
    GP = abi.ground_params()
    for name, CP, rate in (("run_mulls_reg.sh (r 1.0, k 50)", abi.classify_params(), 3), ("kitti flags (r 0.7, k 25)", abi.classify_params(neighbor_searching_radius=0.7, neighbor_k=25, neigh_k_min=7, curvature_thre=0.08), 3),
                           ("every unground point (rate 1)", abi.classify_params(), 1)):
        GPr = abi.ground_params(nonground_random_down_rate=rate)
        ung = ctx.ground_filter(pts, GPr)[2]
        a = ctx.classify_nground(ung, CP)
        t = time.time()
        for _ in range(10):
            a = ctx.classify_nground(ung, CP)
        dt = (time.time() - t) / 10
        t = time.time()
        g = ctx.ground_filter(pts, GPr)
        a = ctx.classify_nground(g[2], CP)
        dboth = time.time() - t
        t = time.time()
        b, _ = pyoracle.classify_nground(ung, CP)
        do = time.time() - t
        ok = all(np.array_equal(x, y) for x, y in zip(a, b))
        print("%-32s %d unground points -> %s: device %.2f ms (upload + kernels + host sort + download), scan -> features %.2f ms, oracle %.1f ms (one core), identical %s"
              % (name, len(ung), [len(x) for x in a], dt * 1e3, dboth * 1e3, do * 1e3, ok))
    X = abi.extract_params(ground=abi.ground_params(), classify=abi.classify_params())
    a = ctx.extract_features(pts, X)
    t = time.time()
    for _ in range(10):
        a = ctx.extract_features(pts, X)
    dx = (time.time() - t) / 10
    t = time.time()
    for _ in range(10):
        g = ctx.ground_filter(pts, abi.ground_params())
        c = ctx.classify_nground(g[2], abi.classify_params())
    d2 = (time.time() - t) / 10
    print("mulls_extract_features (one call, clouds stay on the device): %.2f ms; the two calls: %.2f ms; %d points -> %s" % (dx * 1e3, d2 * 1e3, len(pts), [len(x) for x in a]))


def kitti_shape():
    """lo_gflag_list_kitti_urban.txt as tools/gpu_odometry.py passes it, with the shipped ground normal method (3: the per-cell plane RANSAC)"""
    return abi.extract_params(ground=abi.ground_params(estimate_ground_normal_method=3, fixed_num_downsampling=1, down_ground_fixed_num=800, rng_seed=1),
                              classify=abi.classify_params(neighbor_searching_radius=0.7, neighbor_k=25, neigh_k_min=7, curvature_thre=0.08, fixed_num_downsampling=1,
                                                           unground_down_fixed_num=20000, pillar_down_fixed_num=400, facade_down_fixed_num=1200, beam_down_fixed_num=200,
                                                           roof_down_fixed_num=200, rng_seed=1),
                              apply_dist_filter=1, min_dist_used=1.5, max_dist_used=120.0)


def drive_scans(count, distinct=8):
    """`count` 64 x 1900 scans along a drive through one scene (`distinct` poses, repeated in turn: a scan's work does not depend on its neighbours)"""
    rng = np.random.default_rng(11)
    scene = synth.Scene(11)
    world0, pose, made = synth.se3(0, 0, scene.sensor_height), np.eye(4), []
    for k in range(min(count, distinct)):
        s = synth.raycast(scene, world0 @ pose, 64, 1900, seed=77 + k)
        made.append(abi.records(abi.make_points(s["xyz"], np.zeros_like(s["xyz"]), s["intensity"], s["t"])))
        pose = pose @ synth.se3(rng.uniform(0.7, 1.3) * 0.9, rng.normal(0, 0.03), rng.normal(0, 0.01), 0, 0, np.deg2rad(rng.normal(0, 1.0)))
    return [made[k % len(made)] for k in range(count)]


def batch_report(sizes, repeats, out_path):
    X = kitti_shape()
    ctx = lib.Context(0)
    scans = drive_scans(max(sizes))
    lines = ["mulls_extract_features_batch vs mulls_extract_features_resident, %d-return scans (64 x 1900, synthetic drive), KITTI parameter shape (ground normal method 3, "
             "dist filter 1.5 .. 120 m, r 0.7 k 25, fixed numbers 800 / 20000 / 400 / 1200 / 200 / 200); medians of %d alternating repeats after a warm-up" % (len(scans[0]), repeats)]
    held = [k for k in range(abi.EX_COUNT) if k not in (abi.EX_RAW, abi.EX_DOWN)]
    for B in sizes:
        blocks = [lib.Block(ctx) for _ in range(B)]
        singles = [lib.Block(ctx) for _ in range(B)]
        clouds = (abi.Cloud * B)()
        for i in range(B):
            clouds[i].pts, clouds[i].n, clouds[i].stride = scans[i].ctypes.data, len(scans[i]), abi.POINT_BYTES
        handles = (C.c_void_p * B)(*[b.h for b in blocks])
        results, stats, nout = (abi.ExtractBatchResult * B)(), abi.ExtractBatchStats(), (C.c_uint32 * abi.EX_COUNT)()

        def batch_call():
            t = time.perf_counter()
            rc = ctx.lib.mulls_extract_features_batch(ctx.h, clouds, B, C.byref(X), handles, 0, results, C.byref(stats))
            assert rc == 0, rc
            return time.perf_counter() - t

        def single_calls():
            t = time.perf_counter()
            for i in range(B):
                rc = ctx.lib.mulls_extract_features_resident(ctx.h, C.c_void_p(clouds[i].pts), clouds[i].n, abi.POINT_BYTES, C.byref(X), singles[i].h, nout)
                assert rc == 0, rc
            return time.perf_counter() - t

        batch_call(), single_calls()  # warm-up of this shape: arenas, pinned scratch, blocks, round hints
        tb, ts = [], []
        for _ in range(repeats):
            tb.append(batch_call())
            ts.append(single_calls())
        same = all(np.array_equal(blocks[i].download(k), singles[i].download(k)) for i in (0, B - 1) for k in held)
        mb, ms = float(np.median(tb)), float(np.median(ts))
        lines.append("B %3d: batch %8.3f ms (%6.3f ms/scan, %7.0f scans/s)   %d single calls %8.3f ms (%6.3f ms/scan)   speed-up %5.2fx   sub-batches %d, kernels %d, waits %d, "
                     "promotion rounds %d, suppression rounds %d   first and last scan identical to their single calls: %s"
                     % (B, mb * 1e3, mb * 1e3 / B, B / mb, B, ms * 1e3, ms * 1e3 / B, ms / mb, stats.n_subbatches, stats.n_kernel_launches, stats.n_syncs, stats.promote_rounds,
                        stats.nms_rounds, same))
        print(lines[-1], flush=True)
        for b in blocks + singles:
            b.close()
    ctx.close()
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")


def single_rows(calls):
    """One row per entry point and scan size: the median wall time of `calls` calls after two warm-up calls, and the call's status."""
    full = drive_scans(64)
    small = [np.ascontiguousarray(s[np.linspace(0, len(s) - 1, 4097).astype(np.int64)]) for s in full]
    X = kitti_shape()
    XV = kitti_shape()
    XV.vf_downsample_resolution = 0.2
    ctx = lib.Context(0)
    L, h = ctx.lib, ctx.h

    def row(name, n, fn, count):
        fn(), fn()
        ts = []
        for _ in range(count):
            t = time.perf_counter()
            rc = fn()
            ts.append((time.perf_counter() - t) * 1e3)
        print("%-44s n %6d  status %d  median of %2d: %.3f ms (min %.3f, max %.3f)" % (name, n, rc, count, float(np.median(ts)), min(ts), max(ts)), flush=True)

    for scans in (full, small):
        raw = scans[0]
        n, p = len(raw), raw.ctypes.data_as(C.c_void_p)
        blk = lib.Block(ctx)
        nout = (C.c_uint32 * abi.EX_COUNT)()
        outs = [np.zeros((n, abi.POINT_BYTES), np.uint8) for _ in range(abi.EX_COUNT)]
        out_p = (C.c_void_p * abi.EX_COUNT)(*[o.ctypes.data for o in outs])
        cap = (C.c_uint32 * abi.EX_COUNT)(*([n] * abi.EX_COUNT))
        n3 = (C.c_uint32 * 3)()
        vp = lambda k: outs[k].ctypes.data_as(C.c_void_p)  # noqa: E731
        ung = ctx.ground_filter(abi.points_of(raw), X.ground)[2]
        up, n_after = ung.ctypes.data_as(C.c_void_p), C.c_uint32(0)
        row("mulls_extract_features_resident", n, lambda: L.mulls_extract_features_resident(h, p, n, abi.POINT_BYTES, C.byref(X), blk.h, nout), calls)
        row("mulls_extract_features", n, lambda: L.mulls_extract_features(h, p, n, abi.POINT_BYTES, C.byref(X), out_p, cap, nout), calls)
        row("mulls_ground_filter", n, lambda: L.mulls_ground_filter(h, p, n, abi.POINT_BYTES, C.byref(X.ground), vp(1), n, vp(2), n, vp(3), n, n3), calls)
        row("mulls_classify_nground", len(ung), lambda: L.mulls_classify_nground(h, up, len(ung), abi.POINT_BYTES, C.byref(X.classify), out_p, cap, nout, None, C.byref(n_after)), calls)
        row("mulls_extract_features_resident voxels 0.2", n, lambda: L.mulls_extract_features_resident(h, p, n, abi.POINT_BYTES, C.byref(XV), blk.h, nout), calls)
        blk.close()
        for B in (1, 8, 64):
            blocks = [lib.Block(ctx) for _ in range(B)]
            clouds = (abi.Cloud * B)()
            for i in range(B):
                clouds[i].pts, clouds[i].n, clouds[i].stride = scans[i].ctypes.data, len(scans[i]), abi.POINT_BYTES
            handles = (C.c_void_p * B)(*[b.h for b in blocks])
            results = (abi.ExtractBatchResult * B)()
            row("mulls_extract_features_batch B %2d" % B, n, lambda: L.mulls_extract_features_batch(h, clouds, B, C.byref(X), handles, 0, results, None), calls if B < 64 else max(3, calls // 4))
            for b in blocks:
                b.close()
    ctx.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    if "--single-rows" in argv:
        single_rows(int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 20)
    elif "--batch" in argv:
        batch_report([int(v) for v in argv[argv.index("--batch") + 1].split(",")], int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 9,
                     argv[argv.index("--out") + 1] if "--out" in argv else os.path.join("profiles", "features_batch.txt"))
    else:
        one_scan_report()
