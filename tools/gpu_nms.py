"""The key-point non-maximum suppression (mulls_non_max_suppress) timed on the device: wall time per call, host cloud in to kept cloud out, median of 20
after 3 warm-ups, radius 0.25 m, each path (1 = one workgroup, 2 = multi-launch) on the reference's demo key points (tests/golden/ncc_demo.npz: 2 840 and
2 767 records) and on one synthetic 4 096-point and one 65 536-point cloud (the latter beyond path 1's limit: path 2 only).  Printed next to the times: the
kept count and the rounds the path needed.

    python tools/gpu_nms.py                 the table
    python tools/gpu_nms.py --calls 5       five calls per case and path and nothing else: the run to put under `rocprofv3 --kernel-trace --stats -- ...`
    python tools/gpu_nms.py --cpu           also the wall time of the CPU harness (tests/nms_harness.cpp: upstream's std::sort and sequential walk with a
                                            brute-force radius query, one thread) on the same clouds, once each.  It is the harness, not PCL's kd-tree.
    python tools/gpu_nms.py --batch 1,8,64  mulls_non_max_suppress_batch: B clouds through the batch entry and as B single calls (path 0) on the same clouds
                                            and context — the demo key points (scans 0 / 15 alternating, every problem with a copy of its own), synthetic
                                            4 096-point clouds, and the demo clouds device-resident: every output compared, both wall times as the median
                                            of 20 after 3 warm-ups, the calls alternating.  With --calls N: N batch calls per row and nothing else, the
                                            run to trace
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mulls_amd import abi, lib  # noqa: E402
import nms_restated as nr  # noqa: E402


def synthetic(n):
    """uniform points at about the demo key points' survival rate at 0.25 m, keys with ties"""
    rng = np.random.default_rng(n)
    half = 0.13 * n ** (1 / 3)
    return nr.make_records(rng.uniform(-half, half, (n, 3)), np.floor(rng.uniform(0, 1, n) * (n // 8)).astype(np.float32), n)


def cases():
    Z = np.load(os.path.join(ROOT, "tests", "golden", "ncc_demo.npz"), allow_pickle=False)
    return [("demo kpts_0", np.ascontiguousarray(Z["kpts_0"])), ("demo kpts_15", np.ascontiguousarray(Z["kpts_15"])),
            ("synthetic 4096", synthetic(4096)), ("synthetic 65536", synthetic(65536))]


class DevBuf:
    """records in device memory (the HIP runtime the library has loaded)"""

    def __init__(self, raw):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.raw, self.p = np.ascontiguousarray(raw), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), self.raw.nbytes) == 0
        assert self.hip.hipMemcpy(self.p, C.c_void_p(self.raw.ctypes.data), self.raw.nbytes, 1) == 0


def synthetic_seeded(n, seed):
    rng = np.random.default_rng(seed)
    half = 0.13 * n ** (1 / 3)
    return nr.make_records(rng.uniform(-half, half, (n, 3)), np.floor(rng.uniform(0, 1, n) * (n // 8)).astype(np.float32), seed)


def time_batch(ctx, what, raws, resident, calls):
    """one row: the batch call against as many single calls on the same clouds"""
    L, B = ctx.lib, len(raws)
    bufs = [DevBuf(r) for r in raws] if resident else None
    arr, reps = (abi.NmsProblem * B)(), (abi.NmsReport * B)()
    outs = [[np.zeros((len(r), abi.POINT_BYTES), np.uint8) for r in raws] for _ in range(2)]  # [batch | singles]
    idxs = [[np.full(len(r), -1, np.int32) for r in raws] for _ in range(2)]
    orders = [[np.full(len(r), -1, np.int32) for r in raws] for _ in range(2)]
    for b, r in enumerate(raws):
        arr[b].cloud.pts, arr[b].cloud.n, arr[b].cloud.stride = (bufs[b].p.value if resident else r.ctypes.data), len(r), abi.POINT_BYTES
        arr[b].out, arr[b].kept_idx, arr[b].order, arr[b].cap, arr[b].idx_cap = outs[0][b].ctypes.data, idxs[0][b].ctypes.data, orders[0][b].ctypes.data, len(r), len(r)
    P = abi.nms_params(0.25, 0)
    kept = np.zeros((2, B), np.uint32)

    def batch():
        t0 = time.perf_counter()
        rc = L.mulls_non_max_suppress_batch(ctx.h, arr, B, C.byref(P), 0, reps)
        dt = time.perf_counter() - t0
        assert rc == 0, (rc, L.mulls_last_error(ctx.h))
        return dt

    def singles():
        n_out, rep = C.c_uint32(0), abi.NmsReport()
        t0 = time.perf_counter()
        for b in range(B):
            rc = L.mulls_non_max_suppress(ctx.h, C.byref(arr[b].cloud), C.byref(P), outs[1][b].ctypes.data_as(C.c_void_p), arr[b].cloud.n, C.byref(n_out),
                                          idxs[1][b].ctypes.data_as(C.c_void_p), arr[b].cloud.n, orders[1][b].ctypes.data_as(C.c_void_p), C.byref(rep))
            assert rc == 0, (rc, L.mulls_last_error(ctx.h))
            kept[1, b] = n_out.value
        return time.perf_counter() - t0

    if calls:
        for _ in range(calls):
            batch()
        return None
    for _ in range(3):
        batch(), singles()
    kept[0] = [reps[b].n_kept for b in range(B)]
    same = np.array_equal(kept[0], kept[1]) and all(
        outs[0][b].tobytes() == outs[1][b].tobytes() and np.array_equal(idxs[0][b], idxs[1][b]) and np.array_equal(orders[0][b], orders[1][b]) for b in range(B))
    both = [(batch(), singles()) for _ in range(20)]  # alternating: whatever else the host is doing meets both alike
    tb, ts = sorted(a for a, _ in both), sorted(b for _, b in both)
    print("B %3d  %-34s kept %5d / %5d  rounds %3d | batch call, median of 20: %8.3f ms (min %.3f, max %.3f) | %d single calls: %8.3f ms (min %.3f, max %.3f) |"
          " singles / batch %.2f | every output %s" % (B, what, kept[0, 0], kept[0, min(1, B - 1)], max(reps[b].rounds for b in range(B)), tb[10] * 1e3, tb[0] * 1e3,
                                                       tb[-1] * 1e3, B, ts[10] * 1e3, ts[0] * 1e3, ts[-1] * 1e3, ts[10] / tb[10], "agrees" if same else "DIFFERS"), flush=True)


def batch_mode(sizes, calls):
    Z = np.load(os.path.join(ROOT, "tests", "golden", "ncc_demo.npz"), allow_pickle=False)
    ctx = lib.Context(0)
    for B in sizes:
        demo = [np.ascontiguousarray(Z["kpts_0" if b % 2 == 0 else "kpts_15"]).copy() for b in range(B)]
        time_batch(ctx, "demo key points 2840 / 2767", demo, False, calls)
        time_batch(ctx, "synthetic 4096", [synthetic_seeded(4096, 100 + b) for b in range(B)], False, calls)
        time_batch(ctx, "demo key points, device-resident", demo, True, calls)
    ctx.close()


def main():
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
    if "--batch" in sys.argv:
        return batch_mode([int(b) for b in sys.argv[sys.argv.index("--batch") + 1].split(",")], calls)
    cpu = "--cpu" in sys.argv
    ctx = lib.Context(0)
    L = ctx.lib
    H = None
    if cpu:
        import test_nms

        H = test_nms.build_harness()
    for name, raw in cases():
        n = len(raw)
        c = abi.Cloud()
        c.pts, c.n, c.stride = raw.ctypes.data, n, abi.POINT_BYTES
        out, idx, n_out, rep = np.zeros((n, abi.POINT_BYTES), np.uint8), np.zeros(n, np.int32), C.c_uint32(0), abi.NmsReport()
        for path in (1, 2):
            if path == 1 and n > abi.NMS_LDS_MAX_POINTS:
                continue
            P = abi.nms_params(0.25, path)

            def call():
                t0 = time.perf_counter()
                rc = L.mulls_non_max_suppress(ctx.h, C.byref(c), C.byref(P), out.ctypes.data_as(C.c_void_p), n, C.byref(n_out), idx.ctypes.data_as(C.c_void_p), n,
                                              None, C.byref(rep))
                dt = time.perf_counter() - t0
                assert rc == 0 and rep.path == path, (rc, L.mulls_last_error(ctx.h))
                return dt

            if calls:
                for _ in range(calls):
                    call()
                continue
            for _ in range(3):
                call()
            ts = sorted(call() for _ in range(20))
            print("%-16s n %6d  path %d  kept %6d  rounds %4d  median %8.3f ms  (min %.3f, max %.3f)" % (
                name, n, path, rep.n_kept, rep.rounds, ts[10] * 1e3, ts[0] * 1e3, ts[-1] * 1e3), flush=True)
        if cpu and not calls:
            t0 = time.perf_counter()
            k = len(H.suppress(raw, 0.25)[1])
            print("%-16s n %6d  CPU harness (one thread, brute-force radius query) %8.3f ms, kept %d" % (name, n, (time.perf_counter() - t0) * 1e3, k), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
