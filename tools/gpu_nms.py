"""The key-point non-maximum suppression (mulls_non_max_suppress) timed on the device: wall time per call, host cloud in to kept cloud out, median of 20
after 3 warm-ups, radius 0.25 m, each path (1 = one workgroup, 2 = multi-launch) on the reference's demo key points (tests/golden/ncc_demo.npz: 2 840 and
2 767 records) and on one synthetic 4 096-point and one 65 536-point cloud (the latter beyond path 1's limit: path 2 only).  Printed next to the times: the
kept count and the rounds the path needed.

    python tools/gpu_nms.py                 the table
    python tools/gpu_nms.py --calls 5       five calls per case and path and nothing else: the run to put under `rocprofv3 --kernel-trace --stats -- ...`
    python tools/gpu_nms.py --cpu           also the wall time of the CPU harness (tests/nms_harness.cpp: upstream's std::sort and sequential walk with a
                                            brute-force radius query, one thread) on the same clouds, once each.  It is the harness, not PCL's kd-tree.
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


def main():
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
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
