"""The statistical outlier removal (mulls_sor_filter) timed on the device: wall time per call, host cloud in to kept cloud out, median of 20 after 3 warm-ups,
mean_k 20 and std_mul 2.0, on three clouds: a synthetic 64-beam scan (about 121 k points), a merged map of 8 poses (about 1 M points) and a merged map of 34
poses (more than 4 M points), built from seeded mulls_amd.synth scans moved along a track.  Printed next to the times: points per second and n_fallback, the
number of queries the grid walk did not certify and brute force answered.

    python tools/gpu_sor.py                 the table
    python tools/gpu_sor.py --calls 5       five calls per case and nothing else: the run to put under `rocprofv3 --kernel-trace --stats -- ...`
    python tools/gpu_sor.py --cpu           also the wall time of the CPU restatement (tests/sor_restated.py: scipy's kd-tree, then numpy) on the same clouds,
                                            once each, with its thread count.  It is the restatement, not PCL.
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
import sor_restated as sr  # noqa: E402

CASES = [("scan 64 x 1900", lambda: sr.synth_scan(3, 64, 1900)), ("map of 8 poses", lambda: sr.merged_map(11, 8)), ("map of 34 poses", lambda: sr.merged_map(11, 34, step=3.0))]


def main():
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
    cpu = "--cpu" in sys.argv
    threads = int(os.environ.get("OMP_NUM_THREADS", 0)) or min(16, os.cpu_count())
    ctx = lib.Context(0)
    L = ctx.lib
    P = abi.sor_params(20, 2.0)
    for name, make in CASES:
        xyz = make()
        n = len(xyz)
        raw = np.zeros((n, 12), np.float32)
        raw[:, :3] = xyz
        raw = raw.view(np.uint8).reshape(n, abi.POINT_BYTES)
        c = abi.Cloud()
        c.pts, c.n, c.stride = raw.ctypes.data, n, abi.POINT_BYTES
        out, n_out, rep = np.zeros((n, abi.POINT_BYTES), np.uint8), C.c_uint32(0), abi.SorReport()

        def call():
            t0 = time.perf_counter()
            rc = L.mulls_sor_filter(ctx.h, C.byref(c), C.byref(P), out.ctypes.data_as(C.c_void_p), n, C.byref(n_out), None, 0, None, C.byref(rep))
            dt = time.perf_counter() - t0
            assert rc == 0, (rc, L.mulls_last_error(ctx.h))
            return dt

        if calls:
            for _ in range(calls):
                call()
            continue
        for _ in range(3):
            call()
        ts = sorted(call() for _ in range(20))
        line = "%-16s n %8d  kept %8d  threshold %.6f  n_fallback %6d  median %9.3f ms  (min %.3f, max %.3f)  %7.2f M points/s" % (
            name, n, rep.n_kept, rep.threshold, rep.n_fallback, ts[10] * 1e3, ts[0] * 1e3, ts[-1] * 1e3, n / ts[10] * 1e-6)
        if cpu:
            try:
                t0 = time.perf_counter()
                d2 = sr.knn_tree(xyz, 21, workers=threads)
                r = sr.restate(xyz, 20, 2.0, d2_sorted=d2)
                dt = time.perf_counter() - t0
                line += "   CPU restatement (%d threads in the kd-tree queries) %9.1f ms, kept %d" % (threads, dt * 1e3, int(r["keep"].sum()))
            except ImportError:
                line += "   CPU restatement: not measured (scipy is not importable)"
        print(line, flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
