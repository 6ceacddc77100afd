"""Key-point descriptor matching (mulls_ncc_correspond) timed on the device: host-to-host wall time per call, median of 20 after 3 warm-ups, on the
key points of the reference's demo scans 000000 / 000015 (tests/golden/ncc_demo.npz: 2840 x 2767) and on 16 384 x 12 288 seeded random key points, in
the four modes of DESIGN.md's table.

    python tools/gpu_ncc.py                 the table
    python tools/gpu_ncc.py --calls 5       five calls per case and nothing else: the run to put under `rocprofv3 --kernel-trace --stats -- ...`
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mulls_amd import abi, lib  # noqa: E402

MODES = (("reciprocal nearest neighbour", 0, 2000, 1), ("nearest neighbour", 0, 2000, 0), ("fixed number, corr_num 2000", 1, 2000, 0), ("fixed number, corr_num 300", 1, 300, 0))


def random_kpts(seed, n):
    rng = np.random.default_rng(seed)
    f = np.zeros((n, 12), np.float32)
    code = lambda: (rng.integers(0, 30, n) * 1000000 + rng.integers(0, 40, n) * 10000 + rng.integers(0, 60, n) * 100 + rng.integers(0, 99, n)).astype(np.float32)
    f[:, 3], f[:, 4], f[:, 5], f[:, 7], f[:, 8] = rng.uniform(-2, 12, n), code(), code(), rng.uniform(0, 1, n), rng.uniform(0, 255, n)
    return f.view(np.uint8).reshape(n, 48)


def cloud(raw):
    c = abi.Cloud()
    c.pts, c.n, c.stride = raw.ctypes.data, len(raw), abi.POINT_BYTES
    return c


def main():
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
    Z = np.load(os.path.join(ROOT, "tests", "golden", "ncc_demo.npz"))
    cases = (("demo scans 0 / 15", np.ascontiguousarray(Z["kpts_0"]), np.ascontiguousarray(Z["kpts_15"])), ("random", random_kpts(31, 16384), random_kpts(32, 12288)))
    ctx = lib.Context(0)
    L = ctx.lib
    for what, t, s in cases:
        ct, cs = cloud(t), cloud(s)
        ti, si = np.zeros(65536, np.int32), np.zeros(65536, np.int32)
        n = C.c_uint32(0)
        for name, fixed, cn, recip in MODES:
            P = abi.ncc_params(fixed, cn, recip)

            def call():
                t0 = time.perf_counter()
                rc = L.mulls_ncc_correspond(ctx.h, C.byref(ct), C.byref(cs), C.byref(P), ti.ctypes.data_as(C.c_void_p), si.ctypes.data_as(C.c_void_p), 65536, C.byref(n))
                dt = time.perf_counter() - t0
                assert rc == 1, (rc, L.mulls_last_error(ctx.h))
                return dt

            if calls:
                for _ in range(calls):
                    call()
                continue
            for _ in range(3):
                call()
            ts = sorted(call() for _ in range(20))
            print("%-18s %6d x %6d  %-30s %6d pairs  median %8.3f ms  (min %.3f, max %.3f)" % (what, len(t), len(s), name, n.value, ts[10] * 1e3, ts[0] * 1e3, ts[-1] * 1e3))
    ctx.close()


if __name__ == "__main__":
    main()
