"""Key-point descriptor matching (mulls_ncc_correspond) timed on the device: host-to-host wall time per call, median of 20 after 3 warm-ups, on the
key points of the reference's demo scans 000000 / 000015 (tests/golden/ncc_demo.npz: 2840 x 2767) and on 16 384 x 12 288 seeded random key points, in
the four modes of DESIGN.md's table.

    python tools/gpu_ncc.py                 the table
    python tools/gpu_ncc.py --calls 5       five calls per case and nothing else: the run to put under `rocprofv3 --kernel-trace --stats -- ...`
    python tools/gpu_ncc.py --batch 1,8,64  mulls_ncc_correspond_batch: B problems on the demo key points (scans 0 / 15, the direction alternating, every
                                            problem with copies of its own of the two clouds) through the batch entry and as B single calls on the same
                                            clouds and context, in three modes (reciprocal, nearest neighbour, fixed number with corr_num 4000): every
                                            index list compared, both wall times as the median of 20 after 3 warm-ups.  With --calls N: N batch calls per
                                            row and nothing else, the run to trace
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


BATCH_MODES = (("reciprocal nearest neighbour", 0, 2000, 1), ("nearest neighbour", 0, 2000, 0), ("fixed number, corr_num 4000", 1, 4000, 0))


def batch_mode(sizes, calls):
    """B problems through mulls_ncc_correspond_batch and as B calls of mulls_ncc_correspond: equality of every list, and the two wall times"""
    Z = np.load(os.path.join(ROOT, "tests", "golden", "ncc_demo.npz"))
    ctx = lib.Context(0)
    L = ctx.lib
    for B in sizes:
        kp = [(Z["kpts_0"].copy(), Z["kpts_15"].copy()) if b % 2 == 0 else (Z["kpts_15"].copy(), Z["kpts_0"].copy()) for b in range(B)]
        arr, res = (abi.NccProblem * B)(), (abi.NccResult * B)()
        idx = np.zeros((2, B, 2, 4096), np.int32)  # [batch | singles][problem][target | source]
        for b, (t, s) in enumerate(kp):
            arr[b].tgt, arr[b].src = cloud(t), cloud(s)
            arr[b].tgt_idx, arr[b].src_idx, arr[b].cap = idx[0, b, 0].ctypes.data, idx[0, b, 1].ctypes.data, 4096
        counts = np.zeros((2, B), np.uint32)
        for name, fixed, cn, recip in BATCH_MODES:
            P = abi.ncc_params(fixed, cn, recip)

            def batch():
                t0 = time.perf_counter()
                rc = L.mulls_ncc_correspond_batch(ctx.h, arr, B, C.byref(P), 0, res)
                dt = time.perf_counter() - t0
                assert rc == 0, (rc, L.mulls_last_error(ctx.h))
                return dt

            def singles():
                n = C.c_uint32(0)
                t0 = time.perf_counter()
                for b in range(B):
                    rc = L.mulls_ncc_correspond(ctx.h, C.byref(arr[b].tgt), C.byref(arr[b].src), C.byref(P), idx[1, b, 0].ctypes.data_as(C.c_void_p),
                                                idx[1, b, 1].ctypes.data_as(C.c_void_p), 4096, C.byref(n))
                    assert rc == 1, (rc, L.mulls_last_error(ctx.h))
                    counts[1, b] = n.value
                return time.perf_counter() - t0

            if calls:
                for _ in range(calls):
                    batch()
                continue
            idx[:] = -1
            for _ in range(3):
                batch(), singles()
            counts[0] = [res[b].n_corr for b in range(B)]
            same = np.array_equal(idx[0], idx[1]) and np.array_equal(counts[0], counts[1]) and all(res[b].ret == 1 for b in range(B)) and counts.max() <= 4096
            both = [(batch(), singles()) for _ in range(20)]  # alternating: whatever else the host is doing meets both alike
            tb, ts = sorted(a for a, _ in both), sorted(b for _, b in both)
            print("B %3d  2840 x 2767 / 2767 x 2840  %-30s %5d / %5d pairs | batch call, median of 20: %9.3f ms (min %.3f, max %.3f) | %d single calls: %9.3f ms"
                  " (min %.3f, max %.3f) | ratio %.2f | every list %s" % (B, name, counts[0, 0], counts[0, min(1, B - 1)], tb[10] * 1e3, tb[0] * 1e3, tb[-1] * 1e3, B,
                                                                          ts[10] * 1e3, ts[0] * 1e3, ts[-1] * 1e3, ts[10] / tb[10], "agrees" if same else "DIFFERS"), flush=True)
    ctx.close()


def main():
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
    if "--batch" in sys.argv:
        return batch_mode([int(b) for b in sys.argv[sys.argv.index("--batch") + 1].split(",")], calls)
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
