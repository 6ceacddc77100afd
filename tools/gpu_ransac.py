"""The RANSAC coarse-registration solver (mulls_coarse_reg_ransac) timed on the device: wall time per call, host clouds in to result out, median of 20 after 3
warm-ups, for N in {517, 2840, 16384} pairs x max_iter_num in {2000, 20000}, refinement on and off.  The pairs carry 2 % planted inliers, so that the
sequential rule runs to max_iter_num and every hypothesis the device scores is one the definition evaluates; a 50 % set shows the other end (the rule stops
after tens of iterations, the device has scored max_iter_num + 1 all the same).  Printed next to the times: scored point transforms per second,
(max_iter_num + 1) x N / wall.  Behind these rows: 2 840 pairs with 40 % inliers and 12 cm of noise at the bound 0.3 (a refinement of several rounds), the demo
scans' four key-point pair lists through mulls_coarse_reg_ransac_indexed (two of them on device-resident key points as well), and 65 536 pairs from host and
from device-resident clouds.

    python tools/gpu_ransac.py                 the table
    python tools/gpu_ransac.py --calls 5       five calls per case and nothing else: the run to put under `rocprofv3 --kernel-trace --stats -- ...`
    python tools/gpu_ransac.py --batch 1,8,64  mulls_coarse_reg_ransac_batch: per B, one batch call of B problems against B single calls in this process, on
                                               the demo scans' four key-point pair lists (indexed, noise_bound 1.0, cycled to B problems) and on B synthetic
                                               sets of 2 840 pairs (40 % inliers with 12 cm of noise, noise_bound 0.3: refinements of several rounds); the
                                               defaults otherwise (max_iter_num 20000, refinement on); median of 20 after a warm-up call of each
    python tools/gpu_ransac.py --batch 64 --batch-only --calls 3    the batch calls alone: the run for `rocprofv3 --kernel-trace --stats`
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mulls_amd import abi, lib  # noqa: E402


def planted(seed, n, ratio, sigma=0.05):
    """n pairs as (n, 48) records: a fraction `ratio` related by one rigid transform, the rest uniform in the scene's box"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-40.0, -40.0, -3.0]), np.array([40.0, 40.0, 10.0])
    src = rng.uniform(lo, hi, (n, 3))
    a = rng.uniform(0.2, 1.2)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    tgt = src @ R.T + rng.uniform([-8, -8, -0.5], [8, 8, 0.5]) + rng.normal(0, sigma, (n, 3))
    out = rng.random(n) >= ratio
    tgt[out] = rng.uniform(lo, hi, (int(out.sum()), 3))
    rec = []
    for p in (tgt, src):
        f = np.zeros((n, 12), np.float32)
        f[:, :3], f[:, 3] = p, rng.uniform(0, 8, n)
        rec.append(f.view(np.uint8).reshape(n, 48))
    return rec


def cloud(raw):
    c = abi.Cloud()
    c.pts, c.n, c.stride = raw.ctypes.data, len(raw), abi.POINT_BYTES
    return c


def batch_table(sizes, calls, batch_only):
    ctx = lib.Context(0)
    L = ctx.lib
    Z = np.load(os.path.join(ROOT, "tests", "golden", "ncc_demo.npz"))
    kt, ks = np.ascontiguousarray(Z["kpts_0"]), np.ascontiguousarray(Z["kpts_15"])
    lists = [np.ascontiguousarray(Z[name + "_pairs"], np.int32) for name in ("recip_0_15", "nn_0_15", "fixed2000_0_15", "fixed300_0_15")]
    lists = [(np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])) for pr in lists]
    synth = [planted(200 + k, 2840, 0.4, sigma=0.12) for k in range(max(sizes))]
    inl = np.zeros((max(sizes), 4096), np.int32)
    print("mulls_coarse_reg_ransac_batch against B single calls: max_iter_num 20000, refine 1, wall time host clouds in to results out, median of %d" % (calls or 20))
    for what, bound in (("demo pair lists (indexed)", 1.0), ("synthetic 2840 pairs", 0.3)):
        P = abi.ransac_params(bound, 8, 20000, 1)
        for B in sizes:
            arr, res, single = (abi.RansacProblem * B)(), (abi.RansacResult * B)(), (abi.RansacResult * B)()
            for b in range(B):
                if bound == 1.0:
                    ti, si = lists[b % len(lists)]
                    arr[b].tgt, arr[b].src, arr[b].tgt_idx, arr[b].src_idx, arr[b].n_corr = cloud(kt), cloud(ks), ti.ctypes.data, si.ctypes.data, len(ti)
                else:
                    arr[b].tgt, arr[b].src = cloud(synth[b][0]), cloud(synth[b][1])
                arr[b].inlier_cap, arr[b].inliers = inl.shape[1], inl[b].ctypes.data

            def batch_call():
                t0 = time.perf_counter()
                rc = L.mulls_coarse_reg_ransac_batch(ctx.h, arr, B, C.byref(P), 0, res)
                dt = time.perf_counter() - t0
                assert rc == 0, (rc, L.mulls_last_error(ctx.h))
                return dt

            def single_calls():
                t0 = time.perf_counter()
                for b in range(B):
                    A = arr[b]
                    ip = C.c_void_p(A.inliers)
                    if A.tgt_idx:
                        rc = L.mulls_coarse_reg_ransac_indexed(ctx.h, C.byref(A.tgt), C.byref(A.src), C.c_void_p(A.tgt_idx), C.c_void_p(A.src_idx), A.n_corr, C.byref(P),
                                                               C.byref(single[b]), ip, A.inlier_cap)
                    else:
                        rc = L.mulls_coarse_reg_ransac(ctx.h, C.byref(A.tgt), C.byref(A.src), C.byref(P), C.byref(single[b]), ip, A.inlier_cap)
                    assert rc == 0, (rc, L.mulls_last_error(ctx.h))
                return time.perf_counter() - t0

            batch_call()
            tb = sorted(batch_call() for _ in range(calls or 20))
            rounds = max(r.refine_iterations for r in res)
            if batch_only:
                print("%-26s B %3d  batch %9.3f ms  longest refinement %d rounds" % (what, B, tb[len(tb) // 2] * 1e3, rounds))
                continue
            single_calls()
            ts = sorted(single_calls() for _ in range(calls or 20))
            assert all(bytes(res[b]) == bytes(single[b]) for b in range(B))  # the same bytes, or the times compare nothing
            mb, ms = tb[len(tb) // 2], ts[len(ts) // 2]
            print("%-26s B %3d  batch %9.3f ms (min %.3f, max %.3f)  %3d single calls %9.3f ms (min %.3f, max %.3f)  single / batch %5.2f  longest refinement %d rounds"
                  % (what, B, mb * 1e3, tb[0] * 1e3, tb[-1] * 1e3, B, ms * 1e3, ts[0] * 1e3, ts[-1] * 1e3, ms / mb, rounds))
    ctx.close()


class DevBuf:
    """records in device memory (the HIP runtime the library has loaded)"""

    def __init__(self, raw):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.raw, self.p = np.ascontiguousarray(raw), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), self.raw.nbytes) == 0
        assert self.hip.hipMemcpy(self.p, C.c_void_p(self.raw.ctypes.data), self.raw.nbytes, 1) == 0

    def cloud(self):
        c = abi.Cloud()
        c.pts, c.n, c.stride = self.p.value, len(self.raw), abi.POINT_BYTES
        return c


def main():
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
    if "--batch" in sys.argv:
        return batch_table([int(v) for v in sys.argv[sys.argv.index("--batch") + 1].split(",")], calls, "--batch-only" in sys.argv)
    ctx = lib.Context(0)
    L = ctx.lib
    res = abi.RansacResult()
    inl = np.zeros(65536, np.int32)
    ip = inl.ctypes.data_as(C.c_void_p)

    def row(label, ct, cs, P, n, lists=None):
        """one row: 3 warm-up calls, then the median of 20 (with --calls: that many calls and nothing else)"""
        def call():
            t0 = time.perf_counter()
            if lists is None:
                rc = L.mulls_coarse_reg_ransac(ctx.h, C.byref(ct), C.byref(cs), C.byref(P), C.byref(res), ip, 65536)
            else:
                rc = L.mulls_coarse_reg_ransac_indexed(ctx.h, C.byref(ct), C.byref(cs), lists[0].ctypes.data_as(C.c_void_p), lists[1].ctypes.data_as(C.c_void_p), n,
                                                       C.byref(P), C.byref(res), ip, 65536)
            dt = time.perf_counter() - t0
            assert rc == 0, (rc, L.mulls_last_error(ctx.h))
            return dt

        if calls:
            for _ in range(calls):
                call()
            return
        for _ in range(3):
            call()
        ts = sorted(call() for _ in range(20))
        print("%-58s  max_iter %6d  refine %d  status %2d  iterations %6d  refine rounds %d  n_inliers %6d  median %8.3f ms  (min %.3f, max %.3f)"
              "  %7.2f G point transforms/s" % (label, P.max_iter_num, P.refine, res.status, res.iterations, res.refine_iterations, res.n_inliers, ts[10] * 1e3,
                                                ts[0] * 1e3, ts[-1] * 1e3, (P.max_iter_num + 1) * n / ts[10] * 1e-9), flush=True)

    for ratio in (0.02, 0.5):
        for n in (517, 2840, 16384):
            t, s = planted(100 + n, n, ratio)
            for max_iter in (2000, 20000):
                for refine in (0, 1):
                    row("inliers %2.0f %%  N %6d" % (100 * ratio, n), cloud(t), cloud(s), abi.ransac_params(0.5, 8, max_iter, refine), n)
    # refinements of several rounds: the first synthetic set of --batch
    t, s = planted(200, 2840, 0.4, sigma=0.12)
    row("inliers 40 %  N   2840  sigma 0.12  bound 0.3", cloud(t), cloud(s), abi.ransac_params(0.3, 8, 20000, 1), 2840)
    # the demo scans' key-point pair lists through the indexed entry point, on host and on device-resident key points
    Z = np.load(os.path.join(ROOT, "tests", "golden", "ncc_demo.npz"))
    kt, ks = np.ascontiguousarray(Z["kpts_0"]), np.ascontiguousarray(Z["kpts_15"])
    dkt, dks = DevBuf(kt), DevBuf(ks)
    P = abi.ransac_params(1.0, 8, 20000, 1)
    for name in ("recip_0_15", "nn_0_15", "fixed2000_0_15", "fixed300_0_15"):
        pr = np.ascontiguousarray(Z[name + "_pairs"], np.int32)
        lists = (np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1]))
        row("demo %-14s  N %6d  indexed, host key points" % (name, len(pr)), cloud(kt), cloud(ks), P, len(pr), lists)
        if name in ("nn_0_15", "fixed300_0_15"):
            row("demo %-14s  N %6d  indexed, device key points" % (name, len(pr)), dkt.cloud(), dks.cloud(), P, len(pr), lists)
    # the largest problem: three masks come down, and with a device-resident source both point arrays
    t, s = planted(100 + 65536, 65536, 0.5)
    dt, ds = DevBuf(t), DevBuf(s)
    P = abi.ransac_params(0.5, 8, 100, 1)
    row("inliers 50 %  N  65536  host clouds", cloud(t), cloud(s), P, 65536)
    row("inliers 50 %  N  65536  device clouds", dt.cloud(), ds.cloud(), P, 65536)
    ctx.close()


if __name__ == "__main__":
    main()
