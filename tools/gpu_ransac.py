"""The RANSAC coarse-registration solver (mulls_coarse_reg_ransac) timed on the device: wall time per call, host clouds in to result out, median of 20 after 3
warm-ups, for N in {517, 2840, 16384} pairs x max_iter_num in {2000, 20000}, refinement on and off.  The pairs carry 2 % planted inliers, so that the
sequential rule runs to max_iter_num and every hypothesis the device scores is one the definition evaluates; a 50 % set shows the other end (the rule stops
after tens of iterations, the device has scored max_iter_num + 1 all the same).  Printed next to the times: scored point transforms per second,
(max_iter_num + 1) x N / wall.

    python tools/gpu_ransac.py                 the table
    python tools/gpu_ransac.py --calls 5       five calls per case and nothing else: the run to put under `rocprofv3 --kernel-trace --stats -- ...`
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


def main():
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 0
    ctx = lib.Context(0)
    L = ctx.lib
    res = abi.RansacResult()
    inl = np.zeros(65536, np.int32)
    for ratio in (0.02, 0.5):
        for n in (517, 2840, 16384):
            t, s = planted(100 + n, n, ratio)
            ct, cs = cloud(t), cloud(s)
            for max_iter in (2000, 20000):
                for refine in (0, 1):
                    P = abi.ransac_params(0.5, 8, max_iter, refine)

                    def call():
                        t0 = time.perf_counter()
                        rc = L.mulls_coarse_reg_ransac(ctx.h, C.byref(ct), C.byref(cs), C.byref(P), C.byref(res), inl.ctypes.data_as(C.c_void_p), 65536)
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
                    print("inliers %4.0f %%  N %6d  max_iter %6d  refine %d  status %2d  iterations %6d  refine rounds %d  n_inliers %6d  median %8.3f ms  (min %.3f, max %.3f)"
                          "  %7.2f G point transforms/s" % (100 * ratio, n, max_iter, refine, res.status, res.iterations, res.refine_iterations, res.n_inliers, ts[10] * 1e3,
                                                            ts[0] * 1e3, ts[-1] * 1e3, (max_iter + 1) * n / ts[10] * 1e-9))
    ctx.close()


if __name__ == "__main__":
    main()
