"""The --rows mode of tools/gpu_ndt.py, gpu_gicp.py and gpu_pcl_icp.py: rows in the form tools/gpu_ab_single_calls.py collects ("<what>  status <code>
median of N: X ms (min Y, max Z)"), wall time host clouds in to results out, and nothing written to profiles/."""
import time

import numpy as np


def row(what, fn, calls, code=lambda r: r.code):
    """two warm-up calls, then `calls` timed ones"""
    fn(), fn()
    ts = []
    for _ in range(calls):
        t = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    print("%-44s  status %2d  median of %2d: %9.3f ms  (min %.3f, max %.3f)" % (what, code(out), calls, float(np.median(ts)), min(ts), max(ts)), flush=True)


def rows(name, single, one_iteration, batch):
    """the single call, the call cut to one iteration (uploads, setup, one tick, fitness), a batch of 64"""
    row(name + ": one call", single, 15)
    row(name + ": one call, one iteration", one_iteration, 15)
    row(name + ": batch of 64", batch, 5, code=lambda rs: max(r.code for r in rs))
