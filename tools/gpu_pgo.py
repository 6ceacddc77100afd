"""Timing of the pose graph optimisation on the GPU (mulls_pgo_optimize / mulls_pgo_optimize_batch) -> profiles/pgo.txt.

    python tools/gpu_pgo.py [--out FILE] [--repeat 20] [--warmup 3]

1. the inter-submap shape: one 300-node submap graph (chain, node 0 fixed) with three loop edges;
2. the inner-submap shape: B = 1 / 8 / 64 / 256 chain problems of 151 nodes, both ends fixed, limits 0.1 / 0.01, in one batch call against B single
   calls on the same context;
3. the numpy restatement (tests/pgo_restated.py) on one CPU thread, once per shape: not the same program (interpreted loops), there for scale.
Every time is a host clock around a call that ends synchronised (the calls return their results, so they end in a device synchronise); warm-ups first,
then the median of the repetitions with min and max (the B single calls at B >= 64 are repeated a quarter as often).  Every result is compared with the restatement's bits before anything is timed.  No time is a pass criterion."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
os.environ.setdefault("OMP_NUM_THREADS", "1")

import make_pgo_golden as G  # noqa: E402
import pgo_restated as R  # noqa: E402
from mulls_amd import abi, lib  # noqa: E402


def submap_graph(seed, n=300):
    poses, fixed, stable, edges, gt = G.chain(seed, n, t_sigma=0.05, deg=0.3, both_ends=False)
    rng = np.random.default_rng(seed + 1)
    for a, b in ((5, 120), (60, 250), (10, 299)):
        edges.append((a, b, R.SMOOTH, G.noisy(rng, G.inv(gt[a]) @ gt[b], 0.02, 0.1), G.info(rng)))
    return poses, fixed, stable, edges


def timed(fn, warmup, repeat):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return np.median(t), min(t), max(t)


def same(got, r):
    res, poses, wrong = got
    return (poses.view(np.uint64) == r["poses"].view(np.uint64)).all() and res.iterations == r["iterations"] and res.final_cost == r["final_cost"] and (wrong == r["edge_wrong"]).all()


class Marshalled:
    """the C structs of a list of problems, built once: the timed calls are the library's entry points alone"""

    def __init__(self, probs):
        B = len(probs)
        self.keep, self.arr, self.res = [], (abi.PgoProblem * B)(), (abi.PgoResult * B)()
        for b, (poses, fixed, stable, edges) in enumerate(probs):
            nodes, earr = abi.pgo_nodes(poses, fixed, stable), abi.pgo_edges(edges)
            out, wrong = np.zeros((len(poses), 16)), np.zeros(len(edges), np.uint8)
            self.keep.append((nodes, earr, out, wrong))
            P = self.arr[b]
            P.nodes, P.n_nodes, P.edges, P.n_edges = C.addressof(nodes), len(poses), C.addressof(earr), len(edges)
            P.poses_out, P.edge_wrong = out.ctypes.data, wrong.ctypes.data

    def batch(self, ctx, p):
        rc = ctx.lib.mulls_pgo_optimize_batch(ctx.h, self.arr, len(self.keep), C.byref(p), 0, self.res)
        assert rc == 0, ctx.lib.mulls_last_error(ctx.h)

    def singles(self, ctx, p):
        for b, P in enumerate(self.arr):
            rc = ctx.lib.mulls_pgo_optimize(ctx.h, P.nodes, P.n_nodes, P.edges, P.n_edges, C.byref(p), P.poses_out, P.edge_wrong, C.byref(self.res[b]))
            assert rc == 0, ctx.lib.mulls_last_error(ctx.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgo.txt"))
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", default="1,8,64,256")
    a = ap.parse_args()
    ctx = lib.Context(0)
    lines = ["# pose graph optimisation (mulls_pgo_optimize / mulls_pgo_optimize_batch) on one MI355X (gfx950): python tools/gpu_pgo.py",
             "# host clock around calls that end synchronised; median of %d after %d warm-ups (min, max), except the single-call column at B >= 64: median of %d after %d warm-ups; the restatement: tests/pgo_restated.py, numpy, one CPU thread, one run" % (a.repeat, a.warmup, max(3, a.repeat // 4), a.warmup)]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    # 1. the submap graph
    g = submap_graph(7)
    p = abi.pgo_params()
    t0 = time.perf_counter()
    r = R.solve(*g, R.params())
    cpu_ms = (time.perf_counter() - t0) * 1e3
    got = ctx.pgo_optimize(*g, p)
    ok = same(got, r)
    m = Marshalled([g])
    med, lo, hi = timed(lambda: m.singles(ctx, p), a.warmup, a.repeat)
    emit("submap graph, 300 nodes, 299 + 3 edges, %d iterations (%d successful), cost %.4e -> %.4e | single call %.3f ms (min %.3f, max %.3f) | restatement %.0f ms | %s" % (
        got[0].iterations, got[0].successful_steps, got[0].initial_cost, got[0].final_cost, med, lo, hi, cpu_ms, "the restatement's bits" if ok else "BITS DIFFER"))
    # 2. chains of 151
    pc = abi.pgo_params(t_limit=0.1, r_limit=0.01)
    for B in [int(x) for x in a.batch.split(",")]:
        probs = [G.chain(1000 + b, 151)[:4] for b in range(B)]
        t0 = time.perf_counter()
        r0 = R.solve(*probs[0], R.params(t_limit=0.1, r_limit=0.01))
        cpu_ms = (time.perf_counter() - t0) * 1e3
        batch = ctx.pgo_optimize_batch(probs, pc)
        singles = [ctx.pgo_optimize(*q, pc) for q in probs]
        ok = same(batch[0], r0) and all((x[1].view(np.uint64) == y[1].view(np.uint64)).all() and x[0].iterations == y[0].iterations for x, y in zip(batch, singles))
        its = [x[0].iterations for x in batch]
        m = Marshalled(probs)
        bm = timed(lambda: m.batch(ctx, pc), a.warmup, a.repeat)
        sm = timed(lambda: m.singles(ctx, pc), a.warmup, max(3, a.repeat // 4) if B >= 64 else a.repeat)
        emit("B %3d chains of 151 nodes, iterations %d .. %d | batch call %.3f ms (min %.3f, max %.3f) | %d single calls %.3f ms (min %.3f, max %.3f) | ratio %.2f | restatement, one problem %.0f ms | %s" % (
            B, min(its), max(its), bm[0], bm[1], bm[2], B, sm[0], sm[1], sm[2], sm[0] / bm[0], cpu_ms, "batch = singles = the restatement's bits" if ok else "BITS DIFFER"))
    emit("# the nodes and edges are marshalled into the C structs once, outside the timed calls; the calls take host arrays and return host arrays")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
