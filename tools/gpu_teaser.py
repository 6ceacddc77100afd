"""The TEASER coarse-registration solver (mulls_coarse_reg_teaser_indexed) timed on the device: wall time per call, host key points and index lists in to
result out, median of 20 after 2 warm-ups (3 calls, the first among them, where one call takes more than a second: the host clique search is the whole of it), on the
demo scans' key-point pair lists of 517, 294, 1 543 and 2 840 pairs (tests/golden/ncc_demo.npz) at the noise bounds 0.25 and 1.0, and on 4 000 random pairs
with 5 % planted inliers; one row takes the key points from device memory ("dev").  The host clique search's time is reported on its own (result.search_seconds), and mulls_coarse_reg_ransac_indexed on the same
pairs next to it.  The search is given --budget nodes (default 2^20, so that a timing run ends; the library's default is 2^28).

    python tools/gpu_teaser.py                 the table
    python tools/gpu_teaser.py --calls 3       three calls per case and nothing else: the run to put under `rocprofv3 --kernel-trace --stats -- ...`
    python tools/gpu_teaser.py --search both   the clique search on the host, on the device (MULLS_OPT_TEASER_DEVICE_SEARCH) or both: with `both`, one call of
                                               each per case, search_seconds and clique_nodes of either, and whether every result field agrees
    python tools/gpu_teaser.py --batch 1,8,64  mulls_coarse_reg_teaser_batch: B copies of a demo pair list (recip_0_15 and fixed300_0_15 at the bound 0.25), and a
                                               mixed list of B problems (the four small pair lists in turn), through the batch entry and as B single calls on the
                                               same context: every result field compared, both wall times as the median of 20.  The two paths compile one kernel
                                               text; the single call passes launch arguments where the batch reads a descriptor, so the "B single calls" column
                                               is B times the per-call cost (launches, copies, synchronisations) and the ratio what sharing them among B saves
    --cases fixed2000_0_15:1.0,nn_15_0:0.25    only these rows (pair list of tests/golden/ncc_demo.npz : bound); with --search device --calls 1, the run to trace the search's kernels with
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mulls_amd import abi, lib  # noqa: E402


def random_pairs(seed, n, share=0.05, bound=1.0):
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-40.0, -40.0, -3.0]), np.array([40.0, 40.0, 10.0])
    src = rng.uniform(lo, hi, (n, 3))
    a = rng.uniform(0.2, 1.2)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    tgt = src @ R.T + rng.uniform([-8, -8, -0.5], [8, 8, 0.5]) + rng.uniform(-0.1 * bound, 0.1 * bound, (n, 3))
    out = rng.random(n) >= share
    tgt[out] = rng.uniform(lo, hi, (int(out.sum()), 3))
    rec = []
    for p in (tgt, src):
        f = np.zeros((n, 12), np.float32)
        f[:, :3] = p
        rec.append(f.view(np.uint8).reshape(n, 48))
    idx = np.arange(n, dtype=np.int32)
    return rec[0], rec[1], idx, idx


FIELDS = ("status", "n_edges", "max_core", "clique_size", "clique_exact", "gnc_iterations", "n_rotation_inliers", "n_translation_inliers")


def compare(ctx, name, nb, kt, ks, ti, si, P):
    """one call with the host search and one with the device search on the same context: the two efforts, and whether every result field agrees"""
    got = {}
    for side, value in (("host", 0), ("device", 1)):
        ctx.set_option(abi.OPT_TEASER_DEVICE_SEARCH, value)
        t0 = time.perf_counter()
        res, clique = ctx.coarse_reg_teaser(kt, ks, P, tgt_idx=ti, src_idx=si)
        got[side] = (res, clique, time.perf_counter() - t0)
    (a, ca, ta), (b, cb, tb) = got["host"], got["device"]
    same = all(getattr(a, f) == getattr(b, f) for f in FIELDS) and np.array_equal(ca, cb) and bytes(a.T) == bytes(b.T) and np.float64(a.cost).tobytes() == np.float64(b.cost).tobytes()
    print("%-15s N %5d  bound %.2f  clique %4d | host search %12.3f ms %10d nodes (%s), call %12.3f ms | device search %12.3f ms %10d nodes (%s), call %12.3f ms | every field %s"
          % (name, len(ti), nb, a.clique_size, a.search_seconds * 1e3, a.clique_nodes, "exact" if a.clique_exact else "budget", ta * 1e3, b.search_seconds * 1e3, b.clique_nodes,
             "exact" if b.clique_exact else "budget", tb * 1e3, "agrees" if same else "DIFFERS"), flush=True)


def same_result_but_nodes(a, ca, b, cb):
    """the device search's effort need not repeat: every field but clique_nodes"""
    return (all(getattr(a, f) == getattr(b, f) for f in FIELDS) and np.array_equal(ca, cb) and bytes(a.T) == bytes(b.T)
            and np.float64(a.cost).tobytes() == np.float64(b.cost).tobytes())


def same_result(a, ca, b, cb):
    return same_result_but_nodes(a, ca, b, cb) and a.clique_nodes == b.clique_nodes


def batch_mode(sizes, budget, search, calls):
    """B problems through mulls_coarse_reg_teaser_batch and as B calls of mulls_coarse_reg_teaser_indexed (the same kernel text, one problem per call): equality of
    every field, and the two wall times"""
    Z = np.load(os.path.join(ROOT, "tests", "golden", "ncc_demo.npz"))

    def problem(name):
        a, b = (0, 15) if name.endswith("0_15") else (15, 0)
        pr = Z[name + "_pairs"]
        return dict(tgt=Z["kpts_%d" % a], src=Z["kpts_%d" % b], tgt_idx=pr[:, 0], src_idx=pr[:, 1])

    small = ("recip_0_15", "fixed300_0_15", "recip_15_0", "fixed300_15_0")
    ctx = lib.Context(0)
    ctx.set_option(abi.OPT_TEASER_DEVICE_SEARCH, 1 if search == "device" else 0)
    P = abi.teaser_params(0.25, 8, budget)
    for B in sizes:
        for label, names in (("recip_0_15", ["recip_0_15"] * B), ("fixed300_0_15", ["fixed300_0_15"] * B), ("mixed", [small[k % 4] for k in range(B)])):
            problems = [problem(n) for n in names]

            def batch():
                t0 = time.perf_counter()
                out = ctx.coarse_reg_teaser_batch(problems, P)
                return time.perf_counter() - t0, out

            def singles():
                t0 = time.perf_counter()
                out = [ctx.coarse_reg_teaser(q["tgt"], q["src"], P, tgt_idx=q["tgt_idx"], src_idx=q["src_idx"]) for q in problems]
                return time.perf_counter() - t0, out

            (_, got), (_, want) = batch(), singles()
            if calls:  # the run to trace: a few batch calls and nothing else
                for _ in range(calls - 1):
                    batch()
                continue
            eq = same_result_but_nodes if search == "device" else same_result
            same = all(eq(a, ca, b, cb) for (a, ca), (b, cb) in zip(got, want))
            tb, ts = sorted(batch()[0] for _ in range(20)), sorted(singles()[0] for _ in range(20))
            print("%-14s B %3d  bound 0.25  GNC iterations %s | batch call, median of 20: %9.3f ms (min %.3f, max %.3f) | %d single calls: %9.3f ms (min %.3f, max %.3f)"
                  " | ratio %.2f | every field %s" % (label, B, sorted(set(r.gnc_iterations for r, _ in got)), tb[10] * 1e3, tb[0] * 1e3, tb[-1] * 1e3, B, ts[10] * 1e3,
                                                      ts[0] * 1e3, ts[-1] * 1e3, ts[10] / tb[10], "agrees" if same else "DIFFERS"), flush=True)
    ctx.close()


def main():
    arg = lambda k, d: type(d)(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d  # noqa: E731
    calls, budget, search, only = arg("--calls", 0), arg("--budget", 1 << 20), arg("--search", "host"), arg("--cases", "")
    if search not in ("host", "device", "both"):
        raise SystemExit("--search host|device|both")
    if "--batch" in sys.argv:
        return batch_mode([int(b) for b in arg("--batch", "1").split(",")], budget, search, calls)
    Z = np.load(os.path.join(ROOT, "tests", "golden", "ncc_demo.npz"))
    cases = []
    for name in ("fixed300_0_15", "recip_0_15", "fixed2000_0_15", "nn_0_15"):
        pr = Z[name + "_pairs"]
        for nb in (0.25, 1.0):
            cases.append((name, nb, Z["kpts_0"], Z["kpts_15"], pr[:, 0], pr[:, 1]))
    cases.append(("random_4000", 1.0) + random_pairs(4000, 4000))
    if only:  # any pair list of the file, either direction
        cases = []
        for c in only.split(","):
            name, nb = c.split(":")[0], float(c.split(":")[1])
            a, b = (0, 15) if name.endswith("0_15") else (15, 0)
            pr = Z[name + "_pairs"]
            cases.append((name, nb, Z["kpts_%d" % a], Z["kpts_%d" % b], pr[:, 0], pr[:, 1]))
    ctx = lib.Context(0)
    ctx.set_option(abi.OPT_TEASER_DEVICE_SEARCH, 1 if search == "device" else 0)
    if not only:  # one pair list on device-resident key points: the gather runs on the device
        from gpu_ransac import DevBuf

        pr = Z["recip_0_15_pairs"]
        resident = DevBuf(np.ascontiguousarray(Z["kpts_0"])), DevBuf(np.ascontiguousarray(Z["kpts_15"]))
        cases.append(("recip_0_15 dev", 0.25, resident[0].cloud(), resident[1].cloud(), pr[:, 0], pr[:, 1]))
    for name, nb, kt, ks, ti, si in cases:
        P = abi.teaser_params(nb, 8, budget)
        if search == "both":
            compare(ctx, name, nb, kt, ks, ti, si, P)
            continue
        RP = abi.ransac_params(nb, 8, 20000, 1)

        def call():
            t0 = time.perf_counter()
            res, _ = ctx.coarse_reg_teaser(kt, ks, P, cap=0, tgt_idx=ti, src_idx=si)
            return time.perf_counter() - t0, res

        def ransac():
            t0 = time.perf_counter()
            ctx.coarse_reg_ransac(kt, ks, RP, cap=0, tgt_idx=ti, src_idx=si)
            return time.perf_counter() - t0

        first, res = call()
        if calls:
            for _ in range(calls - 1 if first < 1.0 else 0):  # (a call the host search dominates is traced once)
                call()
            continue
        n_calls = 20 if first < 1.0 else 3
        if n_calls == 20:
            call()
        runs = [call() for _ in range(n_calls)] if n_calls == 20 else [(first, res), call(), call()]
        ts, ss = sorted(r[0] for r in runs), sorted(r[1].search_seconds for r in runs)
        ransac(), ransac()
        rs = sorted(ransac() for _ in range(20))
        print("%-15s N %5d  bound %.2f  status %2d  edges %7d  max core %4d  clique %4d (%s, %9d nodes)  GNC iterations %3d  rotation inliers %6d | wall median of %2d: %10.3f ms"
              "  (min %.3f, max %.3f) | host search alone %10.3f ms | RANSAC (20000 iterations, refined) on the same pairs %8.3f ms"
              % (name, len(ti), nb, res.status, res.n_edges, res.max_core, res.clique_size, "exact" if res.clique_exact else "budget", res.clique_nodes,
                 res.gnc_iterations, res.n_rotation_inliers, n_calls, ts[n_calls // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3, ss[n_calls // 2] * 1e3, rs[10] * 1e3), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
