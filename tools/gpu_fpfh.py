"""FPFH descriptors and FPFH-based SAC-IA on the device (mulls_fpfh, mulls_coarse_reg_fpfhsac): times written to profiles/fpfh.txt.  The descriptor on
the tests' recovery scene (1 500 points, about 36 neighbours) and on the same surface at 20 000 and 100 000 points; the whole solver on the recovery
scene (1 500 / 1 200 points, 120 hypotheses) and on 20 000 / 16 000 points with 10 and 1 000 hypotheses; the numpy restatement (tests/fpfh_restated.py)
on the recovery scene for scale, with its bits compared.  Medians over the repetitions after one warm-up call, host clock around synchronised calls.  No
target was fixed in advance: the file records what was found.  Per kernel: run `--one` under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/gpu_fpfh.py --one).

--batch 1,8,64 times the batch entry points (mulls_compute_fpfh_batch, mulls_coarse_reg_fpfhsac_batch) against as many single calls, written to
profiles/fpfh_batch.txt: B distinct 1 500 / 1 200 pairs at 120 hypotheses; one 20 000-point target against B 16 000-point sources at 10 hypotheses (the
shared-descriptor case); the descriptors of B clouds of 20 000 points.  Same process and context, a batch call and its B single calls alternating,
medians after one warm-up of each, host clock around synchronised calls; the results' bytes are compared on the way.  The descriptor rows go through
the C calls into reused output arrays (see batch_table).
usage: gpu_fpfh.py [--no-restated] [--one: the recovery scene's solver three times, for a kernel trace] [--batch B,B,...]"""
import ctypes as C
import os
import sys
import time
import warnings

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
sys.path.insert(0, os.path.join("tests", "golden"))
warnings.filterwarnings("ignore")
import numpy as np

import fpfh_scenes
from mulls_amd import abi, lib


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), out


def pair(n_tgt, n_src, side, seed):
    A, An = fpfh_scenes.bumpy(seed, n_tgt, side)
    sel = np.sort(np.random.default_rng(seed + 1).choice(n_tgt, n_src, replace=False))
    B, Bn = fpfh_scenes.moved(A[sel], An[sel], np.linalg.inv(fpfh_scenes.sac_truth()))
    return (A, An), (B, Bn)


def alternating(batch, singles, reps):
    """-> median seconds of batch(), median seconds of singles(), and whether both gave the same bytes; the two alternate after one warm-up of each"""
    same = batch() == singles()
    tb, ts = [], []
    for _ in range(reps):
        t = time.perf_counter()
        batch()
        tb.append(time.perf_counter() - t)
        t = time.perf_counter()
        singles()
        ts.append(time.perf_counter() - t)
    return float(np.median(tb)), float(np.median(ts)), same


def result_bytes(results):
    return [bytes(r) for r in results]


def batch_table(ctx, sizes):
    os.makedirs("profiles", exist_ok=True)
    out = open(os.path.join("profiles", "fpfh_batch.txt"), "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    say("One batch call against B single calls (mulls_coarse_reg_fpfhsac_batch, mulls_compute_fpfh_batch), search_radius 0.4, host clouds of 48-byte records,")
    say("the default scratch limit; one MI355X; a batch call and its single calls alternating in one process and context, medians after a warm-up of each")
    small = dict(fpfh_scenes.RECOVERY)
    big = dict(search_radius=0.4, k_correspondences=2, max_iterations=10, min_sample_distance=2.0, max_correspondence_distance=0.05, seed=1)
    for B in sizes:
        reps = 7 if B <= 8 else 3
        pairs = [pair(1500, 1200, 8.0, 100 + 2 * b) for b in range(B)]
        p = abi.fpfhsac_params(**small)
        tb, ts, same = alternating(lambda: result_bytes(ctx.coarse_reg_fpfhsac_batch(pairs, p)), lambda: result_bytes([ctx.coarse_reg_fpfhsac(t, s, p) for t, s in pairs]), reps)
        say("B = %2d distinct 1 500 / 1 200 pairs, 120 hypotheses: batch %8.2f ms, single calls %8.2f ms (x %.2f), median of %d; equal bytes: %s"
            % (B, tb * 1e3, ts * 1e3, ts / tb, reps, same))
    for B in sizes:
        reps = 5 if B <= 8 else 3
        tgt = fpfh_scenes.bumpy(41, 20000, 29.2)
        srcs = []
        for b in range(B):
            sel = np.sort(np.random.default_rng(200 + b).choice(20000, 16000, replace=False))
            srcs.append(fpfh_scenes.moved(tgt[0][sel], tgt[1][sel], np.linalg.inv(fpfh_scenes.sac_truth())))
        probs = [(tgt, s) for s in srcs]
        p = abi.fpfhsac_params(**big)
        tb, ts, same = alternating(lambda: result_bytes(ctx.coarse_reg_fpfhsac_batch(probs, p)), lambda: result_bytes([ctx.coarse_reg_fpfhsac(t, s, p) for t, s in probs]), reps)
        say("B = %2d sources of 16 000 against one target of 20 000, 10 hypotheses: batch %8.2f ms, single calls %8.2f ms (x %.2f), median of %d; equal bytes: %s"
            % (B, tb * 1e3, ts * 1e3, ts / tb, reps, same))
    # The descriptors through the C calls into output arrays that are reused: with fresh arrays of 2.6 MB a cloud per call (Context.fpfh,
    # Context.fpfh_batch) either way spends tens of milliseconds of host time in this process on memory that was a copy's target and is freed again,
    # which is not what is compared here.
    fp = abi.fpfh_params(0.4)
    for B in sizes:
        reps = 7 if B <= 8 else 3
        raws = [abi.make_points(*fpfh_scenes.bumpy(300 + b, 20000, 29.2)) for b in range(B)]
        arr = (abi.Cloud * B)(*[abi.as_cloud(r) for r in raws])
        outs = [[(np.zeros((len(r), 33), np.float32), np.zeros(len(r), np.uint32)) for r in raws] for _ in range(2)]
        hp, kp = (C.c_void_p * B)(*[h.ctypes.data for h, _ in outs[0]]), (C.c_void_p * B)(*[k.ctypes.data for _, k in outs[0]])

        def batch():
            assert ctx.lib.mulls_compute_fpfh_batch(ctx.h, arr, B, C.byref(fp), hp, kp, 0) == 0
            return True

        def singles():
            for b in range(B):
                assert ctx.lib.mulls_fpfh(ctx.h, C.byref(arr[b]), C.byref(fp), outs[1][b][0].ctypes.data, outs[1][b][1].ctypes.data) == 0
            return True

        tb, ts, _ = alternating(batch, singles, reps)
        same = all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(*outs))
        say("B = %2d clouds of 20 000 points, descriptors (C calls, reused outputs): batch %8.2f ms, single calls %8.2f ms (x %.2f), median of %d; equal bytes: %s"
            % (B, tb * 1e3, ts * 1e3, ts / tb, reps, same))
    out.close()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    ctx = lib.Context(0)
    if "--batch" in argv:
        batch_table(ctx, [int(v) for v in argv[argv.index("--batch") + 1].split(",")])
        return
    rec = fpfh_scenes.sac_cases()["sac_recovery"]
    tgt, src, prm = (rec["tgt"], rec["tgt_nrm"]), (rec["src"], rec["src_nrm"]), abi.fpfhsac_params(**rec["prm"])
    if "--one" in argv:
        for _ in range(3):
            r = ctx.coarse_reg_fpfhsac(tgt, src, prm)
        print("one call, three times: hypothesis %d of %d" % (r.best_iteration, r.iterations))
        return
    os.makedirs("profiles", exist_ok=True)
    out = open(os.path.join("profiles", "fpfh.txt"), "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    say("FPFH and SAC-IA (mulls_fpfh, mulls_coarse_reg_fpfhsac), search_radius 0.4 (feature radius 0.8), host clouds of 48-byte records; one MI355X")
    fp = abi.fpfh_params(0.4)
    for n, side in ((1500, 8.0), (20000, 29.2), (100000, 65.3)):
        cloud = tgt if n == 1500 else fpfh_scenes.bumpy(31, n, side)
        t, (h, k) = timed(lambda: ctx.fpfh(cloud, fp), 7)
        say("mulls_fpfh, %6d points (%.1f neighbours a point, the largest %d): %.2f ms median of 7" % (n, k.mean(), k.max(), t * 1e3))
    t, r = timed(lambda: ctx.coarse_reg_fpfhsac(tgt, src, prm), 7)
    say("mulls_coarse_reg_fpfhsac, the tests' recovery scene (1 500 / 1 200 points, %d hypotheses, k_correspondences %d): %.2f ms median of 7; hypothesis %d wins"
        % (prm.max_iterations, prm.k_correspondences, t * 1e3, r.best_iteration))
    big_t, big_s = pair(20000, 16000, 29.2, 41)
    for iters in (10, 1000):
        p = abi.fpfhsac_params(search_radius=0.4, k_correspondences=2, max_iterations=iters, min_sample_distance=2.0, max_correspondence_distance=0.05, seed=1)
        t, r = timed(lambda: ctx.coarse_reg_fpfhsac(big_t, big_s, p), 3)
        say("mulls_coarse_reg_fpfhsac, 20 000 / 16 000 points, %4d hypotheses (each a brute-force nearest-target pass of 16 000 x 20 000): %.2f ms median of 3; "
            "hypothesis %d wins, fitness %.3g" % (iters, t * 1e3, r.best_iteration, r.fitness))
    if "--no-restated" not in argv:
        import fpfh_restated as fr

        t0 = time.perf_counter()
        want_h, want_k = fr.fpfh(tgt[0], tgt[1], 0.4)
        t1 = time.perf_counter()
        want = fr.fpfhsac(tgt[0], tgt[1], src[0], src[1], fr.fpfhsac_default_params(**rec["prm"]))
        t2 = time.perf_counter()
        h, k = ctx.fpfh(tgt, fp)
        r = ctx.coarse_reg_fpfhsac(tgt, src, prm)
        same = (h.tobytes() == want_h.tobytes() and k.tobytes() == want_k.tobytes() and np.array(r.T).reshape(4, 4).T.tobytes() == want["T"].tobytes()
                and r.best_error == want["best_error"] and r.fitness == want["fitness"] and r.best_iteration == want["best_iteration"])
        say("the numpy restatement on the recovery scene, one CPU thread: the descriptor of 1 500 points %.2f s, the whole solver %.2f s; equal bits of the descriptors, "
            "T, best_error and fitness: %s" % (t1 - t0, t2 - t1, same))
    out.close()


if __name__ == "__main__":
    main()
