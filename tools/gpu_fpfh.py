"""FPFH descriptors and FPFH-based SAC-IA on the device (mulls_fpfh, mulls_coarse_reg_fpfhsac): times written to profiles/fpfh.txt.  The descriptor on
the tests' recovery scene (1 500 points, about 36 neighbours) and on the same surface at 20 000 and 100 000 points; the whole solver on the recovery
scene (1 500 / 1 200 points, 120 hypotheses) and on 20 000 / 16 000 points with 10 and 1 000 hypotheses; the numpy restatement (tests/fpfh_restated.py)
on the recovery scene for scale, with its bits compared.  Medians over the repetitions after one warm-up call, host clock around synchronised calls.  No
target was fixed in advance: the file records what was found.  Per kernel: run `--one` under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/gpu_fpfh.py --one).
usage: gpu_fpfh.py [--no-restated] [--one: the recovery scene's solver three times, for a kernel trace]"""
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


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    ctx = lib.Context(0)
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
