"""Voxelised GICP registration on the device (mulls_gicp / mulls_gicp_batch): times on the synthetic drive of tools/gpu_odometry.py, written to
profiles/gicp.txt.  One 64-beam scan (about 121 600 returns) against the next: one call, and the same call cut after its first iteration (what the
setup costs); batches of 1, 8 and 64 such pairs against as many single calls; the numpy restatement (tests/gicp_restated.py) on one small case of the
fixture for scale, with its bits compared; the pose error against the drive's ground truth.  Medians over the repetitions after one warm-up call.
usage: gpu_gicp.py [--pairs N: distinct pairs, default 8] [--no-restated] [--one: the single call only, for a kernel trace] [--rows: only the rows
tools/gpu_ab_single_calls.py reads (tools/reg_rows.py); no file is written]"""
import json
import os
import sys
import time
import warnings

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
sys.path.insert(0, "tools")
warnings.filterwarnings("ignore")
import numpy as np

import reg_rows
from gpu_ndt import bound, raw_drive
from mulls_amd import abi, lib, synth


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    n_pairs = int(argv[argv.index("--pairs") + 1]) if "--pairs" in argv else 8
    frames = raw_drive(11, n_pairs + 1)
    xyz = [np.ascontiguousarray(np.stack([f[0]["x"], f[0]["y"], f[0]["z"]], axis=1), dtype=np.float32) for f in frames]
    gt = [np.linalg.inv(frames[k][1]) @ frames[k + 1][1] for k in range(n_pairs)]  # frame k + 1 in frame k
    probs = [dict(tgt=xyz[k], src=xyz[k + 1], tgt_bound=bound(xyz[k]), src_bound=bound(xyz[k + 1]), init_guess=None) for k in range(n_pairs)]
    ctx = lib.Context(0)
    prm = abi.gicp_params()
    if "--one" in argv:
        for _ in range(3):
            r = ctx.gicp(**probs[0], params=prm)
        print("one call, three times: %d iterations" % r.iterations)
        return
    if "--rows" in argv:
        reg_rows.rows("mulls_gicp", lambda: ctx.gicp(**probs[0], params=prm), lambda: ctx.gicp(**probs[0], params=abi.gicp_params(max_iterations=1)),
                      lambda: ctx.gicp_batch([probs[k % n_pairs] for k in range(64)], prm))
        return
    os.makedirs("profiles", exist_ok=True)
    out = open("profiles/gicp.txt", "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    say("VGICP (mulls_gicp), default parameters (1 m voxels, 20 neighbours), scan k + 1 onto scan k of the synthetic drive; %d and %d points in the first pair"
        % (len(xyz[0]), len(xyz[1])))
    t1, r = timed(lambda: ctx.gicp(**probs[0], params=prm), 5)
    say("one call: %.2f ms median of 5 (%d iterations, stop %d, %d voxels, %d of %d source points with a voxel)" % (t1 * 1e3, r.iterations + 1, r.stop, r.n_voxels, r.n_corr, r.n_src))
    t0, _ = timed(lambda: ctx.gicp(**probs[0], params=abi.gicp_params(max_iterations=1)), 5)
    say("the same call with max_iterations = 1 (uploads, crop, covariances, voxel map, one tick, fitness): %.2f ms; a further tick: %.3f ms"
        % (t0 * 1e3, (t1 - t0) * 1e3 / max(r.iterations, 1)))
    for B in (1, 8, 64):
        batch = [probs[k % n_pairs] for k in range(B)]
        tb, rb = timed(lambda: ctx.gicp_batch(batch, prm), 2)
        ts, rs = timed(lambda: [ctx.gicp(**p, params=prm) for p in batch], 2)
        same = all(bytes(a) == bytes(b) for a, b in zip(rb, rs))
        say("batch of %2d: %.2f ms; %2d single calls: %.2f ms; equal bits: %s" % (B, tb * 1e3, B, ts * 1e3, same))
    if "--no-restated" not in argv:
        import gicp_restated as gr

        z = np.load(os.path.join("tests", "golden", "gicp_cases.npz"))
        c = {k: z["street/" + k] for k in ("tgt", "src", "tgt_bound", "src_bound", "guess")}
        t = time.perf_counter()
        ref = gr.gicp(c["tgt"], c["src"], c["tgt_bound"], c["src_bound"], c["guess"])
        dt = time.perf_counter() - t
        td, rd = timed(lambda: ctx.gicp(c["tgt"], c["src"], c["tgt_bound"], c["src_bound"], c["guess"]), 5)
        same = np.array(rd.T).reshape(4, 4).T.tobytes() == np.asarray(ref["T"], np.float64).tobytes() and rd.loss == ref["loss"] and rd.iterations == ref["iterations"]
        say("the numpy restatement on the fixture's street case (1 500 / 400 points): %.2f s on one CPU thread; the device: %.2f ms; equal bits of T and loss: %s"
            % (dt, td * 1e3, same))
    say("pose error against the ground truth (translation m, rotation rad), identity guess")
    say("pair   omp_gicp                    true motion m")
    for k in range(n_pairs):
        a = ctx.gicp(**probs[k], params=prm)
        ea = synth.pose_error(np.array(a.T).reshape(4, 4).T, gt[k])
        say("%4d   %.3f %.4f (%2d it, stop %d)   %.3f" % (k, ea[0], ea[1], a.iterations + 1, a.stop, float(np.linalg.norm(gt[k][:3, 3]))))
    out.close()


if __name__ == "__main__":
    main()
