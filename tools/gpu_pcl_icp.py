"""Classical ICP registration on the device (mulls_pcl_icp / mulls_pcl_icp_batch): times on problems of the size of the tests' street_large (3 000
target and about 4 500 source points of a synthetic street), written to profiles/pcl_icp.txt.  Per call: the four combinations of step and
reciprocity, alone, and each cut after its first iteration (what the setup costs; the difference over the iterations is a tick); a batch of 64 against
64 single calls, with the bits compared; the numpy restatement (tests/pcl_icp_restated.py) on the fixture's street case for scale, with its bits
compared.  Medians over the repetitions after one warm-up call, host clock around synchronised calls.  Per kernel: run `--one` under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/gpu_pcl_icp.py --one).
usage: gpu_pcl_icp.py [--pairs N: distinct pairs, default 8] [--no-restated] [--one: the Point2Plane reciprocal call three times, for a kernel trace]
[--rows: only the rows tools/gpu_ab_single_calls.py reads (tools/reg_rows.py), for Point2Point and Point2Plane reciprocal; no file is written]"""
import os
import sys
import time
import warnings

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
sys.path.insert(0, os.path.join("tests", "golden"))
sys.path.insert(0, "tools")
warnings.filterwarnings("ignore")
import numpy as np

import reg_rows
from mulls_amd import abi, lib
from ndt_scenes import bound_of, street


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
    probs = []
    for k in range(n_pairs):
        A, B, _ = street(8 + k, 3000, 4500, (0.2, -0.1, -2.0), n_az=(420, 900))
        A, B = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(B, np.float32)
        probs.append(dict(tgt=A, src=B, tgt_bound=bound_of(A), src_bound=bound_of(B), init_guess=None))
    ctx = lib.Context(0)
    combos = [("Point2Point", dict()), ("Point2Point reciprocal", dict(use_reciprocal_correspondence=1)),
              ("Point2Plane", dict(metrics=abi.PCL_ICP_POINT2PLANE, te=abi.PCL_ICP_LLS)),
              ("Point2Plane reciprocal", dict(metrics=abi.PCL_ICP_POINT2PLANE, te=abi.PCL_ICP_LLS, use_reciprocal_correspondence=1))]
    if "--one" in argv:
        for _ in range(3):
            r = ctx.pcl_icp(**probs[0], params=abi.pcl_icp_params(**combos[3][1]))
        print("one call, three times: %d iterations" % r.iterations)
        return
    if "--rows" in argv:
        for name, over in (combos[0], combos[3]):
            prm = abi.pcl_icp_params(**over)
            reg_rows.rows("mulls_pcl_icp " + name, lambda: ctx.pcl_icp(**probs[0], params=prm),
                          lambda: ctx.pcl_icp(**probs[0], params=abi.pcl_icp_params(max_iter_num=1, **over)),
                          lambda: ctx.pcl_icp_batch([probs[k % n_pairs] for k in range(64)], prm))
        return
    os.makedirs("profiles", exist_ok=True)
    out = open(os.path.join("profiles", "pcl_icp.txt"), "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    say("classical ICP (mulls_pcl_icp), dis_thre_unit 1.5, neighbor_radius 2, the crop on; %d target and %d source points in the first pair"
        % (len(probs[0]["tgt"]), len(probs[0]["src"])))
    for name, over in combos:
        prm = abi.pcl_icp_params(**over)
        t1, r = timed(lambda: ctx.pcl_icp(**probs[0], params=prm), 7)
        t0, _ = timed(lambda: ctx.pcl_icp(**probs[0], params=abi.pcl_icp_params(max_iter_num=1, **over)), 7)
        say("%-23s one call: %.2f ms median of 7 (%d iterations, stop %d, %d pairs); with max_iter_num = 1 (uploads, crop, tables%s, one tick, fitness): %.2f ms; "
            "a further tick: %.3f ms" % (name + ",", t1 * 1e3, r.iterations, r.stop, r.n_corr, ", normals" if "metrics" in over else "", t0 * 1e3,
                                          (t1 - t0) * 1e3 / max(r.iterations - 1, 1)))
    for name, over in (combos[0], combos[3]):
        prm = abi.pcl_icp_params(**over)
        batch = [probs[k % n_pairs] for k in range(64)]
        tb, rb = timed(lambda: ctx.pcl_icp_batch(batch, prm), 3)
        ts, rs = timed(lambda: [ctx.pcl_icp(**p, params=prm) for p in batch], 3)
        same = all(bytes(a) == bytes(b) for a, b in zip(rb, rs))
        say("%-23s batch of 64: %.2f ms; 64 single calls: %.2f ms (medians of 3); ticks of the batch: %d; equal bits: %s"
            % (name + ",", tb * 1e3, ts * 1e3, max(r.iterations for r in rb), same))
    if "--no-restated" not in argv:
        import pcl_icp_restated as pr
        from make_pcl_icp_golden import cloud_of

        z = np.load(os.path.join("tests", "golden", "pcl_icp_cases.npz"))
        c = dict(tgt=cloud_of(z, "street_plane", "tgt"), src=cloud_of(z, "street_plane", "src"), tgt_bound=z["street_plane/tgt_bound"],
                 src_bound=z["street_plane/src_bound"])
        prm = pr.default_params(metrics=pr.POINT2PLANE, te=pr.LLS)
        t = time.perf_counter()
        ref = pr.pcl_icp(c["tgt"], c["src"], c["tgt_bound"], c["src_bound"], np.eye(4), prm)
        dt = time.perf_counter() - t
        td, rd = timed(lambda: ctx.pcl_icp(**c, params=abi.pcl_icp_params(metrics=abi.PCL_ICP_POINT2PLANE, te=abi.PCL_ICP_LLS)), 7)
        same = np.array(rd.T).reshape(4, 4).T.tobytes() == np.asarray(ref["T"], np.float64).tobytes() and rd.mse == ref["mse"] and rd.iterations == ref["iterations"]
        say("the numpy restatement on the fixture's street_plane case (1 500 / 400 points): %.2f s on one CPU thread; the device: %.2f ms; equal bits of T and mse: %s"
            % (dt, td * 1e3, same))
    out.close()


if __name__ == "__main__":
    main()
