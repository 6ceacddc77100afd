"""NDT registration on the device (mulls_ndt / mulls_ndt_batch): times and accuracy on the synthetic drive of tools/gpu_odometry.py, written to
profiles/ndt.txt.  One 64-beam scan (about 121 600 returns) against the next: one call; batches of 1, 8 and 64 such pairs against as many single calls;
the numpy restatement (tests/ndt_restated.py) on the first pair for scale, with its bits compared; the pose error of NDT and of scan-to-scan mm_lls_icp
against the drive's ground truth on the same pairs.  usage: gpu_ndt.py [--pairs N: distinct pairs, default 8] [--no-restated] [--rows: only the rows
tools/gpu_ab_single_calls.py reads (tools/reg_rows.py); no file is written]"""
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
from mulls_amd import abi, lib, synth


def raw_drive(seed, n_frames, n_beams=64, n_az=1900, step=0.9):
    """the drive of tools/gpu_odometry.py"""
    rng = np.random.default_rng(seed)
    scene = synth.Scene(seed)
    world0 = synth.se3(0, 0, scene.sensor_height)
    pose = np.eye(4)
    frames = []
    for k in range(n_frames):
        s = synth.raycast(scene, world0 @ pose, n_beams, n_az, seed=seed * 7 + k)
        frames.append((abi.make_points(s["xyz"], np.zeros_like(s["xyz"]), s["intensity"], s["t"]), pose.copy()))
        pose = pose @ synth.se3(rng.uniform(0.7, 1.3) * step, rng.normal(0, 0.03), rng.normal(0, 0.01), 0, 0, np.deg2rad(rng.normal(0, 1.0)))
    return frames


def block_of(ex):
    """(full clouds, down clouds) in class order ground, pillar, facade, beam, roof, vertex from the clouds of mulls_extract_features"""
    c = ex[abi.EX_PILLAR:]
    full = [ex[abi.EX_GROUND], c[abi.CL_PILLAR], c[abi.CL_FACADE], c[abi.CL_BEAM], c[abi.CL_ROOF], c[abi.CL_VERTEX]]
    down = [ex[abi.EX_GROUND_DOWN], c[abi.CL_PILLAR_DOWN], c[abi.CL_FACADE_DOWN], c[abi.CL_BEAM_DOWN], c[abi.CL_ROOF_DOWN], c[abi.CL_VERTEX]]
    return [abi.points_of(x) for x in full], [abi.points_of(x) for x in down]


def bound(pts):
    return np.concatenate([pts.min(axis=0), pts.max(axis=0)]).astype(np.float64)


def timed(fn, reps):
    fn()
    best = 1e30
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t)
    return best, out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    n_pairs = int(argv[argv.index("--pairs") + 1]) if "--pairs" in argv else 8
    frames = raw_drive(11, n_pairs + 1)
    xyz = [np.ascontiguousarray(np.stack([f[0]["x"], f[0]["y"], f[0]["z"]], axis=1), dtype=np.float32) for f in frames]
    gt = [np.linalg.inv(frames[k][1]) @ frames[k + 1][1] for k in range(n_pairs)]  # frame k + 1 in frame k
    probs = [dict(tgt=xyz[k], src=xyz[k + 1], tgt_bound=bound(xyz[k]), src_bound=bound(xyz[k + 1]), init_guess=None) for k in range(n_pairs)]
    ctx = lib.Context(0)
    prm = abi.ndt_params()
    if "--rows" in argv:
        reg_rows.rows("mulls_ndt", lambda: ctx.ndt(**probs[0], params=prm), lambda: ctx.ndt(**probs[0], params=abi.ndt_params(max_iterations=1)),
                      lambda: ctx.ndt_batch([probs[k % n_pairs] for k in range(64)], prm))
        return
    os.makedirs("profiles", exist_ok=True)
    out = open("profiles/ndt.txt", "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    say("NDT (mulls_ndt), default parameters (1 m leaves, DIRECT7), scan k + 1 onto scan k of the synthetic drive; %d and %d points in the first pair" % (len(xyz[0]), len(xyz[1])))
    t1, r = timed(lambda: ctx.ndt(**probs[0], params=prm), 5)
    say("one call: %.2f ms (%d iterations, %d evaluations, %d of %d leaves used, %d source points after the crop)" % (t1 * 1e3, r.iterations, r.evaluations, r.n_leaves_used, r.n_leaves, r.n_src))
    for B in (1, 8, 64):
        batch = [probs[k % n_pairs] for k in range(B)]
        tb, rb = timed(lambda: ctx.ndt_batch(batch, prm), 2)
        ts, rs = timed(lambda: [ctx.ndt(**p, params=prm) for p in batch], 2)
        same = all(bytes(a) == bytes(b) for a, b in zip(rb, rs))
        say("batch of %2d: %.2f ms; %2d single calls: %.2f ms; equal bits: %s" % (B, tb * 1e3, B, ts * 1e3, same))
    if "--no-restated" not in argv:
        import ndt_restated as nr

        t = time.perf_counter()
        ref = nr.ndt(xyz[0], xyz[1], probs[0]["tgt_bound"], probs[0]["src_bound"], np.eye(4), with_fitness=False)
        dt = time.perf_counter() - t
        T = np.array(r.T).reshape(4, 4).T
        same = T.tobytes() == np.asarray(ref["T"], np.float64).tobytes() and r.trans_probability == ref["trans_probability"] and r.iterations == ref["iterations"]
        say("the numpy restatement on the first pair, without the fitness pass: %.1f s on one CPU thread; equal bits of T and trans_probability: %s" % (dt, same))
    # accuracy: NDT with upstream's constants, NDT with transformation_epsilon 0.01 (it may then take steps beyond the first few), scan-to-scan mm_lls_icp
    X = abi.extract_params(ground=abi.ground_params(fixed_num_downsampling=1, down_ground_fixed_num=800, rng_seed=1),
                           classify=abi.classify_params(neighbor_searching_radius=0.7, neighbor_k=25, neigh_k_min=7, curvature_thre=0.08, fixed_num_downsampling=1,
                                                        unground_down_fixed_num=20000, pillar_down_fixed_num=400, facade_down_fixed_num=1200, beam_down_fixed_num=200,
                                                        roof_down_fixed_num=200, rng_seed=1),
                           apply_dist_filter=1, min_dist_used=1.5, max_dist_used=120.0)
    P = abi.kitti_params(dis_thre_unit=1.5, used_feature_type="111110")
    blocks = [block_of(ctx.extract_features(f[0], X)) for f in frames]
    fine = abi.ndt_params(transformation_epsilon=0.01)
    off = synth.se3(0.2, 0.05, 0.0, yaw=np.deg2rad(1.0))  # a guess this far from the truth: what a constant-velocity model leaves
    say("pose error against the ground truth (translation m, rotation rad); left: identity guess; right: a guess 0.21 m and 1 degree off the truth")
    say("pair   omp_ndt (upstream constants)   omp_ndt (epsilon 0.01)   mm_lls_icp (scan to scan)   true motion m | omp_ndt   omp_ndt (epsilon 0.01)   mm_lls_icp")
    for k in range(n_pairs):
        a = ctx.ndt(**probs[k], params=prm)
        b = ctx.ndt(**probs[k], params=fine)
        pair = abi.PairData(blocks[k][0], blocks[k + 1][1], tgt_bound=list(bound(xyz[k])))
        c = ctx.icp(pair, P)[0]
        ea, eb = (synth.pose_error(np.array(x.T).reshape(4, 4).T, gt[k]) for x in (a, b))
        ec = synth.pose_error(c.T_matrix(), gt[k])
        G = gt[k] @ off
        withg = dict(probs[k], init_guess=G)
        ga, gb = ctx.ndt(**withg, params=prm), ctx.ndt(**withg, params=fine)
        gc = ctx.icp(abi.PairData(blocks[k][0], blocks[k + 1][1], init_guess=G, tgt_bound=list(bound(xyz[k]))), P)[0]
        fa, fb = (synth.pose_error(np.array(x.T).reshape(4, 4).T, gt[k]) for x in (ga, gb))
        fc = synth.pose_error(gc.T_matrix(), gt[k])
        say("%4d   %.3f %.4f (%2d it)   %.3f %.4f (%2d it)   %.3f %.4f (code %d)   %.3f | %.3f %.4f (%2d it)   %.3f %.4f (%2d it)   %.3f %.4f (code %d)"
            % (k, ea[0], ea[1], a.iterations, eb[0], eb[1], b.iterations, ec[0], ec[1], c.code, float(np.linalg.norm(gt[k][:3, 3])),
               fa[0], fa[1], ga.iterations, fb[0], fb[1], gb.iterations, fc[0], fc[1], gc.code))
    out.close()


if __name__ == "__main__":
    main()
