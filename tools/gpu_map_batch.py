"""mulls_map_update_batch against as many mulls_map_update calls, in one process on one GPU.
usage: gpu_map_batch.py [--batch 1,8,64] [--removal] [--resident] [--updates 20] [--map-points 20000] [--out profiles/map_batch.txt]

B streams, each a map of about --map-points feature points (max_num_pts = that, so it stays there) and a drive of frames of the KITTI fixed-number sizes
(synth.R_SOURCE).  Every update runs twice: as one batched call on the maps and as B single calls on twin maps.  A single call is a batch of one, so the
"single calls" column is B groups of one against one group of B: what lock step saves, and at B = 1 the cost of the single entry point itself.  After every
update all twelve clouds, the pose and the report of every stream are compared byte for byte, and only then is a time printed.  Times are medians of the C
calls alone (arguments marshalled beforehand) over `--updates` updates after one warm-up update.  --removal: map-based dynamic removal on (tree_mode 1).
--resident: the frames are device clouds (lent by maps that hold them), as a feature block's would be."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mulls_amd import abi, lib, synth

MAP_COUNTS = {abi.GROUND: 7000, abi.PILLAR: 2500, abi.FACADE: 8500, abi.BEAM: 1200, abi.ROOF: 800}  # 20 000
N_SCENES, N_FRAMES = 4, 6


def scenes(map_points):
    out = []
    scale = map_points / 20000.0  # (a scan of 64 beams has about 120 000 returns: more beams for a larger map)
    counts = {c: int(n * scale) for c, n in MAP_COUNTS.items()}
    for s in range(N_SCENES):
        pair, _ = synth.make_pair(500 + s, n_beams=64 * max(1, round(scale / 5)), tgt_counts=counts, vertex_count=800)
        drive = synth.drive(500 + s, N_FRAMES + 1, n_beams=64, n_az=1900, counts=synth.R_SOURCE, vertex_count=300)[1:]
        out.append(([pair.tgt[c] for c in range(6)], drive))
    return out


def state(m):
    return [m.download(c).tobytes() for c in range(6)], [m.frame_download(c).tobytes() for c in range(6)], m.pose().tobytes()


def run(ctx, world, B, updates, removal, resident, map_points):
    P = abi.map_params(max_num_pts=map_points, kept_vertex_num=800, local_map_radius=80.0, rng_seed=1, map_based_dynamic_removal_on=int(removal),
                       tree_mode=1 if removal else 0, tree_used="111110" if removal else "000000")
    maps = [ctx.local_map(world[i % N_SCENES][0], np.eye(4)) for i in range(B)]
    twins = [ctx.local_map(world[i % N_SCENES][0], np.eye(4)) for i in range(B)]
    lenders = {}
    t_batch, t_single, launches, syncs = [], [], 0, 0
    report_bytes = abi.MapReport.ms_total.offset
    for u in range(updates + 1):
        items, results, stats = (abi.MapUpdateItem * B)(), (abi.MapBatchResult * B)(), abi.MapBatchStats()
        arrs, poses, keep = [], [], []
        for i in range(B):
            fc, fp = world[i % N_SCENES][1][(u + i // N_SCENES) % N_FRAMES]
            fp = fp @ synth.se3(0.0, 0.0, 0.0, 0.0, 0.0, np.deg2rad(0.01 * i))  # no two streams alike
            if resident:
                key = (i % N_SCENES, (u + i // N_SCENES) % N_FRAMES)
                if key not in lenders:
                    lenders[key] = ctx.local_map(fc, np.eye(4))
                fc = [lenders[key].cloud(c) for c in range(6)]
            arr, held = lib.LocalMap._clouds(fc)
            arrs.append(arr), poses.append(abi.colmajor16(fp)), keep.append(held)
            items[i].map, items[i].frame_down, items[i].frame_pose_lo = maps[i].h, arr, poses[i]
        reps = [abi.MapReport() for _ in range(B)]
        t0 = time.perf_counter()
        rc = ctx.lib.mulls_map_update_batch(ctx.h, items, B, C.byref(P), 0, results, C.byref(stats))
        t1 = time.perf_counter()
        for i in range(B):
            ctx.lib.mulls_map_update(ctx.h, twins[i].h, arrs[i], poses[i], C.byref(P), C.byref(reps[i]))
        t2 = time.perf_counter()
        assert rc == 0, ctx.lib.mulls_last_error(ctx.h)
        for i in range(B):  # equal bytes before any time is printed
            assert results[i].status == 0 and bytes(results[i].report)[:report_bytes] == bytes(reps[i])[:report_bytes], (u, i)
            assert state(maps[i]) == state(twins[i]), (u, i)
        if u:  # (update 0 warms up: allocations, module load)
            t_batch.append(t1 - t0), t_single.append(t2 - t1)
            launches, syncs = stats.n_kernel_launches, stats.n_syncs
    sizes = [int(results[0].report.n[c]) for c in range(6)]
    for m in maps + twins + list(lenders.values()):
        m.close()
    b, s = np.median(t_batch) * 1e3, np.median(t_single) * 1e3
    return ("B=%-3d removal=%d resident=%d | batch %8.3f ms (%.3f per map) | %d single calls %8.3f ms (%.3f per map) | ratio %.2f | launches %d waits %d per call | "
            "map sizes %s | bytes equal over %d updates" % (B, removal, resident, b, b / B, B, s, s / B, s / b, launches, syncs, sizes, updates + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--removal", action="store_true")
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--map-points", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join("profiles", "map_batch.txt"))
    a = ap.parse_args()
    assert a.updates >= 20, "medians of at least 20 updates"
    world = scenes(a.map_points)
    ctx = lib.Context(0)
    lines = [run(ctx, world, int(b), a.updates, a.removal, a.resident, a.map_points) for b in a.batch.split(",")]
    ctx.close()
    with open(a.out, "a") as f:
        for line in lines:
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
