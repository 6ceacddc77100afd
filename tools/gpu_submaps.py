"""The submap archive (mulls_submaps_*) at the size of a long run: 256 submaps of about 22 000 points (5.6 M records, 270 MB of arena).  Wall time per call,
median of 20 after 3 warm-ups, written to profiles/submaps.txt.  usage: gpu_submaps.py [--out PATH]
  mulls_submaps_set_poses   with update_bbx: all 256 submaps in one call, and as 256 single-submap calls; without update_bbx
  mulls_submaps_push_map    one local map of that size, device to device (bounds taken on the device: the map was set, not updated)
  mulls_submaps_push        the same clouds from host memory
  numpy                     tests/submaps_restated.py's bounds of the same 256 submaps on this machine's CPU, one run
Recorded, not gated."""
import ctypes as C
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.filterwarnings("ignore")
import numpy as np  # noqa: E402

import submaps_restated as R  # noqa: E402
from mulls_amd import abi, lib  # noqa: E402

N_SUBMAPS = 256
SIZES = (9000, 2500, 7000, 1500, 1200, 800)  # ground, pillar, facade, beam, roof, vertex: 22 000 points


def median_ms(fn, reps=20, warm=3):
    t = []
    for _ in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[warm:]))


def pose(k, drift=0.0):
    a = 0.02 * k + drift
    P = np.eye(4)
    P[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    P[:3, 3] = (8.0 * k + drift, 3.0 * np.sin(0.1 * k), 0.01 * k)
    return P


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "submaps.txt")
    rng = np.random.RandomState(0)
    clouds = []
    for n in SIZES:
        raw = np.zeros((n, abi.POINT_BYTES), np.uint8)
        raw[:, :12] = (rng.standard_normal((n, 3)) * (25.0, 25.0, 3.0)).astype(np.float32).view(np.uint8).reshape(n, 12)
        clouds.append(raw)
    per = sum(SIZES)
    ctx = lib.Context(0)
    m = ctx.local_map([abi.points_of(c) for c in clouds], pose(0))
    store = ctx.submaps(N_SUBMAPS * per, N_SUBMAPS)
    for k in range(N_SUBMAPS):
        store.push_map(m, id_in_strip=k)
        store.set_poses(k, [pose(k)], update_bbx=False)
    new = np.ascontiguousarray(np.concatenate([pose(k, 0.5).T.reshape(-1) for k in range(N_SUBMAPS)]))
    ptr = new.ctypes.data_as(C.POINTER(C.c_double))
    step = 16 * 8

    def one_call(bbx=1):
        assert ctx.lib.mulls_submaps_set_poses(ctx.h, store.h, 0, N_SUBMAPS, ptr, bbx) == 0

    def single_calls():
        for k in range(N_SUBMAPS):
            assert ctx.lib.mulls_submaps_set_poses(ctx.h, store.h, k, 1, C.cast(new.ctypes.data + k * step, C.POINTER(C.c_double)), 1) == 0

    lines = ["# tools/gpu_submaps.py on one MI355X: %d submaps of %d points (%d records, %.0f MB), MULLS_SUBMAP_CHUNK %d; wall time per call, median of 20 after 3 warm-ups"
             % (N_SUBMAPS, per, N_SUBMAPS * per, N_SUBMAPS * per * 48 / 1e6, abi.SUBMAP_CHUNK)]
    t_one = median_ms(one_call)
    batched = [list(store.info(k).bound) for k in range(N_SUBMAPS)]
    t_single = median_ms(single_calls, reps=5, warm=1)
    assert batched == [list(store.info(k).bound) for k in range(N_SUBMAPS)]
    t_poses = median_ms(lambda: one_call(0))
    lines.append("mulls_submaps_set_poses, update_bbx, one call for %d submaps: %.3f ms (%.1f GB/s of the 16 bytes read per record, %.1f GB/s of the 48-byte records it strides over)"
                 % (N_SUBMAPS, t_one, N_SUBMAPS * per * 16 / 1e6 / t_one, N_SUBMAPS * per * 48 / 1e6 / t_one))
    lines.append("mulls_submaps_set_poses, update_bbx, %d single-submap calls: %.3f ms = %.3f ms per call (ratio of the one call %.3f)" % (N_SUBMAPS, t_single, t_single / N_SUBMAPS, t_one / t_single))
    lines.append("mulls_submaps_set_poses, poses only: %.3f ms" % t_poses)
    lines.append("packed position mirror: not built (see DESIGN.md 7.7)")
    one = ctx.submaps(per, 1)

    def push_map():
        one.clear()
        one.push_map(m)

    def push_host():
        one.clear()
        one.push(clouds, pose(0))

    lines.append("mulls_submaps_push_map, one local map of %d points, device to device, bounds on the device: %.3f ms" % (per, median_ms(push_map)))
    lines.append("mulls_submaps_push, the same clouds from host memory: %.3f ms" % median_ms(push_host))
    merged = R.merge(clouds)
    t0 = time.perf_counter()
    want = [R.submap_bounds(merged, pose(k, 0.5))[1].tolist() for k in range(N_SUBMAPS)]
    t_np = (time.perf_counter() - t0) * 1e3
    assert want == batched
    lines.append("numpy restatement of the same %d bounds on this machine's CPU, one run: %.1f ms (the results are equal)" % (N_SUBMAPS, t_np))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    one.close()
    store.close()
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
