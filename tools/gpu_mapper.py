"""Scan preparation and the merged-map builder (mulls_scan_prepare, mulls_mapper_add) on one 64-beam synthetic scan of about 121 k points: wall time per call,
median of 20 after 3 warm-ups.  usage: gpu_mapper.py [--cpu] [--calls N]
  mulls_scan_prepare   host round trip (upload, passes, download of what stays) and in place on a device buffer; the frame loop's steps (dist filter,
                       calibration 0.195 degrees) and the export's (calibration, dist filter 2 - 80 m, ratio 5, time ratio from stamps)
  mulls_mapper_add     batches of 1, 8 and 64 frames (host scans and device-resident scans) against as many single-frame calls in the same run, per frame
  --cpu                adds tests/scanprep_harness.cpp (the same arithmetic, -O3, one thread; upstream's loops are serial) on the same frames
  --calls N            only N calls of the 64-frame mulls_mapper_add on device-resident scans: the run to trace with rocprofv3 --kernel-trace --stats
  --report TXT CSV     no device needed: profiles/mapper_kernel_stats.txt from this tool's output (TXT) and the trace's kernel_stats.csv (CSV), each pass
                       next to the bytes it moves by its definition"""
import ctypes as C
import os
import struct
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
import numpy as np  # noqa: E402

from mulls_amd import abi, lib, synth  # noqa: E402


def median_ms(fn, reps=20, warm=3, before=None):
    t = []
    for k in range(warm + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[warm:]))


class DevBuf:
    def __init__(self, raw):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.raw, self.p = np.ascontiguousarray(raw), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), self.raw.nbytes) == 0
        self.upload()

    def upload(self):
        assert self.hip.hipMemcpy(self.p, C.c_void_p(self.raw.ctypes.data), self.raw.nbytes, 1) == 0

    def cloud(self):
        c = abi.Cloud()
        c.pts, c.n, c.stride = self.p.value, len(self.raw), abi.POINT_BYTES
        return c


def harness_ms(frames, p, reps):
    exe = os.path.join(ROOT, "tools", "_bin", "scanprep_harness")
    if not os.path.exists(exe):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", os.path.join(ROOT, "tests", "scanprep_harness.cpp"), "-o", exe])
    fin = os.path.join(ROOT, "tools", "_bin", "mapper_in.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<IIQ", len(frames), 1, 1 << 40))
        f.write(bytes(p))
        for scan, pose, adj in frames:
            f.write(struct.pack("<Ii", len(scan), int(adj is not None)))
            f.write(np.asarray(pose, np.float64).T.tobytes())
            f.write(np.asarray(np.eye(4) if adj is None else adj, np.float64).T.tobytes())
            f.write(scan.tobytes())
    out = subprocess.check_output([exe, "run", fin, fin + ".out", str(reps)]).decode()
    os.remove(fin), os.remove(fin + ".out")
    return float(out.split()[1])


def report(txt, stats_csv):
    import csv

    lines = open(txt).read().strip().split("\n")
    n = int(lines[0].split()[2])
    kept = int(lines[-1].split()[-2])
    n_pts, chunks = 64 * n, 64 * (n // abi.SCAN_CHUNK + 1)
    moved = {"k_scan_flag": (16 * n_pts + 32 * chunks, "16 B read per point (word 0), 32 B of ballots written per chunk"),
             "k_scan_minmax": (16 * kept + 36 * chunks, "ballots and base per chunk, 16 B read per kept point (word 2)"),
             "k_scan_write": (96 * kept + 36 * chunks, "ballots and base per chunk, 48 B read and 48 B written per kept point")}
    out = ["# tools/gpu_mapper.py --cpu on one MI355X (wall time per call, median of 20 after 3 warm-ups; the C calls themselves, arrays marshalled once)", ""] + lines
    out += ["", "# rocprofv3 --kernel-trace --stats -- python tools/gpu_mapper.py --calls 10: mulls_mapper_add, 64 device-resident frames of %d points per call" % n,
            "# (%d points in, %d records out: calibration 0.195 degrees first, dist 2 - 80 m, ratio 5, time ratio from stamps, 63 frames compensated)" % (n_pts, kept),
            "%-24s %6s %12s %8s   %s" % ("kernel", "calls", "average us", "percent", "bytes moved per launch by the pass's definition, and the rate that would be if memory set the time")]
    for r in list(csv.reader(open(stats_csv)))[1:]:
        name, avg = r[0].replace("(anonymous namespace)::", "").split("(")[0], float(r[3]) / 1e3
        extra = "%.1f MB (%s): %.0f GB/s" % (moved[name][0] / 1e6, moved[name][1], moved[name][0] / 1e9 / (avg * 1e-6)) if name in moved else ""
        out.append("%-24s %6s %12.1f %8.2f   %s" % (name, r[1], avg, float(r[4]), extra))
    path = os.path.join(ROOT, "profiles", "mapper_kernel_stats.txt")
    open(path, "w").write("\n".join(out) + "\n")
    print(path)


def main():
    if "--report" in sys.argv:
        k = sys.argv.index("--report")
        return report(sys.argv[k + 1], sys.argv[k + 2])
    scene = synth.Scene(3)
    s = synth.raycast(scene, synth.se3(0, 0, scene.sensor_height), 64, 1900, seed=3)
    scan = abi.records(abi.make_points(s["xyz"], np.zeros_like(s["xyz"]), s["intensity"], s["t"] * 100.0)).copy()
    n = len(scan)
    ctx = lib.Context(0)
    loop = abi.scan_prep_params(calib_on=1, dist_filter_on=1, calib_first=0, vertical_ang_correction_deg=0.195, min_dist=1.0, max_dist=120.0)
    export = abi.scan_prep_params(calib_on=1, dist_filter_on=1, calib_first=1, downsample_ratio=5, timestamp_mode=1, vertical_ang_correction_deg=0.195, min_dist=2.0, max_dist=80.0)
    poses = [synth.se3(0.9 * k, 0.05 * k, 0.0, 0.0, 0.0, 0.01 * k) for k in range(64)]
    host = [(scan, poses[k], np.linalg.inv(poses[k]) @ poses[k - 1] if k else None) for k in range(64)]
    dev = DevBuf(scan)
    resident = [(dev.cloud(), pose, adj) for _, pose, adj in host]
    m = ctx.mapper(64 * (n // 5 + 1))

    def marshalled(frames):
        """the C arrays made once: the whole batch, and one array per frame"""
        return lib.Mapper.marshal(frames), [lib.Mapper.marshal([fr]) for fr in frames]

    def add(arr, B):
        rc = ctx.lib.mulls_mapper_add(ctx.h, m.h, arr, B, C.byref(export), None, None)
        assert rc == 0, rc

    def batch(M, B):
        m.clear()
        add(M[0][0], B)

    def singles(M, B):
        m.clear()
        for arr, _ in M[1][:B]:
            add(arr, 1)

    if "--calls" in sys.argv:
        M = marshalled(resident)
        for _ in range(int(sys.argv[sys.argv.index("--calls") + 1])):
            batch(M, 64)
        print("%d calls of mulls_mapper_add, 64 device-resident frames of %d points -> %d records" % (int(sys.argv[sys.argv.index("--calls") + 1]), n, m.cloud().n))
        return
    print("one scan: %d points; MULLS_SCAN_CHUNK %d" % (n, abi.SCAN_CHUNK))
    work = scan.copy()
    for name, p in (("frame loop (dist 1 - 120 m, calibration 0.195)", loop), ("export (calibration, dist 2 - 80 m, ratio 5, stamps)", export)):
        n_out = C.c_uint32(0)
        t_host = median_ms(lambda: ctx.lib.mulls_scan_prepare(ctx.h, C.c_void_p(work.ctypes.data), n, 48, C.byref(p), C.byref(n_out), None), before=lambda: np.copyto(work, scan))
        t_dev = median_ms(lambda: ctx.lib.mulls_scan_prepare(ctx.h, dev.p, n, 48, C.byref(p), C.byref(n_out), None), before=dev.upload)
        print("mulls_scan_prepare, %s: %d -> %d points; host round trip %.3f ms, in place %.3f ms" % (name, n, n_out.value, t_host, t_dev))
    dev.upload()
    for label, frames in (("host scans", host), ("device-resident scans", resident)):
        M = marshalled(frames)
        for B in (1, 8, 64):
            t_batch = median_ms(lambda: batch(M, B))
            t_single = median_ms(lambda: singles(M, B))
            line = "mulls_mapper_add, %s, %2d frames: one call %.3f ms = %.3f ms per frame; %d single-frame calls %.3f ms = %.3f ms per frame (ratio %.3f)" % (
                label, B, t_batch, t_batch / B, B, t_single, t_single / B, t_batch / t_single)
            if "--cpu" in sys.argv and label == "host scans":
                t_cpu = harness_ms(host[:B], export, 3)
                line += "; CPU harness, one thread %.1f ms = %.2f ms per frame" % (t_cpu, t_cpu / B)
            print(line)
    print("map of 64 frames: %d records" % m.cloud().n)
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
