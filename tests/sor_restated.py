"""An independent numpy restatement of the statistical outlier removal as include/mulls_hip.h defines it (mulls_sor_filter):
pcl::StatisticalOutlierRemoval's expressions restated from memory of PCL 1.8 - 1.10, and the library's own choices (the double square root, the order of
the statistics' sums).  Nothing here was compared with PCL, which is not available where this project is built and tested.

Two neighbour searches: blocked brute force in float32 with the stated expression order (small clouds), and a kd-tree-assisted one for large clouds
(scipy.spatial.cKDTree proposes mean_k + 1 + 8 candidates in double, which are re-evaluated in float32)."""
import numpy as np

PARTIALS = 16384  # the statistics' strided partial sums (MULLS_SOR_PARTIALS)
MARGIN = 8
BRUTE_MAX = 30000


def d2_f32(q, p):
    """(len(q), len(p)) float32 squared distances, (dx dx + dy dy) + dz dz, every operation rounded to float32"""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def knn_brute(xyz, kk, block=256):
    """the kk smallest squared distances of every point to the cloud (itself included), ascending: (n, kk) float32"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    out = np.empty((len(xyz), kk), np.float32)
    for b in range(0, len(xyz), block):
        d = d2_f32(xyz[b:b + block], xyz)
        out[b:b + block] = np.sort(np.partition(d, kk - 1, axis=1)[:, :kk], axis=1)
    return out


def knn_tree(xyz, kk, workers=-1):
    """the same through a kd-tree: candidates in double, values in float32; asserts that no near-tie reached past the candidates"""
    from scipy.spatial import cKDTree

    xyz = np.ascontiguousarray(xyz, np.float32)
    n = len(xyz)
    k = min(n, kk + MARGIN)
    x64 = xyz.astype(np.float64)
    dd, idx = cKDTree(x64).query(x64, k=k, workers=workers)
    p = xyz[idx]  # (n, k, 3)
    dx, dy, dz = xyz[:, None, 0] - p[:, :, 0], xyz[:, None, 1] - p[:, :, 1], xyz[:, None, 2] - p[:, :, 2]
    d = np.sort((dx * dx + dy * dy) + dz * dz, axis=1)
    if k < n:
        # everything outside the candidates is at least dd[:, -1] away in exact arithmetic; its float32 value cannot fall below that by more than 1e-6
        # relative, so the kk-th float32 value must lie clearly below it for the candidates to hold the answer
        far = dd[:, -1] ** 2 * (1.0 - 1e-6)
        assert (d[:, kk - 1].astype(np.float64) < far).all(), "the margin of %d candidates was exhausted by near-ties" % MARGIN
    return np.ascontiguousarray(d[:, :kk])


def knn(xyz, kk, method="auto"):
    if method == "auto":
        method = "brute" if len(xyz) <= BRUTE_MAX else "tree"
    return knn_brute(xyz, kk) if method == "brute" else knn_tree(xyz, kk)


def mean_dist(d2_sorted, mean_k, float_sqrt=False):
    """dist_i: the smallest value dropped, the square roots of the mean_k behind it summed in double in ascending order, / mean_k, rounded to float32.
    float_sqrt: the other reading of PCL's unqualified sqrt (the float overload), which the library does not define"""
    s = np.zeros(len(d2_sorted), np.float64)
    with np.errstate(invalid="ignore"):
        for j in range(1, mean_k + 1):
            v = d2_sorted[:, j]
            s = s + (np.sqrt(v).astype(np.float64) if float_sqrt else np.sqrt(v.astype(np.float64)))
        return (s / np.float64(mean_k)).astype(np.float32)


def sums(dist):
    """(sum, sq_sum) in the defined order: PARTIALS strided partial sums in ascending index, then the pairwise tree"""
    dist = np.asarray(dist, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        terms = [dist.astype(np.float64), (dist * dist).astype(np.float64)]
        out = []
        for t in terms:
            rows = -(-len(t) // PARTIALS)
            pad = np.zeros(rows * PARTIALS, np.float64)  # (a partial that runs out of terms earlier adds nothing: + 0.0 leaves these non-negative sums alone)
            pad[:len(t)] = t
            pad = pad.reshape(rows, PARTIALS)
            s = np.zeros(PARTIALS, np.float64)
            for r in range(rows):
                s = s + pad[r]
            half = PARTIALS // 2
            while half >= 1:
                s = s[:half] + s[half:2 * half]
                half //= 2
            out.append(np.float64(s[0]))
    return out[0], out[1]


def statistics(dist, std_mul):
    """(mean, stddev, threshold), float64; a variance that rounding made negative gives NaN, as the arithmetic says"""
    n = np.float64(len(dist))
    s, q = sums(dist)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = s / n
        variance = (q - s * s / n) / (n - np.float64(1.0))
        stddev = np.sqrt(variance)
        return mean, stddev, mean + np.float64(std_mul) * stddev


def restate(xyz, mean_k=20, std_mul=2.0, float_sqrt=False, method="auto", d2_sorted=None):
    """the whole filter: dict(dist, mean, stddev, threshold, keep, kept_idx)"""
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    assert len(xyz) > mean_k >= 1
    if d2_sorted is None:
        d2_sorted = knn(xyz, mean_k + 1, method)
    dist = mean_dist(d2_sorted, mean_k, float_sqrt)
    mean, stddev, thr = statistics(dist, std_mul)
    with np.errstate(invalid="ignore"):
        keep = ~(dist.astype(np.float64) > thr)
    return dict(dist=dist, mean=mean, stddev=stddev, threshold=thr, keep=keep, kept_idx=np.flatnonzero(keep).astype(np.int32), d2=d2_sorted)


def gap(r):
    """smallest relative distance of any dist_i to the threshold"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.min(np.abs(r["dist"].astype(np.float64) - r["threshold"]) / abs(r["threshold"])))


# ---------------------------------------------------------------------------------------------------------------- the large cases' inputs
def synth_scan(seed, n_beams, n_az):
    from mulls_amd import synth

    scene = synth.Scene(seed)
    return np.ascontiguousarray(synth.raycast(scene, synth.se3(0, 0, scene.sensor_height), n_beams, n_az, seed=seed)["xyz"], np.float32)


def merged_map(seed, n_poses, n_beams=64, n_az=1900, step=4.0):
    """scans of one scene from poses along its street, moved into the world frame (double, rounded to float32 once) and concatenated"""
    from mulls_amd import synth

    scene = synth.Scene(seed)
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(n_poses):
        pose = synth.se3((k - n_poses / 2) * step, rng.normal(0, 0.2), scene.sensor_height, 0.0, 0.0, rng.normal(0, 0.02))
        xyz = synth.raycast(scene, pose, n_beams, n_az, seed=seed * 1000 + k)["xyz"].astype(np.float64)
        parts.append((xyz @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(parts))


def demo_scan(golden_dir):
    import os

    return np.ascontiguousarray(np.load(os.path.join(golden_dir, "demo_pair.npz"))["scan_0"][:, :3], np.float32)


LARGE_CASES = {
    "scan7": lambda g: synth_scan(7, 32, 900),
    "scan3": lambda g: synth_scan(3, 64, 1900),
    "demo0": demo_scan,
    "map8": lambda g: merged_map(11, 8),
}
KEEPS_DIST = "scan7"  # the case whose mean_dist array the fixture stores in full
