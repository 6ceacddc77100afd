"""The definition of the key-point non-maximum suppression (include/mulls_hip.h: mulls_non_max_suppress) restated in numpy,
independently of the library's code: upstream's walk (cfilter.hpp:1211-1228) as it is written there — take the first unvisited point, keep it, erase what
its radius query returns — over a brute-force radius query with FLANN's arithmetic, d2 = (dx dx + dy dy) + dz dz in float against
r2 = (float)((double)r * (double)r), strict.

    walk(records, order, radius)   the walk over the points in a given visiting order -> the kept points' indices into `records`, in visiting order
    suppress(records, radius)      gate, visiting order, walk -> (kept_idx, order, ran)

suppress sorts with a STABLE descending order.  Upstream's std::sort is not stable, so the two agree only where the keys are distinct: suppress asserts that.
Inputs with ties are the harness's (tests/nms_harness.cpp), which runs the std::sort itself.

PCL is not available where these tests run: the radius test restates pcl::search::KdTree::radiusSearch from memory and was not compared with it."""
import numpy as np

GATE = 10  # cfilter.hpp:1190


def xyz_of(records):
    """(n, 3) float32 coordinates of raw (n, 48) uint8 records, or of a float array whose first three columns are x, y, z"""
    a = np.asarray(records)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a[:, :12]).view(np.float32).reshape(len(a), 3)
    return np.ascontiguousarray(a[:, :3], np.float32)


def keys_of(records):
    """normal[3]: the float at byte 28 of the record"""
    a = np.asarray(records)
    assert a.dtype == np.uint8 and a.shape[1] >= 32
    return np.ascontiguousarray(a[:, 28:32]).view(np.float32).reshape(len(a))


def r2_of(radius):
    r = np.float64(np.float32(radius))
    return np.float32(r * r)


def walk(records, order, radius):
    xyz = xyz_of(records)[np.asarray(order, np.int64)]
    n, r2 = len(xyz), r2_of(radius)
    unvisited = np.ones(n, bool)
    kept = []
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    for i in range(n):
        if not unvisited[i]:
            continue
        kept.append(i)
        unvisited[i] = False
        dx, dy, dz = x - x[i], y - y[i], z - z[i]
        d2 = (dx * dx + dy * dy) + dz * dz  # float32 throughout, one rounding per operation
        unvisited &= ~(d2 < r2)
    return np.asarray(order, np.int32)[np.asarray(kept, np.int64)] if kept else np.zeros(0, np.int32)


def suppress(records, radius):
    n = len(records)
    if n < GATE:
        ident = np.arange(n, dtype=np.int32)
        return ident, ident.copy(), False
    keys = keys_of(records)
    assert not np.isnan(keys).any()
    assert len(np.unique(keys)) == n, "suppress() is valid for distinct keys only: equal keys fall as std::sort leaves them (use the harness)"
    order = np.argsort(-keys.astype(np.float64), kind="stable").astype(np.int32)
    return walk(records, order, radius), order, True


# ---------------------------------------------------------------------------------------------------------------- inputs the tests share
def make_records(xyz, keys, seed=0):
    """48-byte records around coordinates and keys, every other byte random: what comes back must be these bytes"""
    xyz, keys = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(keys, np.float32)
    raw = np.random.default_rng(seed).integers(0, 256, (len(xyz), 48), dtype=np.uint8)
    raw[:, :12] = xyz.view(np.uint8).reshape(len(xyz), 12)
    raw[:, 28:32] = keys.view(np.uint8).reshape(len(xyz), 4)
    return raw


# tie-heavy synthetic clouds of tests/golden/nms_cases.npz: name -> (seed, n, distinct key values, box half width, radius)
TIE_CASES = {"tie2": (21, 300, 2, 0.8, 0.25), "tie8": (22, 1000, 8, 1.2, 0.25), "tie64": (23, 1025, 64, 2.0, 0.4), "tie_all": (24, 257, 1, 0.7, 0.25)}


def tie_cloud(name):
    """(xyz, keys): uniform points in a box, keys quantised to a few values, so that most of the visiting order is std::sort's tie order"""
    seed, n, levels, half, _ = TIE_CASES[name]
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    keys = (np.floor(rng.uniform(0, 1, n) * levels) / np.float32(max(levels, 1))).astype(np.float32)
    return xyz, keys
