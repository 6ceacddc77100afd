"""Inputs that put the device-resident local map (mulls_map_*: map.cpp, map_kernels.hip) on the sizes at which its kernels change behaviour
-- the 4096-record segments of the stable compaction and the 64-segment trips of their scan, the 2048-point chunks and 1024-point tiles of the
nearest-tree-point search, the sorted neighbour lists of the PCA refresh, the grid-stride loop of the bounds -- and numpy restatements of the
quantities that decide whether such an edge is crossed.  tests/test_map_edges.py asserts the edges on any machine and pins the oracle to plain
numpy statements of the same operations; tests/test_gpu_map_edges.py runs the same inputs on the device.  Every input is made once per process
and never modified.  No GPU here, and nothing of the reference lines."""
import functools

import numpy as np

from mulls_amd import abi, synth

# the sizes the inputs aim at (map_kernels.hip, map.cpp)
MAP_SEG = 4096  # records per workgroup of k_map_seg_count / k_map_seg_scatter
MAP_SCAN_TRIP = 64  # segments per trip of k_map_seg_scan
MAP_NN_CHUNK = 2048  # tree points per job of k_mapb_nn
MAP_NN_TILE = 1024  # tree points per LDS tile
MAP_PCA_K = 24  # list slots per lane of k_mapb_pca
MAP_BBOX_SPAN = 64 * 256  # records of a class cloud beyond which the bounds take many 2048-record tiles of k_mapb_bbox (eight)
PCA_RADIUS = np.float32(1.8)
PCA_MAX_K = 20
PCA_MIN_K = 6
REMOVAL_MIN_FRAME = 10  # a frame class cloud with this many points or fewer is not searched

CLASSES = range(6)


def records(xyz, seed):
    """POINT_DTYPE records around coordinates with random unit normals, intensities and curvatures, so that a swapped record shows."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    nrm = rng.normal(0.0, 1.0, (len(xyz), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True) + 1e-30
    return abi.make_points(xyz, nrm, rng.uniform(0.0, 255.0, len(xyz)), rng.uniform(0.0, 1.0, len(xyz)))


def empty():
    return np.zeros(0, abi.POINT_DTYPE)


def xyz_of(cloud):
    return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(np.float32)


def moved(xyz, T):
    """pcl::transformPointCloud on coordinates: double arithmetic, float store"""
    x, y, z = (np.asarray(xyz, np.float32)[:, k].astype(np.float64) for k in range(3))
    T = np.asarray(T, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):  # the sums left to right, as the reference writes them
        return np.stack([T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3] for r in range(3)], 1).astype(np.float32)


def turned(nrm, T):
    """... and on normals: the rotation alone"""
    x, y, z = (np.asarray(nrm, np.float32)[:, k].astype(np.float64) for k in range(3))
    T = np.asarray(T, np.float64)
    return np.stack([T[r, 0] * x + T[r, 1] * y + T[r, 2] * z for r in range(3)], 1).astype(np.float32)


def moved_records(cloud, T):
    """a whole cloud through transform_feature: positions and normals move, everything else stays"""
    out = abi.as_points(cloud).copy()
    p, n = moved(xyz_of(out), T), turned(np.stack([out["nx"], out["ny"], out["nz"]], 1), T)
    out["x"], out["y"], out["z"], out["nx"], out["ny"], out["nz"] = p[:, 0], p[:, 1], p[:, 2], n[:, 0], n[:, 1], n[:, 2]
    return out


def segments(n):
    return (n + MAP_SEG - 1) // MAP_SEG


def scan_trips(n):
    return (segments(n) + MAP_SCAN_TRIP - 1) // MAP_SCAN_TRIP


class Case:
    """One map and the frames folded into it: frames[k] = (six clouds, pose), params[k] the update's parameters."""

    def __init__(self, name, map_clouds, map_pose, frames, params, **notes):
        self.name, self.map_clouds, self.map_pose, self.frames, self.params = name, map_clouds, map_pose, frames, params
        self.__dict__.update(notes)

    def sequence(self):
        """in the form test_gpu_map.drive takes: [(map clouds, map pose), (frame clouds, frame pose), ...]"""
        return [(self.map_clouds, self.map_pose)] + list(self.frames)


# ------------------------------------------------------------------------------------------------------------------------------ S: segments
S_SIZES = [266245, 4097, 8192, 4095, 4096, 12305]  # ground: 65 segments + 5 points (two trips of the scan); the others straddle one and two segments
S_FRAME = 300
S_PATTERNS = ("all", "none", "alternate", "last", "first", "half")
S_POSES = [np.eye(4), synth.se3(0.21, -0.13, 0.02, 0.002, -0.001, np.deg2rad(0.7)), synth.se3(0.45, -0.2, 0.03, 0.001, 0.002, np.deg2rad(1.1))]


def keep_pattern(n, rng):
    """which records of a cloud lie inside the filter radius: chosen per 4096-record segment, cycling over S_PATTERNS"""
    keep = np.zeros(n, bool)
    for s in range(segments(n)):
        lo, hi = s * MAP_SEG, min(n, (s + 1) * MAP_SEG)
        p = S_PATTERNS[s % len(S_PATTERNS)]
        if p == "all":
            keep[lo:hi] = True
        elif p == "alternate":
            keep[lo:hi:2] = True
        elif p == "last":
            keep[hi - 1] = True
        elif p == "first":
            keep[lo] = True
        elif p == "half":
            keep[lo:hi] = rng.random(hi - lo) < 0.5
    return keep


def ring_xyz(keep, rng):
    """kept records 10 m or 30 m from the origin in xy (a second filter at 20 m splits them again), dropped ones 70 m, at a random angle"""
    n = len(keep)
    r = np.where(keep, rng.choice([10.0, 30.0], n), 70.0)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    return np.column_stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(-2.0, 5.0, n)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def s_map():
    rng = np.random.default_rng(9100)
    keeps = [keep_pattern(n, rng) for n in S_SIZES]
    return [records(ring_xyz(k, rng), 9110 + c) for c, k in enumerate(keeps)], keeps


@functools.lru_cache(maxsize=None)
def s_frames():
    out = []
    for k in (1, 2):
        rng = np.random.default_rng(9200 + k)
        out.append(([records(ring_xyz(rng.random(S_FRAME) < 0.6, rng), 9210 + 10 * k + c) for c in CLASSES], S_POSES[k]))
    return out


def inside(xyz, radius):
    """CFilter::dist_filter, keep_inside: float products and sum, widened, strict compare against the double radius squared, z finite"""
    x, y, z = (np.asarray(xyz, np.float32)[:, k] for k in range(3))
    d = (x * x + y * y).astype(np.float64)
    r = float(np.float32(radius))
    with np.errstate(invalid="ignore"):
        return (d < r * r) & (z < np.finfo(np.float64).max) & (z > -np.finfo(np.float64).max)


@functools.lru_cache(maxsize=None)
def scene_s(variant):
    m, _ = s_map()
    f = s_frames()
    if variant == "a":  # the radius filter alone, twice (the second radius splits the survivors of the first again)
        P = [abi.map_params(max_num_pts=10**7, kept_vertex_num=10**7, local_map_radius=50.0),
             abi.map_params(max_num_pts=10**7, kept_vertex_num=10**7, local_map_radius=20.0)]
        return Case("S(a)", m, S_POSES[0], f, P)
    if variant == "b":  # everything survives the radius; the thinning masks run over more than 64 segments of ground, twice
        P = [abi.map_params(max_num_pts=150000, kept_vertex_num=5000, local_map_radius=200.0, rng_seed=31),
             abi.map_params(max_num_pts=100000, kept_vertex_num=4097, local_map_radius=200.0, rng_seed=32)]
        return Case("S(b)", m, S_POSES[0], f, P)
    if variant == "c":
        return Case("S(c)", m, S_POSES[0], f[:1], [abi.map_params(max_num_pts=60000, kept_vertex_num=800, local_map_radius=50.0, rng_seed=33)])
    raise KeyError(variant)


# thresholds of the removal cases: squares exact in float, so that a query can sit exactly ON one
NEAR, DMIN, DMAX, CENTER = 0.25, 0.75, 1.25, 25.0


@functools.lru_cache(maxsize=None)
def scene_s_removal():
    """S(d): mask mode on frame clouds of three and two segments (pillar 8193, facade 4097: the facade's slot in the shared verdict array starts
    beyond 4096), the trees being the multi-segment map clouds.  Queries are tree points plus an offset of 0 / 0.1 / 0.5 / 2 m."""
    m, _ = s_map()
    T = np.linalg.inv(S_POSES[1]) @ S_POSES[0]  # tran_target_map: a map-frame point x appears in the frame at T x
    rng = np.random.default_rng(9300)
    fc = list(s_frames()[0][0])
    for c, n in ((abi.PILLAR, 8193), (abi.BEAM, S_FRAME), (abi.FACADE, 4097)):
        base = xyz_of(m[c])[rng.integers(0, len(m[c]), n)].astype(np.float64)
        step = rng.normal(0.0, 1.0, (n, 3))
        step *= (rng.choice([0.0, 0.1, 0.5, 2.0], n) / np.linalg.norm(step, axis=1))[:, None]
        fc[c] = records(moved(base + step, T), 9310 + c)
    P = abi.map_params(max_num_pts=10**6, kept_vertex_num=10**7, local_map_radius=50.0, map_based_dynamic_removal_on=1, dynamic_removal_center_radius=30.0,
                       dynamic_dist_thre_min=0.3, dynamic_dist_thre_max=1.0, near_dist_thre=0.03, tree_mode=1, tree_used="011100")
    return Case("S(d)", m, S_POSES[0], [(fc, S_POSES[1])], [P])


# ------------------------------------------------------------------------------------------------------------------- P: neighbour lists
P_CROSS = np.array([[0.25, 0.0], [-0.25, 0.0], [0.0, 0.25]])  # a pillar's cross-section (from the third point the other two are equally far)
P_HEIGHTS = (24, 20, 19, 16)  # levels per pillar, 0.25 m apart: 15 levels (45 points) lie within 1.8 m of a point in the middle
P_EXTRAS = 7 + 25 + (3 + 4 + 5 + 6 + 7) + 9
P_SIZES = (255, 256, 257, 513)


def _centres():
    """integer-metre centres 4 m apart (no two structures are within 1.8 m of each other), the origin first"""
    g = [(4 * i, 4 * j) for i in range(-7, 8) for j in range(-7, 8)]
    g.sort(key=lambda c: (c[0] ** 2 + c[1] ** 2, c))
    return g


def pillar_layout(n, seed):
    """Scene P's pillar cloud of exactly n points, unpermuted: pillars, then seven exact duplicates, 25 coincident points, isolated vertical
    runs of 3..7 points, and a vertical run of eight points with a ninth exactly 1.8f away from its lowest along x (d == radius^2: excluded)."""
    rng = np.random.default_rng(seed)
    cen = _centres()
    pts = []
    x18 = float(PCA_RADIUS)
    for lev in range(8):  # at the origin: 0 + 1.8f is exact
        pts.append((0.0, 0.0, 0.25 * lev))
    pts.append((x18, 0.0, 0.0))
    ci = 1
    for run in (3, 4, 5, 6, 7):
        cx, cy = cen[ci]
        ci += 1
        pts += [(cx, cy, 0.25 * lev) for lev in range(run)]
    cx, cy = cen[ci]
    ci += 1
    pts += [(cx + 0.25, cy - 0.5, 1.75)] * 25
    n_pillar = n - P_EXTRAS
    assert n_pillar >= 60
    pil = []
    k = 0
    while len(pil) < n_pillar:
        cx, cy = cen[ci]
        ci += 1
        for lev in range(P_HEIGHTS[k % len(P_HEIGHTS)]):
            for ox, oy in P_CROSS:
                pil.append((cx + ox, cy + oy, 0.25 * lev))
        k += 1
    pil = pil[:n_pillar]
    dup = [pil[i] for i in rng.choice(n_pillar, 7, replace=False)]
    xyz = np.array(pil + dup + pts, np.float32)
    assert len(xyz) == n
    return xyz


def reorder(xyz, order, seed):
    """random, or by distance from the first point ascending / descending (stable)"""
    if order == "random":
        return xyz[np.random.default_rng(seed).permutation(len(xyz))]
    d = ((xyz.astype(np.float64) - xyz[0]) ** 2).sum(1)
    idx = np.argsort(d, kind="stable")
    return xyz[idx if order == "ascending" else idx[::-1]]


P_ORDERS = ("random", "ascending", "descending")


@functools.lru_cache(maxsize=None)
def scene_p_xyz(n, order, jitter=False):
    xyz = reorder(pillar_layout(n, 9400 + n), order, 9500 + n)
    if jitter:  # the control: no two distances equal
        xyz = (xyz + np.random.default_rng(9600 + n).uniform(-0.02, 0.02, xyz.shape)).astype(np.float32)
    return xyz


@functools.lru_cache(maxsize=None)
def scene_p(n, order, jitter=False):
    """Pillars as laid out above and beams as the same cloud with x and z swapped; the last twelve records of each arrive with the frame.
    Identity poses: every coordinate reaches the refresh as it is written here."""
    xyz = scene_p_xyz(n, order, jitter)
    pil, beam = records(xyz, 9700 + n), records(xyz[:, ::-1], 9800 + n)
    other = lambda s: records(np.random.default_rng(s).uniform(-20.0, 20.0, (40, 3)), s)
    m = [other(1), pil[:-12], other(2), beam[:-12], other(3), other(4)]
    f = [other(5), pil[-12:], other(6), beam[-12:], other(7), other(8)]
    P = abi.map_params(max_num_pts=10**7, kept_vertex_num=10**7, local_map_radius=60.0, recalculate_feature_on=1)
    return Case("P(%d,%s%s)" % (n, order, ",jitter" if jitter else ""), m, np.eye(4), [(f, np.eye(4))], [P], pillar_xyz=xyz, beam_xyz=xyz[:, ::-1])


@functools.lru_cache(maxsize=None)
def scene_s_pca():
    """S(e): the refresh's own compaction across a segment edge: 4600 pillar points laid out as in scene P, moved by a small rigid motion"""
    xyz = reorder(pillar_layout(4600, 9900), "random", 9901)
    other = lambda s: records(np.random.default_rng(s).uniform(-20.0, 20.0, (S_FRAME, 3)), s)
    m = [other(11), records(xyz, 9902), other(12), records(xyz[:700, ::-1], 9903), other(13), other(14)]
    f = [other(15), other(16)[:20], other(17), other(18)[:20], other(19), other(20)]
    P = abi.map_params(max_num_pts=10**7, kept_vertex_num=10**7, local_map_radius=60.0, recalculate_feature_on=1)
    return Case("S(e)", m, S_POSES[0], [(f, S_POSES[1])], [P])


def pair_d2(q, t):
    """FLANN L2_Simple<float> between every q and every t: ((dx*dx) + dy*dy) + dz*dz in float"""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (q[:, None, k] - t[None, :, k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


def neighbour_lists(xyz, radius=PCA_RADIUS, max_k=PCA_MAX_K):
    """The refresh's lists in numpy: for every point the candidates strictly inside radius^2 in (distance, index) order, cut at max_k.
    Returns dict(in_radius, m, idx (list of index arrays), tie_at_k, on_radius)."""
    xyz = np.asarray(xyz, np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    d2 = pair_d2(xyz, xyz)
    inr = d2 < r2
    count = inr.sum(1)
    idx, tie = [], np.zeros(len(xyz), bool)
    for i in range(len(xyz)):
        cand = np.nonzero(inr[i])[0]
        cand = cand[np.lexsort((cand, d2[i, cand]))]
        if len(cand) > max_k:
            tie[i] = d2[i, cand[max_k - 1]] == d2[i, cand[max_k]]
        idx.append(cand[:max_k])
    return dict(in_radius=count, m=np.minimum(count, max_k), idx=idx, tie_at_k=tie, on_radius=(d2 == r2).sum(1))


# ------------------------------------------------------------------------------------------------------------ N: nearest tree point
N_TREES = (1, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 6145)
N_FRAMES = (10, 11, 255, 256, 257, 1001)
N_BOX = [-16.0, -16.0, -0.5, 16.0, 16.0, 40.0]  # tree points with |x| or |y| >= 16 are outside (16 itself: the rule is strict)
N_BOX_NOWHERE = [100.0, 100.0, 100.0, 101.0, 101.0, 101.0]
# (tree sizes, frame sizes) for pillar, beam, facade -- the order the removal visits them in --, tree_mode, tree_used, box
N_COMBOS = (
    ((1, 1023, 1024), (11, 257, 1001), 1, "011100", N_BOX),
    ((1025, 2047, 2048), (255, 256, 10), 1, "011100", N_BOX),  # the facade is not searched: its cloud and the slot behind the beams' stay as they are
    ((2049, 4096, 4097), (1001, 11, 257), 2, "011100", N_BOX),
    ((6145, 4097, 2049), (257, 1001, 11), 2, "011100", N_BOX),
    ((6145, 1, 4096), (256, 255, 1001), 1, "010100", N_BOX),  # a hole: pillar and beam searched, the facade between them in class order not
    ((4097, 6145, 2048), (11, 10, 257), 2, "011100", N_BOX_NOWHERE),  # no tree point inside the box: every cloud is left alone
    ((2048, 1024, 6145), (1001, 257, 11), 1, "011100", N_BOX),
    ((1, 1025, 2047), (257, 11, 255), 2, "011100", N_BOX),  # the pillars' only tree point may lie outside the box
    ((4096, 2049, 1023), (10, 1001, 256), 2, "011100", N_BOX),
    ((1023, 6145, 1025), (255, 11, 1001), 1, "001100", N_BOX),
)
N_ORDER = (abi.PILLAR, abi.BEAM, abi.FACADE)
# offsets on the 0.25 m lattice: squared lengths 0, near^2, between, dmin^2 (two ways), between, dmax^2, just above, well above
N_OFFSETS = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0], [0.75, 0, 0], [0.5, 0.5, 0.25], [1.0, 0, 0], [0.75, 0.75, 0.25], [1.25, 0, 0],
                      [1.25, 0.25, 0], [1.0, 1.0, 0.5], [0.25, 0.25, 0], [0.25, 0.25, 0.25]])


def tree_xyz(n, seed):
    """n distinct points of a 2 m lattice (x, y in -20..18, z in 0..30; a quarter of them outside N_BOX, corners outside the centre radius) in random
    order.  From 4097 points on, a decoy in chunk 0 sits a hair farther from one query than that query's nearest point in chunk 2, and the other way round."""
    rng = np.random.default_rng(seed)
    lat = np.array([(2 * i, 2 * j, 2 * k) for i in range(-10, 10) for j in range(-10, 10) for k in range(16)], np.float64)
    if n == 1:
        return lat[rng.integers(0, len(lat), 1)].astype(np.float32)
    t = lat[rng.permutation(len(lat))[:n]]
    if n > 2 * MAP_NN_CHUNK:
        t[7] = t[n - 3] + [1.0, 1.0, 0.25]  # the query t[n-3] + (0.5, 0.5, 0) is 0.5 from t[n-3] (chunk 2) and 0.5625 = dmin^2 from t[7] (chunk 0)
        t[n - 2] = t[9] + [1.0, 1.0, 0.25]  # and the mirror image: nearest in chunk 0, decoy in chunk 2
    return t.astype(np.float32)


def query_xyz(tree, nq, seed):
    """nq queries = a tree point + a lattice offset (random sign and axis order).  The first ones are fixed: the last record of the tree hit exactly
    and at 0.5 m, the decoy pairs, a tree point outside N_BOX hit exactly."""
    rng = np.random.default_rng(seed)
    n = len(tree)
    t = tree.astype(np.float64)
    fixed = [t[n - 1], t[n - 1] + [0.0, 0.5, 0.0]]
    if n > 2 * MAP_NN_CHUNK:
        fixed += [t[n - 3] + [0.5, 0.5, 0.0], t[9] + [0.5, 0.5, 0.0]]
    out = np.nonzero((np.abs(t[:, 0]) >= 16.0) | (np.abs(t[:, 1]) >= 16.0))[0]
    if len(out):
        fixed += [t[out[0]], t[out[-1]] + [0.0, 0.0, 0.25]]
    base = t[rng.integers(0, n, nq)]
    off = N_OFFSETS[rng.integers(0, len(N_OFFSETS), nq)] * rng.choice([-1.0, 1.0], (nq, 3))
    off = np.take_along_axis(off, np.argsort(rng.random((nq, 3)), axis=1), axis=1)
    q = base + off
    k = min(len(fixed), nq)
    q[:k] = np.array(fixed)[:k]
    return q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene_n(i):
    """One update per combination, identity poses (queries meet the trees as written).  A 2000-point ground cloud carries the map over the
    removal's size condition; max_num_pts is four times the map, so that nothing is thinned."""
    trees, frames, mode, used, box = N_COMBOS[i]
    g = np.random.default_rng(9050 + i)
    other = lambda n, s: records(g.uniform(-20.0, 20.0, (n, 3)), s)
    m, f = [other(2000, 1), None, None, None, other(50, 2), other(50, 3)], [other(100, 4), None, None, None, other(20, 5), other(20, 6)]
    for k, c in enumerate(N_ORDER):
        t = tree_xyz(trees[k], 9000 + 100 * i + k)
        m[c] = records(t, 9001 + 100 * i + k)
        f[c] = records(query_xyz(t, frames[k], 9002 + 100 * i + k), 9003 + 100 * i + k)
    fpn0 = sum(len(m[c]) for c in range(5))
    P = abi.map_params(max_num_pts=4 * fpn0, kept_vertex_num=10**7, local_map_radius=80.0, map_based_dynamic_removal_on=1, dynamic_removal_center_radius=CENTER,
                       dynamic_dist_thre_min=DMIN, dynamic_dist_thre_max=DMAX, near_dist_thre=NEAR, tree_mode=mode, tree_used=used, tree_box=box)
    return Case("N(%d)" % i, m, np.eye(4), [(f, np.eye(4))], [P])


def in_box(xyz, box):
    """CFilter::bbx_filter: strict on all six sides, float coordinate against double bound"""
    x, y, z = (np.asarray(xyz, np.float32)[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore"):
        return (x > box[0]) & (x < box[3]) & (y > box[1]) & (y < box[4]) & (z > box[2]) & (z < box[5])


def removal_verdict(frame_xyz, tree, P, block=512):
    """map_scan_feature_pts_distance_removal in numpy for one class: (keep[q], searched[q], d2[q], argmin[q]).  `tree` is what the search indexes
    (after the box).  Not searched at all (10 points or fewer, or an empty tree): everything kept."""
    q = np.asarray(frame_xyz, np.float32)
    n = len(q)
    keep, d2, arg = np.ones(n, bool), np.full(n, np.finfo(np.float32).max, np.float32), np.full(n, -1)
    if n <= REMOVAL_MIN_FRAME or len(tree) == 0:
        return keep, np.zeros(n, bool), d2, arg
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        searched = ~(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] > f(P.dynamic_removal_center_radius) * f(P.dynamic_removal_center_radius))
    for lo in range(0, n, block):
        d = pair_d2(q[lo:lo + block], tree)
        d = np.where(d < np.finfo(np.float32).max, d, np.finfo(np.float32).max)  # NaN and overflow never win the minimum
        d2[lo:lo + block], arg[lo:lo + block] = d.min(1), d.argmin(1)
    dmax = f(max(float(f(P.dynamic_dist_thre_max)), float(f(P.dynamic_dist_thre_min)) + 0.1))
    near2, dmin2, dmax2 = f(P.near_dist_thre) * f(P.near_dist_thre), f(P.dynamic_dist_thre_min) * f(P.dynamic_dist_thre_min), dmax * dmax
    rule = ((d2 > near2) & (d2 < dmin2)) | (d2 > dmax2)
    keep = np.where(searched, rule, True)
    return keep, searched, d2, arg


# --------------------------------------------------------------------------------------------------------------- B: bounds and empties
def _b_other(n, s, at=0.0):
    xyz = np.random.default_rng(s).uniform(-3.0, 3.0, (n, 3))
    xyz[:, 0] += at
    return records(xyz, s)


@functools.lru_cache(maxsize=None)
def scene_b(name):
    none = [empty() for _ in CLASSES]
    wide = dict(max_num_pts=10**7, kept_vertex_num=10**7)
    if name == "filtered_away":  # clouds 100 m out, a 5 m map: nothing is left and no bound has a key
        m = [_b_other(60, 9601 + c, at=100.0) for c in CLASSES]
        f = [_b_other(30, 9611 + c, at=-100.0) for c in CLASSES]
        return Case("B(filtered_away)", m, S_POSES[0], [(f, S_POSES[1])], [abi.map_params(local_map_radius=5.0, **wide)])
    if name == "empty":
        return Case("B(empty)", none, S_POSES[0], [(none, S_POSES[1])], [abi.map_params(**wide)])
    if name == "single_vertex":  # one point in all: negative coordinates and a negative zero
        f = list(none)
        f[abi.VERTEX] = records(np.array([[-3.5, -0.0, -1.25]], np.float32), 9621)
        return Case("B(single_vertex)", none, np.eye(4), [(f, np.eye(4)), (none, S_POSES[1])], [abi.map_params(**wide), abi.map_params(**wide)])
    if name == "far":  # coordinates of 1e6 (the squares fit a float; the posed bounds do not sit on float neighbours of the local ones)
        m = [records(np.random.default_rng(9631 + c).uniform(-1.0, 1.0, (50, 3)) * [1e6, 1e6, 1e3], 9641 + c) for c in CLASSES]
        f = [records(np.random.default_rng(9651 + c).uniform(-1.0, 1.0, (30, 3)) * [1e6, 1e6, 1e3], 9661 + c) for c in CLASSES]
        return Case("B(far)", m, S_POSES[0], [(f, S_POSES[1])], [abi.map_params(local_map_radius=1.2e6, **wide)])
    if name == "bbox_second_trip":  # a class cloud above 64 x 256 points whose extremes sit in its last records
        rng = np.random.default_rng(9671)
        xyz = rng.uniform(-20.0, 20.0, (MAP_BBOX_SPAN + 300, 3))
        xyz[-1], xyz[-2], xyz[-3] = [39.0, 0.5, 0.25], [-38.0, -39.5, 0.0], [1.0, 38.5, 44.0]
        xyz[-4] = [0.0, 0.0, -41.0]
        m = [_b_other(50, 9681 + c) for c in CLASSES]
        m[abi.FACADE] = records(xyz, 9672)
        f = [_b_other(30, 9691 + c) for c in CLASSES]
        return Case("B(bbox_second_trip)", m, S_POSES[0], [(f, S_POSES[1])], [abi.map_params(local_map_radius=60.0, **wide)])
    if name == "nonfinite":
        # NaN, +-inf, +-3e38 and 1e20 in x and y, NaN / +-inf in z, in the frame's and the map's removal classes; identity poses, so that a
        # bad coordinate stays in its own column on the way to the search.  (No huge finite heights: see update_cloud_vectors in the oracle.)
        bad_xy = [np.nan, np.inf, -np.inf, 3e38, -3e38, 1e20]
        bad_z = [np.nan, np.inf, -np.inf]
        m, f = [_b_other(400, 9701 + c) for c in CLASSES], [_b_other(60, 9711 + c) for c in CLASSES]
        for c in N_ORDER:
            for cloud in (m[c], f[c]):  # records 3, 4, 8, 9, ... 29, then 33, 38, 43, and 48 (all three coordinates NaN)
                k = 3
                for v in bad_xy:
                    cloud["x"][k], cloud["y"][k + 1] = v, v
                    k += 5
                for v in bad_z:
                    cloud["z"][k] = v
                    k += 5
                cloud["x"][k], cloud["y"][k], cloud["z"][k] = np.nan, np.nan, np.nan
            good = np.arange(0, 50, 5)  # ten finite map records set apart from the rest; the queries half a metre from them are removed by the rule
            m[c]["x"][good], m[c]["y"][good], m[c]["z"][good] = np.arange(-9.0, 11.0, 2.0), 12.0, 0.0
            f[c]["x"][50:], f[c]["y"][50:], f[c]["z"][50:] = m[c]["x"][good], m[c]["y"][good] + np.float32(0.5), m[c]["z"][good]
        P = abi.map_params(local_map_radius=60.0, map_based_dynamic_removal_on=1, dynamic_removal_center_radius=CENTER, dynamic_dist_thre_min=0.3,
                           dynamic_dist_thre_max=1.0, near_dist_thre=0.03, tree_mode=1, tree_used="011100", max_num_pts=9000, kept_vertex_num=10**7)
        return Case("B(nonfinite)", m, np.eye(4), [(f, np.eye(4))], [P])
    raise KeyError(name)


B_NAMES = ("filtered_away", "empty", "single_vertex", "far", "bbox_second_trip", "nonfinite")


def bounds_of(clouds, pose):
    """get_cloud_bbx over all six clouds and over the same points moved by the pose: +-DBL_MAX where there is no point"""
    big = np.finfo(np.float64).max
    xyz = np.concatenate([xyz_of(c) for c in clouds]) if sum(len(c) for c in clouds) else np.zeros((0, 3), np.float32)
    if not len(xyz):
        return [big] * 3 + [-big] * 3, [big] * 3 + [-big] * 3
    posed = moved(xyz, np.asarray(pose))
    box = lambda p: [float(v) for v in p.min(0)] + [float(v) for v in p.max(0)]
    return box(xyz), box(posed)
