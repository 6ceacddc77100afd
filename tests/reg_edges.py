"""The scenes of the size and table-edge tests of NDT and GICP (tests/test_reg_edges.py, tests/test_gpu_reg_edges.py) and of the fixtures
tests/golden/ndt_edges.npz and tests/golden/gicp_edges.npz: the parts of k_ndt.hip and k_gicp.hip that only matter at size or at the end of a range —
more source points than the MULLS_NDT_TREE = 4096 lanes of the strided partials, hash tables whose probe sequences run long and wrap past the last
slot, cells fuller than the one-lane sort's first gap, coordinates at the ends of the voxel key's range, an NDT grid of almost INT32_MAX cells, the
register lists at k = 3, 8, 9 and 21.  Every case is named for the edge it reaches; tests/test_reg_edges.py asserts that it does.

build(solver) -> clouds, cases.  clouds: name -> (n, 3) float32, each stored once in the fixture.  A case: dict(tgt, src: (cloud name, first, last),
tgt_bound, src_bound (6,), guess (4, 4), prm: overrides of the default parameters).  resolve(clouds, case) cuts the slices."""
import json

import numpy as np

import gicp_restated as gr
import gicp_scenes
from ndt_scenes import bound_of, street

WIDE_NS = (4095, 4096, 4097, 8193)
KS = (3, 8, 9, 21)


# ---- the hash tables, restated (open addressing, linear probing, a power of two of slots)

def table_log2(n):
    """log2 of the slots of a table for a cloud of n points before the crop: a power of two >= max(2 n, 1024) (both solvers)"""
    return gr.table_log2(n)


def ndt_home(key, lg):
    """k_ndt.hip's hash_slot: ((uint32)key * 2654435761) >> (32 - lg)"""
    return ((int(key) * 2654435761) & 0xFFFFFFFF) >> (32 - lg)


def occupied(homes, slots):
    """the slots that hold a key after keys with these home slots were inserted.  Under linear probing the set does not depend on the order of insertion
    (only which key sits where does), so whatever order the device's atomics arrived in, these are the slots it filled."""
    occ = np.zeros(slots, bool)
    for h in homes:
        h = int(h)
        while occ[h]:
            h = (h + 1) & (slots - 1)
        occ[h] = True
    return occ


def run_of(occ, slot):
    """(first, last) of the maximal stretch of occupied slots around `slot` that does not cross the table's end; None when the slot is empty"""
    if not occ[slot]:
        return None
    a = b = int(slot)
    while a > 0 and occ[a - 1]:
        a -= 1
    while b < len(occ) - 1 and occ[b + 1]:
        b += 1
    return a, b


def longest_run(occ):
    best, a = (0, 0), None
    for s in range(len(occ) + 1):
        if s < len(occ) and occ[s]:
            a = s if a is None else a
        elif a is not None:
            best, a = max(best, (s - a, a)), None
    return best[1], best[0]  # first, length


def wrap_of(homes, occ):
    """a: the first slot of the maximal occupied stretch that ends at the last slot (None when the last slot is empty); the number of keys whose home
    lies in [a, slots); slots - a.  More keys than slots: some key's probe sequence went past the last slot to slot 0, in every order of insertion."""
    slots = len(occ)
    r = run_of(occ, slots - 1)
    if r is None:
        return None, 0, 0
    return r[0], int((np.asarray(homes) >= r[0]).sum()), slots - r[0]


def miss_walk(home, occ):
    """the slots a lookup of an absent key reads: from its home to the first empty slot, wrapping"""
    out, h = [], int(home)
    while occ[h]:
        out.append(h)
        h = (h + 1) & (len(occ) - 1)
    return out + [h]


def choose_cells(homes, slots, rng, run_keys, wrap_keys, window, n_absent):
    """indices into `homes` (the candidate cells' home slots): `run`, run_keys cells with homes in a window of `window` < run_keys slots in mid-table (they
    fill one stretch of at least run_keys slots); `wrap`, wrap_keys > window cells with homes in the table's last `window` slots (the stretch runs past
    the end); `absent_run`, `absent_wrap`: cells left out of the target whose home lies inside those stretches"""
    out = {}
    for name, first, count in (("run", slots // 3, run_keys), ("wrap", slots - window, wrap_keys)):
        idx = np.flatnonzero((homes >= first) & (homes < first + window))
        idx = idx[np.argsort(homes[idx], kind="stable")]
        assert len(idx) >= count + n_absent, (name, len(idx))
        rest = rng.permutation(idx[1:])
        out[name] = np.concatenate([idx[:1], rest[:count - 1]])  # (the smallest home is taken: every other home then lies inside the stretch)
        out["absent_" + name] = rest[count - 1:count - 1 + n_absent]
    return out


# ---- scenes

def wide():
    """one synthetic street, wide enough for 9 000 target and 8 193 source points"""
    A, B, _ = street(8, 9000, 8500, (0.1, -0.05, -1.0), n_az=(700, 560))
    assert len(A) == 9000 and len(B) >= WIDE_NS[-1]
    return A, np.ascontiguousarray(B[:WIDE_NS[-1]])


def wide_crop_bounds(A, B):
    """bounds that make the crop cut both clouds: the target's block is said to end at x = 14"""
    tb, sb = bound_of(A), bound_of(B)
    tb[3] = 14.0
    return tb, sb


NDT_DENSE = dict(lo=(-20, -24, -3), dims=(48, 48, 8), n_tgt=2000, run_keys=18, wrap_keys=12, window=8, n_absent=3, leaf_points=6)


def ndt_dense():
    """a target of 2 000 points in 1 850 cells of 1 m (4 096 slots: a load of 0.45; 0.5 is the most the table's sizing allows).  30 cells are leaves of
    six points: 18 whose home slots lie in a window of 8 slots in mid-table and 12 whose homes lie in the last 8 slots; every other cell holds one point.
    The source has points in every leaf, and points in cells that are not in the target and whose home slot lies inside those two stretches.
    -> tgt, src, info (the chosen cells, relative to the grid's corner)"""
    P = NDT_DENSE
    rng = np.random.default_rng(41)
    lo, dims = np.array(P["lo"]), P["dims"]
    lg = table_log2(P["n_tgt"])
    slots = 1 << lg
    cells = np.array([(i, j, k) for k in range(dims[2]) for j in range(dims[1]) for i in range(dims[0])])
    keys = cells[:, 0] + cells[:, 1] * dims[0] + cells[:, 2] * dims[0] * dims[1]
    homes = np.array([ndt_home(k, lg) for k in keys])
    pick = choose_cells(homes, slots, rng, P["run_keys"], P["wrap_keys"], P["window"], P["n_absent"])
    leaves = np.concatenate([pick["run"], pick["wrap"]])
    absent = np.concatenate([pick["absent_run"], pick["absent_wrap"]])
    corners = np.array([0, len(cells) - 1])  # the grid's extent
    n_single = P["n_tgt"] - P["leaf_points"] * len(leaves)
    taken = set(leaves) | set(absent) | set(corners)
    guard = slots - P["window"] - 8  # no other cell has its home this near the table's end: the keys that can be pushed past it are the 12 leaves
    rest = np.array([i for i in rng.permutation(len(cells)) if i not in taken and homes[i] < guard])
    assert homes[corners].max() < guard
    singles = np.concatenate([corners, rest[:n_single - len(corners)]])
    inside = lambda idx, n: (lo + cells[np.repeat(idx, n)]) + rng.uniform(0.15, 0.85, (len(idx) * n, 3))
    leaf_pts = inside(leaves, P["leaf_points"])
    tgt = np.concatenate([leaf_pts, inside(singles, 1)])
    tgt = tgt[rng.permutation(len(tgt))].astype(np.float32)
    src = np.concatenate([inside(leaves, 4), lo + cells[np.repeat(absent, 2)] + rng.uniform(0.3, 0.7, (2 * len(absent), 3)), inside(singles[2:62], 1)])
    src = (src[rng.permutation(len(src))] + [0.03, -0.02, 0.02]).astype(np.float32)
    return tgt, src, dict(leaves=cells[leaves], absent_run=cells[pick["absent_run"]], absent_wrap=cells[pick["absent_wrap"]], lg=lg)


GICP_DENSE = dict(lo=(-14, -14, -7), dims=(28, 28, 14), n_tgt=2000, n_cells=1960, run_keys=24, wrap_keys=18, window=12, n_absent=3)


def gicp_dense():
    """a target of 2 000 points in 1 960 cells of 1 m (4 096 slots: a load of 0.48).  Every point lies in the upper half of its cell on every axis, so
    that its voxel (floor(x - 0.5)) and its neighbour cell (floor(x)) have the same coordinates: the voxel table and the target's neighbour table hold
    the same keys.  24 cells have their home slots in a window of 12 slots in mid-table, 18 in the last 12 slots.  Cells that are not in the target
    and whose home lies inside those stretches have an occupied neighbour cell (the ring walk looks them up) and source points in them (the evaluation
    looks them up); the 42 chosen cells have a source point each.  -> tgt, src, info"""
    P = GICP_DENSE
    rng = np.random.default_rng(43)
    lo, dims = np.array(P["lo"]), P["dims"]
    lg = table_log2(P["n_tgt"])
    slots = 1 << lg
    cells = np.array([(i, j, k) for k in range(dims[2]) for j in range(dims[1]) for i in range(dims[0])]) + lo
    homes = np.array([gr.home_slot(gr.pack(c), lg) for c in cells])
    pick = choose_cells(homes, slots, rng, P["run_keys"], P["wrap_keys"], P["window"], P["n_absent"])
    chosen = np.concatenate([pick["run"], pick["wrap"]])
    absent = np.concatenate([pick["absent_run"], pick["absent_wrap"]])
    where = {tuple(c): i for i, c in enumerate(cells)}
    beside = []
    for a in absent:  # an occupied cell next to every absent one
        for step in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)):
            i = where.get(tuple(cells[a] + step))
            if i is not None and i not in absent:
                beside.append(i)
                break
    assert len(beside) == len(absent)
    taken = set(chosen) | set(absent) | set(beside)
    first = np.concatenate([chosen, np.array(sorted(set(beside) - set(chosen)), np.int64)])
    guard = slots - P["window"] - 8  # no other cell has its home this near the table's end: the keys that can be pushed past it are the 18 chosen ones
    rest = np.array([i for i in rng.permutation(len(cells)) if i not in taken and homes[i] < guard])
    assert all(homes[i] < guard for i in set(beside) - set(chosen))
    occupied_cells = np.concatenate([first, rest[:P["n_cells"] - len(first)]])
    twice = rng.choice(occupied_cells, P["n_tgt"] - P["n_cells"], replace=False)
    at = np.concatenate([occupied_cells, twice])
    tgt = cells[at] + rng.uniform(0.55, 0.95, (len(at), 3))
    tgt = tgt[rng.permutation(len(tgt))].astype(np.float32)
    near = tgt[rng.choice(len(tgt), 320, replace=False)].astype(np.float64) + rng.normal(0, 0.03, (320, 3))
    middle = lambda idx, n: cells[np.repeat(idx, n)] + 1.0 + rng.uniform(-0.1, 0.1, (n * len(idx), 3))  # of the voxel [c + 0.5, c + 1.5)
    src = np.concatenate([near, middle(absent, 2), middle(chosen, 1)])
    src = src[rng.permutation(len(src))].astype(np.float32)
    return tgt, src, dict(absent_run=cells[pick["absent_run"]], absent_wrap=cells[pick["absent_wrap"]], lg=lg)


FULL_CELLS = (((6, 3, 4), 1751), ((-8, -4, 4), 1749), ((12, 5, 4), 1750), ((-3, 7, 4), 702))


def full_cell(shift):
    """the 1 500 / 400 street and, three metres above it, four cells of 1 m with 1 751, 1 749, 1 750 and 702 target points (the one-lane shell sort's
    first gaps are 1 750 and 701), the target permuted.  shift = 0: NDT's cells [c, c + 1); shift = 0.5: GICP's voxels [c + 0.5, c + 1.5).  40 source
    points lie in each of the four cells."""
    A, B, _ = street(3, 1500, 400, (0.3, 0.05, 3.0))
    rng = np.random.default_rng(47)
    tgt, src = [A.astype(np.float64)], [B.astype(np.float64)]
    for c, n in FULL_CELLS:
        tgt.append(np.array(c) + shift + rng.uniform(0.01, 0.99, (n, 3)))
        src.append(np.array(c) + shift + rng.uniform(0.05, 0.95, (40, 3)))
    tgt = np.concatenate(tgt)
    return tgt[rng.permutation(len(tgt))].astype(np.float32), np.concatenate(src).astype(np.float32)


GRID_CELLS = 1290  # per axis at 1 m: 1290^3 = 2 146 689 000 cells, 794 647 below INT32_MAX


def grid_almost_full():
    """the 1 500 / 400 street and a leaf of eight target points in the cell 1 289 cells beyond the street's lowest corner on every axis: a grid of
    1 290 cells per axis.  Six source points lie in that leaf; others lie one and two cells beyond it (outside the grid)."""
    A, B, _ = street(3, 1500, 400, (0.3, 0.05, 3.0))
    rng = np.random.default_rng(53)
    corner = np.floor(A.min(axis=0).astype(np.float64)) + (GRID_CELLS - 1)
    leaf = corner + rng.uniform(0.1, 0.9, (8, 3))
    tgt = np.concatenate([A, leaf]).astype(np.float32)
    inside = leaf[:6] + rng.normal(0, 0.03, (6, 3))
    beyond = corner + 0.5 + np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2], [2, 2, 2], [1, 1, 1]])
    src = np.concatenate([B, inside, beyond]).astype(np.float32)
    return tgt, src, corner.astype(np.int64)


LIMIT_LO, LIMIT_HI = -1048575.5, 1048575.875  # the first and the last coordinate a target point may have at 1 m (voxel_coord below, knn_coord above)


def range_edge():
    """two clusters on a 1/8 grid (exact in float32 out to 2^20) in opposite corners of the voxel key's range: 400 points in the 4 m below the highest
    accepted coordinate on every axis, 400 in the 4 m above the lowest, the two extreme points among them.  The source is every other target point,
    those more than half a metre inside moved by one grid step; and one point at -2^20 itself on x: a neighbour cell the source may have (knn_coord
    accepts it) where no voxel can be (voxel_coord refuses it: the point adds nothing)."""
    rng = np.random.default_rng(59)
    span = 32  # 1/8 steps: 4 m
    lo = LIMIT_LO + rng.integers(0, span + 1, (400, 3)) / 8.0
    hi = LIMIT_HI - rng.integers(0, span + 1, (400, 3)) / 8.0
    lo[0], hi[0] = LIMIT_LO, LIMIT_HI
    tgt = np.concatenate([lo, hi])
    src = tgt[::2].copy()
    free = (np.abs(src) < 1048575.0).all(axis=1)
    src[free] += rng.integers(-1, 2, (int(free.sum()), 3)) / 8.0
    src = np.concatenate([src, [[-1048576.0, -1048575.0, -1048575.25]]])
    tgt32, src32 = tgt.astype(np.float32), src.astype(np.float32)
    assert np.array_equal(tgt32.astype(np.float64), tgt) and np.array_equal(src32.astype(np.float64), src)
    order = rng.permutation(len(tgt32))
    return tgt32[order], src32


# ---- the cases

def build(solver):
    assert solver in ("ndt", "gicp")
    clouds, cases = {}, {}
    eye = np.eye(4)

    def add(name, tgt, src, tgt_bound=None, src_bound=None, **prm):
        """tgt, src: a cloud's name, or (name, first, last)"""
        ref = lambda r: (r, 0, len(clouds[r])) if isinstance(r, str) else tuple(r)
        tgt, src = ref(tgt), ref(src)
        cut = lambda r: clouds[r[0]][r[1]:r[2]]
        cases[name] = dict(tgt=tgt, src=src, tgt_bound=bound_of(cut(tgt)) if tgt_bound is None else np.asarray(tgt_bound, np.float64),
                           src_bound=bound_of(cut(src)) if src_bound is None else np.asarray(src_bound, np.float64), guess=eye.copy(), prm=prm)

    off = dict(apply_intersection_filter=0) if solver == "ndt" else {}  # (GICP's default is off)
    on = dict(apply_intersection_filter=1)
    clouds["wide_tgt"], clouds["wide_src"] = wide()
    for n in WIDE_NS:
        add("wide_%d" % n, "wide_tgt", ("wide_src", 0, n), **off)
    tb, sb = wide_crop_bounds(clouds["wide_tgt"], clouds["wide_src"])
    add("wide_8193_crop", "wide_tgt", "wide_src", tgt_bound=tb, src_bound=sb, **on)
    if solver == "ndt":
        add("wide_8193_direct26", "wide_tgt", "wide_src", search_method=1, **off)
        add("wide_8193_direct1", "wide_tgt", "wide_src", search_method=3, **off)
        clouds["dense_tgt"], clouds["dense_src"], _ = ndt_dense()
        clouds["full_tgt"], clouds["full_src"] = full_cell(0.0)
        clouds["grid_tgt"], clouds["grid_src"], _ = grid_almost_full()
    else:
        clouds["dense_tgt"], clouds["dense_src"], _ = gicp_dense()
        clouds["full_tgt"], clouds["full_src"] = full_cell(0.5)
    add("dense_table", "dense_tgt", "dense_src", **off)
    add("full_cell", "full_tgt", "full_src", **off)
    if solver == "ndt":
        add("grid_almost_full", "grid_tgt", "grid_src", **off)
    else:
        clouds["range_tgt"], clouds["range_src"] = range_edge()
        add("range_edge", "range_tgt", "range_src", start_rotvec=[0.0, 0.0, 0.0])
        old, _ = gicp_scenes.build_cases()
        clouds["street_tgt"], clouds["street_src"] = old["street"]["tgt"], old["street"]["src"]
        clouds["outliers_tgt"], clouds["outliers_src"] = old["outliers"]["tgt"], old["outliers"]["src"]
        for k in KS:
            add("k%d" % k, "street_tgt", "street_src", k_correspondences=k)
            add("k%d_outliers" % k, "outliers_tgt", "outliers_src", k_correspondences=k)
    return clouds, cases


def resolve(clouds, case):
    """the case with its clouds cut out: what ndt_restated.ndt and gicp_restated.gicp take"""
    cut = lambda r: np.ascontiguousarray(clouds[r[0]][int(r[1]):int(r[2])], np.float32)
    return dict(case, tgt=cut(case["tgt"]), src=cut(case["src"]))


def problem(g, name):
    """a case of a loaded fixture as the arguments of Context.ndt / Context.gicp"""
    cut = lambda ref: np.ascontiguousarray(g["cloud/" + ref[0]][ref[1]:ref[2]])
    return dict(tgt=cut(json.loads(str(g[name + "/tgt_ref"]))), src=cut(json.loads(str(g[name + "/src_ref"]))), tgt_bound=g[name + "/tgt_bound"],
                src_bound=g[name + "/src_bound"], init_guess=g[name + "/guess"])
