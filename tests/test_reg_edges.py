"""CPU tests of the size and table-edge cases of NDT and GICP (tests/reg_edges.py): the fixtures tests/golden/ndt_edges.npz and gicp_edges.npz against the
numpy restatements, and the conditions that make every case mean something — which case reaches which edge of k_ndt.hip / k_gicp.hip, asserted on the
scenes and on the restatement's trace, never assumed.  tests/test_gpu_reg_edges.py compares the device with the fixtures.

The restatements were written from reading upstream; nothing here was compared with ndt_omp, fast_gicp or PCL themselves.

The restatements run once per solver for the whole module (`fresh`) and every test reads that one run: about a minute and a half of CPU time for the
file, most of it the twelve calls on the 9 000-point target."""
import collections
import json
import os
import sys

import numpy as np
import pytest

mpmath = pytest.importorskip("mpmath")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import gicp_restated as gr  # noqa: E402
import ndt_restated as nr  # noqa: E402
import reg_edges as E  # noqa: E402

GOLDEN = {s: os.path.join(ROOT, "tests", "golden", "%s_edges.npz" % s) for s in ("ndt", "gicp")}
NDT_NAMES = ["wide_4095", "wide_4096", "wide_4097", "wide_8193", "wide_8193_crop", "wide_8193_direct26", "wide_8193_direct1", "dense_table", "full_cell",
             "grid_almost_full"]
GICP_NAMES = ["wide_4095", "wide_4096", "wide_4097", "wide_8193", "wide_8193_crop", "dense_table", "full_cell", "range_edge", "k3", "k3_outliers", "k8",
              "k8_outliers", "k9", "k9_outliers", "k21", "k21_outliers"]
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def fresh():
    """per solver: the fixture recomputed, what the restatement returned per case with its trace, and the scenes"""
    import make_reg_edges_golden

    out = {}
    for solver in ("ndt", "gicp"):
        arrays, seen = make_reg_edges_golden.compute(solver)
        clouds, cases = E.build(solver)
        out[solver] = dict(arrays=arrays, seen=seen, case={n: E.resolve(clouds, c) for n, c in cases.items()})
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class tree_width:
    """the restatements' strided partials at another width, for the time of a `with`"""

    def __init__(self, width):
        self.width = width

    def __enter__(self):
        self.was, nr.TREE = nr.TREE, self.width

    def __exit__(self, *exc):
        nr.TREE = self.was


# ---- 1. the fixtures

@pytest.mark.parametrize("solver", ["ndt", "gicp"])
def test_fixture_equals_the_restatement(fresh, solver):
    z = np.load(GOLDEN[solver])
    new = fresh[solver]["arrays"]
    assert json.loads(str(z["names"])) == (NDT_NAMES if solver == "ndt" else GICP_NAMES)
    assert sorted(new) == sorted(z.files)
    for k in z.files:
        a, b = z[k], new[k]
        if a.dtype.kind in "US":
            assert str(a) == str(b), k
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    # every cloud once: a case holds references only
    assert not [k for k in z.files if k.endswith("/tgt") or k.endswith("/src")]
    assert os.path.getsize(GOLDEN[solver]) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "pgo_cases.npz"))


# ---- 2. wide_*: more source points than MULLS_NDT_TREE lanes

def first_terms(fresh, solver, name, grids):
    """the (n_src, 28) per-point terms of the case's first evaluation, the cropped clouds, and the final pose's fitness arguments"""
    c, seen = fresh[solver]["case"][name], fresh[solver]["seen"][name]
    res, trace = seen["res"], seen["trace"]
    pp = []
    if solver == "ndt":
        prm = nr.default_params(**c["prm"])
        tgt_c, src_c, _ = nr.crop(c["tgt"], c["src"], c["tgt_bound"], c["src_bound"], c["guess"], prm["apply_intersection_filter"])
        if "ndt" not in grids:  # (the wide cases without the crop share their target)
            grids["ndt"] = nr.build_grid(tgt_c, prm["resolution"], prm["min_points_per_voxel"], prm["min_covar_eigvalue_mult"])
        d1, d2, _ = nr.gauss_constants(prm["resolution"], prm["outlier_ratio"])
        xt, with_h, phase, recorded = trace[0]
        assert xt == [0.0] * 6 and with_h == 1 and phase == nr.PH_INIT
        sums = nr.evaluate(src_c, xt, grids["ndt"], d1, d2, 1, prm["search_method"], per_point_out=pp)
        fitness = lambda: nr.fitness_of(src_c, tgt_c, res["p"])
    else:
        prm = gr.default_params(**c["prm"])
        tgt_c, src_c = res["tgt_c"], res["src_c"]
        vm = gr.build_voxels(tgt_c, res["C_tgt"], prm["voxel_resolution"])
        r, t, R, recorded, n_corr = trace[0]
        sums, n = gr.evaluate(src_c, res["C_src"], vm, R, t, per_point_out=pp)
        assert n == n_corr
        T = np.asarray(res["T"])
        fitness = lambda: gr.fitness_of(src_c, tgt_c, [float(v) for v in T[:3, :3].reshape(-1)], [float(v) for v in T[:3, 3]])
    assert same_bits(sums, recorded)
    return pp[0], recorded, fitness


@pytest.mark.parametrize("solver", ["ndt", "gicp"])
def test_wide_cases_reach_the_later_trips(fresh, solver):
    """n_src is exactly 4 095, 4 096, 4 097 and 8 193; the points of the second and third trip of a lane (4 096 .., 8 192) add non-zero terms at the first
    evaluation; and the recorded bits depend on the order the definition states.

    The order, measured against other orders of the same additions.  Each of these changes some of the 28 recorded sums, in both cases (asserted):
    a stride of 4 095 (lane l adds l, l + 4095, ..: the later trips land one lane off), the first trip alone (the later trips dropped), and the plain
    running sum over the points in order.  A device that walks the later trips with another stride, skips them, or adds in point order cannot pass.

    A width of 8 192 lanes in place of 4 096 is NOT such an order, and the test says why instead of asserting a change that cannot be relied on:
    - wide_4097: no sum can change.  With at most 2 x 4 096 points the width-4 096 partial of lane l is t_l + t_(l + 4096), which is exactly the first
      level of the width-8 192 tree, and the levels below are the same tree (asserted: 0 of 28 change).
    - wide_8193: only lane 0 differs, (t0 + t8192) + t4096 for the definition's (t0 + t4096) + t8192: at most one rounding of a three-term sum, which
      then enters a total of 8 193 terms and is rounded away (measured: 0 of 28 change for both solvers; printed).
    The fitness is the sum of n_src float squared distances in double.  A few 24-bit values of like exponent add up exactly in any order, and in these
    scenes even the plain running sum gives the recorded bits (printed).  What the fitness does depend on is that every trip is added: the first
    trip alone gives other bits (asserted).  So the 28 sums pin the order, and the fitness pins that k_ndt_fitness walks the later trips."""
    I = {n: dict(zip(("n_src", "n_tgt"), fresh[solver]["arrays"][n + "/ints"][[6, 7] if solver == "ndt" else [4, 5]])) for n in NDT_NAMES[:5]}
    for n in E.WIDE_NS:
        assert I["wide_%d" % n] == dict(n_src=n, n_tgt=9000)
    kept = I["wide_8193_crop"]["n_src"]
    assert 4096 < kept < 8193 and kept % 256 != 0 and I["wide_8193_crop"]["n_tgt"] < 9000
    assert E.table_log2(9000) == 15  # 32 768 slots: segments of 32 per thread of the offsets kernels; ceil(9000 / 1024) = 9 points per thread of the crop
    grids = {}
    for name in ("wide_4097", "wide_8193"):
        terms, recorded, fitness = first_terms(fresh, solver, name, grids)
        adds = terms.any(axis=1)
        assert adds[0] and adds[4096], name
        if name == "wide_8193":
            assert adds[8192] and adds[4096:8192].sum() >= 3000, adds[4096:8192].sum()
        assert same_bits(nr.tree_sum(terms), recorded)
        with tree_width(8192):
            at_8192 = nr.tree_sum(terms)
            fit_8192 = fitness()
        off_by_one = np.zeros((nr.TREE, 28))
        for i in range(len(terms)):
            off_by_one[i % (nr.TREE - 1)] += terms[i]
        running = np.zeros(28)
        for row in terms:
            running += row
        changed = lambda s: int((np.ascontiguousarray(s).view(np.uint64) != np.ascontiguousarray(recorded, np.float64).view(np.uint64)).sum())
        others = dict(stride_4095=changed(nr.tree_sum(off_by_one)), first_trip=changed(nr.tree_sum(terms[:nr.TREE])), running=changed(running))
        print(solver, name, "of 28 sums, changed at width 8192:", changed(at_8192), others)
        assert min(others.values()) >= 1, (name, others)
        assert name != "wide_4097" or changed(at_8192) == 0
        # the fitness
        want = fresh[solver]["arrays"][name + "/floats"][0]
        assert fitness() == want and fit_8192 == want
        c, res = fresh[solver]["case"][name], fresh[solver]["seen"][name]["res"]
        n = len(c["src"])
        first_trip = fitness_terms(solver, c, res)
        assert float(nr.tree_sum(first_trip)) / n == want
        assert float(nr.tree_sum(first_trip[:4096])) / n != want
        run = 0.0
        for v in first_trip:
            run += float(v)
        print(solver, name, "fitness", want, "running sum", run / n, "(equal)" if run / n == want else "(other bits)")


def fitness_terms(solver, c, res):
    """the float squared distances the fitness sums, as doubles (no crop in these cases)"""
    if solver == "ndt":
        xp = nr.transform(nr.make_frame(res["p"]), c["src"])
    else:
        T = np.asarray(res["T"])
        xp = gr.move([float(v) for v in T[:3, :3].reshape(-1)], [float(v) for v in T[:3, 3]], c["src"]).astype(np.float32)
    d2 = np.empty(len(xp), np.float32)
    for b in range(0, len(xp), 256):
        d = xp[b:b + 256, None, :] - c["tgt"][None, :, :]
        d2[b:b + 256] = ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).min(axis=1)
    return d2.astype(np.float64)


def test_ndt_wide_neighbourhoods_differ(fresh):
    a = fresh["ndt"]["arrays"]
    assert len({a[n + "/T"].tobytes() for n in ("wide_8193", "wide_8193_direct26", "wide_8193_direct1", "wide_8193_crop")}) == 4
    for n in NDT_NAMES[:7]:
        assert a[n + "/ints"][1] >= 1, n  # iterations


# ---- 3. dense_table: long probe sequences, the wrap past the last slot, misses that walk a stretch to its first empty slot

def table_facts(keys_homes, slots):
    """the occupied slots; the longest stretch; the wrapping stretch's first slot, the keys that have their home in it, its slots before the end"""
    homes = np.array(list(keys_homes.values()))
    occ = E.occupied(homes, slots)
    assert occ.sum() == len(homes)
    first, length = E.longest_run(occ)
    a, n_home, room = E.wrap_of(homes, occ)
    return occ, length, a, n_home, room


def miss_kinds(missing_homes, occ, a):
    """of lookups of absent keys: how many start inside a stretch of >= 16 slots that ends before the table does and walk it to its first empty
    slot; how many start in the wrapping stretch before the end, so that the walk goes past the last slot"""
    in_run = in_wrap = 0
    longest = 0
    for h in missing_homes:
        walk = E.miss_walk(h, occ)
        longest = max(longest, len(walk))
        r = E.run_of(occ, h)
        if r is not None and r[1] < len(occ) - 1 and r[1] - r[0] + 1 >= 16 and len(walk) >= 2:
            in_run += 1
        if a is not None and h >= a:
            assert walk[0] >= a and len(occ) - 1 in walk and walk[-1] < a  # past the last slot, on to the first empty one
            in_wrap += 1
    return in_run, in_wrap, longest


def test_ndt_dense_table(fresh):
    c, seen = fresh["ndt"]["case"]["dense_table"], fresh["ndt"]["seen"]["dense_table"]
    prm = nr.default_params(**c["prm"])
    assert prm["apply_intersection_filter"] == 0 and 512 <= len(c["tgt"]) <= 2000
    grid = nr.build_grid(c["tgt"], 1.0)
    lg = E.table_log2(len(c["tgt"]))
    slots = 1 << lg
    homes = {k: E.ndt_home(k, lg) for k in grid.index}
    occ, length, a, n_home, room = table_facts(homes, slots)
    load = len(homes) / slots
    print("ndt dense_table: %d cells in %d slots (%.3f), longest stretch %d, wrapping stretch from %d: %d keys for %d slots" % (len(homes), slots, load, length, a, n_home, room))
    assert 0.44 <= load < 0.5 and len(homes) >= 0.9 * len(c["tgt"])  # almost one point per cell
    assert length >= 16
    assert a is not None and n_home > room  # more keys than slots before the end: the table wraps, whatever the order of insertion
    # the keys that may have been pushed past the end are usable leaves, and the source looks every one of them up
    used = {k for k, li in grid.index.items() if grid.n[li] >= prm["min_points_per_voxel"]}
    pushed = {k for k, h in homes.items() if h >= a}
    assert pushed <= used and seen["res"]["n_leaves_used"] == len(used) >= 30
    # the first evaluation's lookups (DIRECT7 around every source point under the identity)
    xt = seen["trace"][0][0]
    assert xt == [0.0] * 6
    q = np.floor(nr.transform(nr.make_frame(xt), c["src"]) / np.float32(1.0)).astype(np.int64)
    hit, missing = set(), []
    for off in nr.offsets_of(prm["search_method"]):
        cell = q + np.array(off)
        for cc in cell:
            if all(grid.min_b[k] <= cc[k] <= grid.max_b[k] for k in range(3)):
                key = int((cc[0] - grid.min_b[0]) + (cc[1] - grid.min_b[1]) * grid.div_b[0] + (cc[2] - grid.min_b[2]) * grid.div_b[0] * grid.div_b[1])
                if key in grid.index:
                    hit.add(key)
                else:
                    missing.append(E.ndt_home(key, lg))
    assert pushed <= hit
    in_run, in_wrap, longest = miss_kinds(missing, occ, a)
    print("ndt dense_table: %d lookups miss; %d walk a stretch of >= 16 slots, %d walk past the last slot; the longest walk reads %d slots" % (len(missing), in_run, in_wrap, longest))
    assert in_run >= 3 and in_wrap >= 3
    assert seen["res"]["iterations"] >= 1


def test_gicp_dense_table(fresh):
    c, seen = fresh["gicp"]["case"]["dense_table"], fresh["gicp"]["seen"]["dense_table"]
    prm = gr.default_params(**c["prm"])
    tgt = c["tgt"]
    assert prm["apply_intersection_filter"] == 0 and 512 <= len(tgt) <= 2000
    lg = E.table_log2(len(tgt))
    slots = 1 << lg
    vc, ok = gr.voxel_coords(tgt, 1.0)
    kc, ok2 = gr.knn_coords(tgt, 1.0)
    assert ok.all() and ok2.all()
    tables = {"voxel": {gr.pack(v) for v in vc}, "neighbour": {gr.pack(v) for v in kc}}
    assert tables["voxel"] == tables["neighbour"]  # (every point lies in the upper half of its cell: both tables hold the same keys)
    # the lookups.  voxel table: the voxel of every moved source point at the first evaluation.  neighbour table: rings 0 and 1 around every target
    # point's cell (the walk never certifies before ring 1).
    r, t, R, sums, n_corr = seen["trace"][0]
    sc, oks = gr.voxel_coords(gr.move(R, t, c["src"]).astype(np.float32), 1.0)
    looked = {"voxel": {gr.pack(v) for v, o in zip(sc, oks) if o},
              "neighbour": {gr.pack(np.array(cell) + (dx, dy, dz)) for cell in {tuple(v) for v in kc} for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)}}
    for name, keys in tables.items():
        homes = {k: gr.home_slot(k, lg) for k in keys}
        occ, length, a, n_home, room = table_facts(homes, slots)
        load = len(keys) / slots
        print("gicp dense_table, %s table: %d cells in %d slots (%.3f), longest stretch %d, wrapping stretch from %d: %d keys for %d slots" % (name, len(keys), slots, load, length, a, n_home, room))
        assert 0.47 <= load < 0.5 and len(keys) >= 0.95 * len(tgt)
        assert length >= 16 and a is not None and n_home > room
        pushed = {k for k, h in homes.items() if h >= a}
        assert pushed <= looked[name]  # whichever key went past the end is looked up
        missing = [gr.home_slot(k, lg) for k in looked[name] - keys]
        in_run, in_wrap, longest = miss_kinds(missing, occ, a)
        print("    %d lookups miss; %d walk a stretch of >= 16 slots, %d walk past the last slot; the longest walk reads %d slots" % (len(missing), in_run, in_wrap, longest))
        assert in_run >= 3 and in_wrap >= 3, name
    assert seen["res"]["n_corr"] > 0 and seen["res"]["iterations"] >= 1 and seen["res"]["n_voxels"] == len(tables["voxel"])


# ---- 4. full_cell: cells fuller than the one-lane sort's first gaps

@pytest.mark.parametrize("solver", ["ndt", "gicp"])
def test_full_cells_hold_exactly_their_counts(fresh, solver):
    c, res = fresh[solver]["case"]["full_cell"], fresh[solver]["seen"]["full_cell"]["res"]
    tgt = c["tgt"]
    if solver == "ndt":
        cell = np.floor(tgt * (np.float32(1.0) / np.float32(1.0))).astype(np.int64)
    else:
        cell, ok = gr.voxel_coords(tgt, 1.0)
        assert ok.all()
    counts = collections.Counter(map(tuple, cell))
    assert [counts[k] for k, _ in E.FULL_CELLS] == [1751, 1749, 1750, 702] == [n for _, n in E.FULL_CELLS]
    assert sorted(counts.values())[-5] < 100  # an ordinary scene otherwise
    for k, n in E.FULL_CELLS:  # the target is permuted: a cell's points are spread over the whole cloud
        idx = np.flatnonzero((cell == np.array(k)).all(axis=1))
        assert idx[-1] - idx[0] > 0.9 * len(tgt) and (np.diff(idx) > 1).sum() > 0.5 * n
    assert res["n_src"] == len(c["src"]) and res["n_tgt"] == len(tgt) == 7452 and res["iterations"] >= 1
    # the source has points in each of the four cells, so that their leaves / voxels enter the sums
    if solver == "ndt":
        sc = np.floor(c["src"]).astype(np.int64)
    else:
        r, t, R, sums, n_corr = fresh[solver]["seen"]["full_cell"]["trace"][0]
        sc, _ = gr.voxel_coords(gr.move(R, t, c["src"]).astype(np.float32), 1.0)
    for k, _ in E.FULL_CELLS:
        assert (sc == np.array(k)).all(axis=1).sum() >= 20, k


# ---- 5. range_edge (GICP): cells at -1048576 and 1048575

def test_gicp_range_edge(fresh):
    c, seen = fresh["gicp"]["case"]["range_edge"], fresh["gicp"]["seen"]["range_edge"]
    tgt, src = c["tgt"], c["src"]
    assert np.array_equal(tgt * 8, np.round(tgt * 8)) and np.array_equal(src * 8, np.round(src * 8))
    # the accepted limits, against the two coordinate rules: they differ
    one = lambda f, x: (lambda q, ok: (int(q[0, 0]), bool(ok[0])))(*f(np.full((1, 3), x, np.float32), 1.0))
    assert one(gr.voxel_coords, -1048575.5) == (-1048576, True) and not one(gr.voxel_coords, -1048575.625)[1]
    assert one(gr.knn_coords, -1048576.0) == (-1048576, True) and not one(gr.knn_coords, -1048576.125)[1]
    assert one(gr.voxel_coords, 1048576.25) == (1048575, True) and not one(gr.voxel_coords, 1048576.5)[1]
    assert one(gr.knn_coords, 1048575.875) == (1048575, True) and not one(gr.knn_coords, 1048576.0)[1]
    assert (E.LIMIT_LO, E.LIMIT_HI) == (-1048575.5, 1048575.875) and tgt.min() == E.LIMIT_LO and tgt.max() == E.LIMIT_HI
    # one step further is refused
    eye, b = np.eye(4), np.zeros(6)
    for which, bad in (("tgt", 1048576.0), ("tgt", -1048575.625), ("src", 1048576.0), ("src", -1048576.125)):
        far = dict(tgt=tgt, src=src)
        far[which] = np.concatenate([far[which], np.full((1, 3), bad, np.float32)])
        assert gr.gicp(far["tgt"], far["src"], b, b, eye, gr.default_params(**c["prm"])) is None, (which, bad)
    vt, ok = gr.voxel_coords(tgt, 1.0)
    kt, ok2 = gr.knn_coords(tgt, 1.0)
    ks, ok3 = gr.knn_coords(src, 1.0)
    assert ok.all() and ok2.all() and ok3.all()
    for name, cells in (("voxel", vt), ("target neighbour", kt), ("source neighbour", ks)):
        for axis in range(3):
            assert cells[:, axis].min() == -1048576 and cells[:, axis].max() == 1048575, (name, axis)
    # a source point the neighbour cells accept and no voxel can hold
    _, oks = gr.voxel_coords(src, 1.0)
    assert (~oks).sum() == 1 and src[~oks][0, 0] == -1048576.0
    # the ring walk around the extreme cells skips neighbours beyond the range on both sides, and still certifies: the 20th neighbour of the extreme
    # points lies within MULLS_GICP_MAX_RING = 3 cells (sor_math.h certifies a list whose worst squared distance is at most (ring x edge)^2 (1 - 2^-18))
    for P in (tgt, src):
        for ext in (E.LIMIT_LO, E.LIMIT_HI):
            i = int(np.flatnonzero((P == ext).all(axis=1))[0])
            d = P - P[i]
            d2 = np.sort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            assert d2[19] <= 9.0 * (1.0 - 2.0 ** -18), (ext, d2[19])
    res = seen["res"]
    assert res is not None and res["n_corr"] > 0 and res["n_src"] == len(src) and res["n_tgt"] == len(tgt) == 800
    r, t, R, sums, n_corr = seen["trace"][0]
    assert r == [0.0, 0.0, 0.0] and n_corr >= len(src) // 2  # the loop starts at the identity: the clusters overlap as built
    print("range_edge: n_corr %d of %d, %d iterations, stop %d" % (res["n_corr"], len(src), res["iterations"], res["stop"]))


# ---- 6. grid_almost_full (NDT): int32 keys near 2^31

def test_ndt_grid_almost_full(fresh):
    c, seen = fresh["ndt"]["case"]["grid_almost_full"], fresh["ndt"]["seen"]["grid_almost_full"]
    tgt, src = c["tgt"], c["src"]
    prm = nr.default_params(**c["prm"])
    assert prm["apply_intersection_filter"] == 0
    inv = np.float32(1.0) / np.float32(prm["resolution"])
    mn, mx = tgt.min(axis=0), tgt.max(axis=0)
    d = [int(np.float32(mx[k] - mn[k]) * inv) + 1 for k in range(3)]  # k_ndt_crop's prod
    grid = nr.build_grid(tgt, prm["resolution"])
    prod, prod_b = d[0] * d[1] * d[2], grid.div_b[0] * grid.div_b[1] * grid.div_b[2]  # (python integers: no overflow here)
    print("grid_almost_full: extents", d, grid.div_b, "products", prod, prod_b, "of", INT32_MAX)
    assert 2 ** 30 < prod <= INT32_MAX and 2 ** 30 < prod_b <= INT32_MAX and grid.div_b == [E.GRID_CELLS] * 3
    assert 2 ** 30 < max(grid.index) == E.GRID_CELLS ** 3 - 1 <= INT32_MAX
    corner = grid.leaves[grid.index[max(grid.index)]]
    assert corner["n"] == 8 >= prm["min_points_per_voxel"]  # usable
    # the first evaluation: the source points in the corner leaf add terms; those two cells beyond it have no cell inside the grid
    xt = seen["trace"][0][0]
    assert xt == [0.0] * 6
    d1, d2, _ = nr.gauss_constants(prm["resolution"], prm["outlier_ratio"])
    pp = []
    sums = nr.evaluate(src, xt, grid, d1, d2, 1, prm["search_method"], per_point_out=pp)
    assert same_bits(sums, seen["trace"][0][3])
    q = np.floor(src).astype(np.int64)
    in_corner = (q == np.array(grid.max_b)).all(axis=1)
    assert in_corner.sum() == 6 and pp[0][in_corner].any(axis=1).all()
    beyond = (q > np.array(grid.max_b)).any(axis=1)
    assert beyond.sum() == 9 and ((q - np.array(grid.max_b)).max(axis=1) >= 2).sum() == 4 and not pp[0][(q - np.array(grid.max_b)).max(axis=1) >= 2].any()
    one_out = beyond & ((q - np.array(grid.max_b)).clip(0).sum(axis=1) == 1)
    assert one_out.sum() == 3 and pp[0][one_out].any(axis=1).all()  # one cell beyond on one axis: DIRECT7's offset back into the grid finds the corner leaf
    assert seen["res"]["n_leaves"] == len(grid.index) and seen["res"]["iterations"] >= 1
    # one more cell on any axis and the grid is refused
    far = np.concatenate([tgt, (tgt.max(axis=0) + [1.0, 0.0, 0.0])[None]]).astype(np.float32)
    assert nr.build_grid(far, prm["resolution"]) is None


# ---- 7. k3, k8, k9, k21 (GICP): the register lists' capacities

def test_gicp_k_cases(fresh):
    a, case = fresh["gicp"]["arrays"], fresh["gicp"]["case"]
    assert E.KS == (3, 8, 9, 21)  # the minimum; fills KBest<8>; the smallest in KBest<20>; the smallest in KBest<32>
    old = np.load(os.path.join(ROOT, "tests", "golden", "gicp_cases.npz"))
    poses = {a["k%d" % k + "/T"].tobytes() for k in E.KS} | {old[n + "/T"].tobytes() for n in ("street", "street_k5", "street_k32")}
    assert len(poses) == 7
    assert len({a["k%d_outliers" % k + "/T"].tobytes() for k in E.KS}) == 4
    for k in E.KS:
        for name in ("k%d" % k, "k%d_outliers" % k):
            assert json.loads(str(a[name + "/prm"])) == dict(k_correspondences=k)
            ints = dict(zip(("code", "iterations", "converged", "stop", "n_src", "n_tgt", "n_voxels", "n_corr"), a[name + "/ints"]))
            assert ints["iterations"] >= 1 and ints["n_corr"] > 0, name
        # outliers: points whose k-th neighbour lies beyond three cells of 1 m, in both clouds: no ring walk certifies them, the brute kernel runs
        c = case["k%d_outliers" % k]
        for cloud, few in ((c["tgt"], 4), (c["src"], 3)):
            d = cloud[-few:, None, :] - cloud[None, :, :]
            d2 = np.sort((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2], axis=1)
            assert (d2[:, k - 1] > 9.0 * 100).all(), k
