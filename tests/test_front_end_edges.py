"""The inputs of tests/front_end_edges.py are where they are meant to be: every test here asserts, without a GPU, that an input crosses the capacity or
segment boundary of k_ground.hip / k_ground_normals.hip / k_classify.hip it was made for — so that a changed seed or recipe cannot move it off the
edge unnoticed — and, where oracle/_ref is built, that the oracle equals the reference's own lines on these inputs too (the border wrap, the fine
grids and the tie-heavy lattices are new ground for it).  tests/test_gpu_front_end_edges.py runs the same inputs on the device."""
import numpy as np
import pytest

from mulls_amd import abi
from oracle import pyoracle, pyref

import front_end_edges as fe


@pytest.fixture(scope="module")
def oracle_ground():
    """the oracle's three clouds per ground case, computed once"""
    return {name: pyoracle.ground_filter(cloud(), P) for name, cloud, P in fe.ground_cases()}


@pytest.fixture(scope="module")
def oracle_classes():
    return {name: pyoracle.classify_nground(cloud(), P) for name, cloud, P in fe.classify_cases()}


# ---------------------------------------------------------------------------------------------------------------------------- A. ground filter
def test_segment_sizes_straddle_steps_and_segments(oracle_ground):
    """A.1: the sizes sit on both sides of one 64-point step and of one and two 1024-point segments; from 63 points up two candidates share a cell
    inside one step (the readlane rank decides their order), and the three clouds are non-empty"""
    assert {63, 64, 65} <= set(fe.SEGMENT_SIZES) and {fe.GF_SEG - 1, fe.GF_SEG, fe.GF_SEG + 1, 2 * fe.GF_SEG + 1} <= set(fe.SEGMENT_SIZES)
    for n in fe.SEGMENT_SIZES:
        cloud = fe.segment_cloud(n)
        assert len(cloud) == n
        g = fe.Grid(cloud, fe.segment_params(0))
        if n < 63:
            continue
        assert (g.row, g.col) == (8, 8)
        assert fe.steps_with_shared_cells(g, n) >= 1, n
        for m in (0, 3):
            assert min(len(x) for x in oracle_ground["segment-n%d-m%d" % (n, m)]) > 0, (n, m)


def test_cell_ids_reach_the_upper_half_and_the_last_cell(oracle_ground):
    """A.2: 200 x 200 and exactly 256 x 256 cells; at least 1000 accepted points (ground candidates inside the grid: what k_gf_walk stores a 16-bit
    cell id for) in cells >= 32768, at least 1000 ground points of the oracle from such cells, and the last cell, 65535, holds a ground point"""
    fine, full = fe.Grid(fe.fine_grid_cloud(), fe.fine_params(0.1, 0)), fe.Grid(fe.full_grid_cloud(), fe.fine_params(0.25, 0))
    assert (fine.row, fine.col, fine.num_grid) == (200, 200, 40000)
    assert (full.row, full.col, full.num_grid) == (256, 256, fe.GF_MAXCELLS)
    for g, name in ((fine, "fine-200x200-m0"), (full, "full-256x256-m0")):
        assert int((g.cell[g.candidate] >= 32768).sum()) >= 1000
        assert int((g.cells_of(oracle_ground[name][0]) >= 32768).sum()) >= 1000
    assert (full.cell[full.candidate] == fe.GF_MAXCELLS - 1).any()
    assert (full.cells_of(oracle_ground["full-256x256-m0"][0]) == fe.GF_MAXCELLS - 1).any()
    for m in (1, 2, 3):
        assert len(oracle_ground["fine-200x200-m%d" % m][0]) > 1000 and len(oracle_ground["full-256x256-m%d" % m][0]) > 10000


def test_border_points_wrap_or_drop():
    """A.3: points on the max-x border get col == the column count: they land in column 0 of the next row, or outside the grid in the last row;
    points on the max-y border are outside the grid"""
    g = fe.Grid(fe.full_grid_cloud(), fe.fine_params(0.25, 0))
    on_col = g.pcol == g.col
    assert int((on_col & (g.prow < g.row - 1)).sum()) >= 32
    assert (g.cell[on_col & (g.prow < g.row - 1)] == (g.prow[on_col & (g.prow < g.row - 1)] + 1) * g.col).all()
    assert int((g.cell < 0).sum()) >= 32 and int((on_col & (g.cell < 0)).sum()) >= 1  # the (32, 32) corner: col == 256 in the last row
    assert int(((g.prow == g.row) & (g.cell < 0)).sum()) >= 32


def test_one_cell_more_than_the_table_holds():
    """A.4: 257 x 256 cells: one row more than the 65536 a 16-bit cell id can name"""
    g = fe.Grid(fe.one_cell_more_cloud(), fe.fine_params(0.25, 0))
    assert (g.row, g.col) == (257, 256) and g.num_grid > fe.GF_MAXCELLS
    assert len(fe.one_cell_more_cloud()) == len(fe.full_grid_cloud())


def test_staging_sizes(oracle_ground):
    """A.5: 409 601 points are 4 097 height samples, one more than a staging round holds; 500 000 is the largest scan accepted"""
    n = fe.GF_STAGE * 100 + 1
    assert (n + 99) // 100 == fe.GF_STAGE + 1 and fe.Grid(fe.staging_cloud(n), abi.ground_params()).n_samples == fe.GF_STAGE + 1
    assert len(fe.staging_cloud(fe.GF_MAX_POINTS)) == fe.GF_MAX_POINTS and (fe.GF_MAX_POINTS + 99) // 100 > fe.GF_STAGE
    for k in (n, fe.GF_MAX_POINTS):
        assert min(len(x) for x in oracle_ground["staging-n%d" % k]) > 1000


def test_degenerate_grids(oracle_ground):
    """A.6: a line has zero rows of cells (three empty clouds); 500 points in one cell make a 1 x 1 grid with ground and non-ground points"""
    line, one = fe.Grid(fe.line_cloud(), abi.ground_params()), fe.Grid(fe.one_cell_cloud(), abi.ground_params())
    assert line.row == 0 and line.col > 0 and line.num_grid == 0
    assert (one.row, one.col, one.num_grid) == (1, 1, 1)
    for m in (0, 3):
        assert [len(x) for x in oracle_ground["line-m%d" % m]] == [0, 0, 0]
        assert min(len(x) for x in oracle_ground["one-cell-m%d" % m]) > 0


def test_neighbourhoods_at_the_buffer_size(oracle_ground):
    """A.7: the most crowded ground point of the patch has exactly 1024 ground points within the radius (itself included: what k_gf_normals buffers),
    with four points more exactly 1025; of the lattice, points with more than 1024 within the 1.0 m the k-nearest search starts from (pruned) and
    with fewer (not pruned), and the cut of the K nearest falls inside a group of equal distances for hundreds of the pruned ones"""
    g = oracle_ground["radius-at-cap"][0]
    assert int(fe.neighbour_counts(g, fe.PATCH_RADIUS).max()) == fe.GN_CAP
    over = pyoracle.ground_filter(fe.patch_cloud(fe.PATCH_N_OVER_CAP), fe.patch_params(0))[0]
    assert int(fe.neighbour_counts(over, fe.PATCH_RADIUS).max()) == fe.GN_CAP + 1
    for name, K in (("knn-K12-lattice-pruned", 12), ("knn-K64-lattice-pruned", 64)):
        P = [p for nm, _, p in fe.ground_cases() if nm == name][0]
        assert 2 * P.min_grid_pt_num == K
        counts, ties = fe.neighbour_counts(oracle_ground[name][0], 1.0, K)
        assert int((counts > fe.GN_CAP).sum()) > 1000 and int((counts <= fe.GN_CAP).sum()) > 10 and ties > 200, (name, ties)
    # K = 64 on terrain: found within the first radius by some points, not by the others (their search radius doubles)
    counts = fe.neighbour_counts(oracle_ground["knn-K64-terrain"][0], 1.0)
    assert int((counts >= 64).sum()) > 10 and int((counts < 64).sum()) > 10 and counts.max() <= fe.GN_CAP


def test_abi_capacities_are_below_the_sizes(oracle_ground):
    """A.8: the raw-call test truncates every cloud"""
    sizes = [len(x) for x in oracle_ground["segment-n2049-m0"]]
    assert all(0 < c < s for c, s in zip(fe.ABI_CAPS, sizes))


@pytest.mark.skipif(not pyref.available(), reason="oracle/_ref not built (needs the reference's sources)")
def test_ground_oracle_equals_reference_lines(oracle_ground):
    n = 0
    for name, cloud, P in fe.ground_cases():
        if name in fe.UNDEFINED_UPSTREAM:
            g = fe.Grid(cloud(), P)
            assert P.estimate_ground_normal_method == 3 and (np.bincount(g.cell[g.candidate]) == 2).any()  # two-member cells: no plane model upstream
            continue
        b = pyref.ground_filter(cloud(), P)
        for k, what in enumerate(("ground", "ground_down", "unground")):
            assert oracle_ground[name][k].shape == b[k].shape, (name, what, oracle_ground[name][k].shape, b[k].shape)
            assert np.array_equal(oracle_ground[name][k], b[k]), (name, what)
        n += 1
    assert n >= 30


# ------------------------------------------------------------------------------------------------------------------------------ B. classifier
def test_candidate_counts_straddle_the_buffer_with_ties_at_rank_k(oracle_classes):
    """B.1: queries with at most 256 in-radius candidates and with more, 256 and 257 themselves among them; for every K run, at least 100 pruned
    queries whose neighbours of rank K - 1 and K are equally far; every class cloud non-empty"""
    counts, ties = fe.candidate_census()
    assert int((counts <= fe.CL_CAND).sum()) > 1000 and int((counts > fe.CL_CAND).sum()) > 1000
    assert (counts == fe.CL_CAND).any() and (counts == fe.CL_CAND + 1).any()
    assert all(ties[K] >= 100 for K in (20, 40, 64)), ties
    for K in (20, 40, 64):
        out, after = oracle_classes["prune-K%d-nms1" % K]
        assert all(len(out[k]) > 0 for k in (abi.CL_PILLAR, abi.CL_BEAM, abi.CL_FACADE, abi.CL_ROOF)) and len(after) == len(fe.classify_cloud())
    # the adaptive radius: beyond 30 m every query has its own, larger one; candidates on both sides of the buffer again
    far = fe.xyz32(fe.classify_far_cloud())
    assert int((fe.adaptive_radii(far) > np.float32(1.0)).sum()) > 2000
    assert (fe.adaptive_radii(fe.xyz32(fe.classify_cloud())) == np.float32(1.0)).all()
    counts, ties = fe.candidate_census(adaptive=True)
    assert int((counts <= fe.CL_CAND).sum()) > 500 and int((counts > fe.CL_CAND).sum()) > 500 and ties[40] >= 100


def test_suppression_lists_overflow(oracle_classes):
    """B.1, sharpen_with_nms = 1: a class cloud comes back in the suppression's visiting order (descending normal[3]); in it, points with more than
    32 earlier neighbours within the suppression radius exist (k_cl_nms_round scans their predecessors), and points with fewer"""
    for K in (20, 40, 64):
        out, _ = oracle_classes["prune-K%d-nms1" % K]
        most = 0
        for k in (abi.CL_PILLAR, abi.CL_BEAM, abi.CL_FACADE, abi.CL_ROOF):
            keys = np.ascontiguousarray(out[k][:, 28:32]).view(np.float32).reshape(-1)
            assert len(keys) >= 10 and (np.diff(keys) <= 0).all()
            most = max(most, int(fe.earlier_neighbours(out[k], 0.25 * 1.0).max()))
        assert most > fe.CL_NMS_CAP
        e = fe.earlier_neighbours(out[abi.CL_PILLAR], 0.25 * 1.0)
        assert int((e > fe.CL_NMS_CAP).sum()) > 100 and int((e <= fe.CL_NMS_CAP).sum()) > 100


def test_wide_clouds_need_a_coarser_grid():
    """B.2: more than 2^22 cells of the radius' size; the first cloud fits after one doubling, the second needs two"""
    once, twice = fe.classify_wide_cloud(), fe.classify_wide_cloud(450.0)
    assert fe.cell_product(fe.classify_cloud(), 1.0) <= fe.CL_MAX_CELLS
    assert fe.cell_product(once, 1.0) > fe.CL_MAX_CELLS >= fe.cell_product(once, 2.0)
    assert fe.cell_product(twice, 2.0) > fe.CL_MAX_CELLS >= fe.cell_product(twice, 4.0)


@pytest.mark.parametrize("K", [24, 40])
def test_oracle_labels_equal_a_float64_pca(K):
    """B.3 for the oracle: the labels against numpy's float64 PCA of the same neighbourhoods, every point checked"""
    cloud = fe.classify_cloud()
    out, _ = pyoracle.classify_nground(cloud, abi.classify_params(neighbor_k=K, sharpen_with_nms=0, extract_vertex_points_method=0))
    want, checked = fe.float64_labels(cloud, K)
    assert int((~checked).sum()) <= len(cloud) // 100
    assert np.array_equal(fe.classify_labels(cloud, out)[checked], want[checked])
    assert all(int((want == lab).sum()) > 50 for lab in (1, 2, 3, 4))


def test_index_order_follows_space(oracle_classes):
    """B.4: ascending x; in the chain cloud the promotion loop gives most beams their label, and nearly every promoted point has a promoted point
    of lower index among its neighbours, whose verdict it has to wait for"""
    for cloud in (fe.classify_sorted_cloud(), fe.promotion_chain_cloud()):
        assert (np.diff(abi.points_of(cloud)["x"]) >= 0).all()
    assert sorted(map(bytes, fe.classify_sorted_cloud())) == sorted(map(bytes, fe.classify_cloud()))
    out, _ = oracle_classes["promotion-chain-nms0"]
    promoted, waiting = fe.promoted_with_promoted_predecessor(fe.promotion_chain_cloud(), out[abi.CL_BEAM], 20)
    assert promoted >= 100 and waiting >= 90, (promoted, waiting)
    assert len(oracle_classes["sorted-by-x"][0][abi.CL_VERTEX]) > 0 and len(oracle_classes["promotion-chain"][0][abi.CL_VERTEX]) > 100


def test_prefix_sizes(oracle_classes):
    """B.5: one query less than, exactly and one more than a block of 256, and 1025"""
    for n in (255, 256, 257, 1025):
        out, after = oracle_classes["prefix-n%d" % n]
        assert len(after) == n and sum(len(o) for o in out[:4]) > 50


@pytest.mark.skipif(not pyref.available(), reason="oracle/_ref not built (needs the reference's sources)")
def test_classify_oracle_equals_reference_lines(oracle_classes):
    n = 0
    for name, cloud, P in fe.classify_cases():
        a, a_in = oracle_classes[name]
        b, b_in = pyref.classify_nground(cloud(), P)
        for k in range(abi.CL_COUNT):
            assert a[k].shape == b[k].shape, (name, abi.CL_NAMES[k], a[k].shape, b[k].shape)
            assert np.array_equal(a[k], b[k]), (name, abi.CL_NAMES[k])
        assert np.array_equal(a_in, b_in), name
        n += 1
    assert n >= 15
