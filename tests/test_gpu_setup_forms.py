"""The setup of a registration in its two shapes: k_src_setup (clone + box + crop of a pair's source side in one workgroup) and k_tgt_grid by size bucket
(4 / 8 / 12 / 19 trips of 512 points) against MULLS_OPT_DEBUG_STOP = 30, the former shape (k_clone_src + k_crop for every pair, one 19-trip k_tgt_grid
workgroup per class cloud).  Same bits: every integer output and the bytes of T, info, sigma.  Synthetic planes, three or four iterations."""
import numpy as np
import pytest

from mulls_amd import abi, synth
from oracle import pyoracle

pytestmark = pytest.mark.gpu

SRC_CAP = 4096  # MULLS_SRC_SETUP_CAP: staged source points of a pair that k_src_setup takes
BUCKET_EDGES = (0, 1, 511, 512, 513, 2047, 2048, 2049, 4096, 4097, 6144, 6145, 9727, 9728)


@pytest.fixture(scope="module")
def ctxs():
    """the LDS tier for the whole batch (every class cloud through k_tgt_grid, up to 9728 points) and the default tier selection (clouds beyond the
    on-chip duplicate table's reach go to the global-memory tier: a mixed batch)"""
    from mulls_amd import lib

    lds, auto = lib.Context(0), lib.Context(0)
    lds.set_nn_mode(3)
    yield {"grid_lds": lds, "auto": auto}
    lds.close()
    auto.close()


def cloud(rng, cls, n):
    """n points of class cls: ground / roof planes, two facade planes, poles, beams, scattered vertices"""
    if n == 0:
        return None
    p = rng.uniform(-10, 10, (n, 3))
    if cls == abi.GROUND:
        p[:, 2], nrm = -1.7, [0, 0, 1]
    elif cls == abi.ROOF:
        p[:, 2], nrm = 5.0, [0, 0, 1]
    elif cls == abi.FACADE:
        half = n // 2
        p[:half, 1], p[half:, 0] = 9.0, 12.0
        nrm = np.where(np.arange(n)[:, None] < half, [[0, -1, 0]], [[-1, 0, 0]])
    elif cls == abi.PILLAR:
        base = rng.uniform(-8, 8, (12, 2))
        p[:, :2], nrm = base[rng.integers(0, 12, n)], [0, 0, 1]
        p[:, 2] = rng.uniform(-1.7, 3.0, n)
    elif cls == abi.BEAM:
        rows = rng.uniform(-8, 8, (8, 2))
        k = rng.integers(0, 8, n)
        p[:, 1], p[:, 2], nrm = rows[k, 0], 3.0 + 0.1 * rows[k, 1], [1, 0, 0]
    else:
        nrm = [0, 0, 1]
    return abi.make_points(p, np.broadcast_to(np.asarray(nrm, np.float64), (n, 3)), rng.uniform(0, 255, n), rng.uniform(0, 1, n))


def moved(c, T, n):
    """the first n points of c under the rigid transform T (float64 math, float32 store)"""
    if c is None or n == 0:
        return None
    c = c[:n]
    xyz = np.column_stack([c["x"], c["y"], c["z"]]).astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    nrm = np.column_stack([c["nx"], c["ny"], c["nz"]]).astype(np.float64) @ T[:3, :3].T
    return abi.make_points(xyz, nrm, c["intensity"], c["curvature"])


def pair_of(rng, tgt_sizes, src_sizes, T=None):
    """a pair with the given class-cloud sizes; a source cloud is cut out of a target-like cloud of its class and moved a little.  The guess is a small
    motion too, so that k_src_setup's transform is not the identity"""
    T = synth.se3(0.15, -0.1, 0.02, 0.0, 0.0, 0.01) if T is None else T
    tgt = [cloud(rng, c, n) for c, n in enumerate(tgt_sizes)]
    src = [moved(cloud(rng, c, n), T, n) for c, n in enumerate(src_sizes)]
    return abi.PairData(tgt, src, init_guess=synth.se3(0.02, 0.01, 0.0, 0.0, 0.0, 0.002))


def rows(results):
    return [(x.code, x.iters, tuple(x.ncorr), tuple(x.nsrc0), tuple(x.ntgt0), x.cropped, tuple(x.crop_box), np.array(x.T[:]).tobytes(),
             np.array(x.info[:]).tobytes(), np.float32(x.sigma).tobytes()) for x in results]


def both_shapes(c, run):
    """run() under the current setup, the former one, and the current one again: the three row lists"""
    out = []
    try:
        for stop in (0, 30, 0):
            c.set_option(abi.OPT_DEBUG_STOP, stop)
            out.append(rows(run()))
    finally:
        c.set_option(abi.OPT_DEBUG_STOP, 0)
    return out


@pytest.fixture(scope="module")
def edge_pairs():
    """target class clouds on every bucket edge; a pair with everything cropped away; a pair without targets; a class empty between two others"""
    rng = np.random.default_rng(41)
    src = (700, 300, 800, 1, 150, 90)
    sizes = ((9728, 513, 2049, 0, 1, 511), (4096, 2047, 9727, 512, 2048, 0), (6144, 4097, 6145, 1, 513, 512))
    assert set(BUCKET_EDGES) == {n for s in sizes for n in s}
    pairs = [pair_of(rng, s, src) for s in sizes]
    far = pair_of(rng, (600, 200, 700, 0, 0, 0), (300, 100, 300, 0, 0, 0), T=synth.se3(200.0, 0, 0))
    none = pair_of(rng, (0,) * 6, src)
    return pairs + [far, none]


@pytest.mark.parametrize("crop", [1, 0])
@pytest.mark.parametrize("tier", ["grid_lds", "auto"])
def test_bucket_edges_same_bits(ctxs, edge_pairs, tier, crop):
    """every bucket edge, intersection filter on and off; under the default tier selection the 9727 / 9728-point targets of searched classes are a
    mixed batch's global-memory clouds (k_crop's list keeps their target sides), under grid_lds they are the 19-trip bucket"""
    c = ctxs[tier]
    b = c.batch(edge_pairs)
    try:
        for P in (abi.kitti_params(dis_thre_unit=2.4, max_iter_num=4, apply_intersection_filter=crop),
                  abi.default_params(used_feature_type="111111", max_iter_num=3, apply_intersection_filter=crop)):
            new, old, again = both_shapes(c, lambda: list(b.run(P)) + [c.icp(edge_pairs[0], P)[0]])
            assert new == again
            assert new == old
            if not crop:  # (nothing cropped: the sizes are the staged ones)
                assert new[0][4] == (9728, 513, 2049, 0, 1, 511) and new[4][4] == (0,) * 6
            else:
                assert sum(new[3][2]) == 0  # the far pair: nothing left to match
    finally:
        b.close()


@pytest.fixture(scope="module")
def cap_pairs():
    """source totals of k_src_setup's capacity and one more (both paths in one launch set), a class of one point, a pair whose source is empty"""
    rng = np.random.default_rng(43)
    tgt = (1500, 600, 1500, 300, 200, 100)
    at = pair_of(rng, tgt, (1500, 596, 1500, 300, 199, 1))
    over = pair_of(rng, tgt, (1500, 597, 1500, 300, 199, 1))
    empty = pair_of(rng, tgt, (0,) * 6)
    assert sum(len(s) for s in at.src if s is not None) == SRC_CAP
    return [at, over, empty]


@pytest.mark.parametrize("copies", [1, 34], ids=["3_pairs", "102_pairs_two_sub_batches"])
def test_source_capacity_edge_same_bits(ctxs, cap_pairs, copies):
    c = ctxs["auto"]
    plist = cap_pairs * copies
    b = c.batch(plist)
    try:
        for P in (abi.kitti_params(dis_thre_unit=2.4, max_iter_num=4), abi.default_params(used_feature_type="111111", max_iter_num=3, apply_intersection_filter=0)):
            new, old, again = both_shapes(c, lambda: list(b.run(P)))
            assert new == again
            assert new == old
            if not P.apply_intersection_filter:  # (nothing cropped: the sizes are the staged ones)
                assert new[0][3] == (1500, 596, 1500, 300, 199, 1) and new[1][3] == (1500, 597, 1500, 300, 199, 1) and new[2][3] == (0,) * 6
            assert new[:3] == new[-3:]
    finally:
        b.close()


def test_one_pair_batch_same_bits(ctxs, cap_pairs):
    c = ctxs["auto"]
    P = abi.kitti_params(dis_thre_unit=2.4, max_iter_num=4)
    for p in cap_pairs:
        new, old, again = both_shapes(c, lambda: c.icp_batch([p], P))
        assert new == again
        assert new == old


@pytest.mark.parametrize("what", ["undistort", "keep_less", "mixed_tier"])
def test_paths_that_keep_the_former_shape(ctxs, edge_pairs, cap_pairs, what):
    """motion undistortion (k_clone_src regenerates the clouds), keep_less_source_points (needs the cropped copies) and a target class beyond 9728 points
    (no fused target setup for that cloud): unchanged results whether or not the switch is set"""
    rng = np.random.default_rng(47)
    c = ctxs["auto"]
    plist = [edge_pairs[1], cap_pairs[0], cap_pairs[1]]
    if what == "undistort":
        P = abi.kitti_params(dis_thre_unit=2.4, max_iter_num=3, apply_motion_undistortion=1)
    elif what == "keep_less":
        P = abi.kitti_params(dis_thre_unit=2.4, max_iter_num=3, keep_less_source_points=1)
    else:
        P = abi.kitti_params(dis_thre_unit=2.4, max_iter_num=3)
        plist = plist + [pair_of(rng, (12000, 500, 3000, 100, 9729, 0), (700, 300, 800, 50, 150, 0))]
    new, old, again = both_shapes(c, lambda: c.icp_batch(plist, P))
    assert new == again
    assert new == old


@pytest.mark.parametrize("n_src,n_tgt", [(SRC_CAP, 2048), (SRC_CAP + 1, 2049)])
def test_stage_entry_at_the_edges(ctxs, n_src, n_tgt):
    """mulls_stage_transform + mulls_stage_correspond (the stage entry points share the setup's launch sequence) against the oracle, the source on
    k_src_setup's capacity edge and the target on a bucket edge, in both shapes"""
    rng = np.random.default_rng(53)
    T = synth.se3(0.2, -0.1, 0.05, 0.0, 0.0, 0.01)
    tgt = cloud(rng, abi.GROUND, n_tgt)
    src0 = cloud(rng, abi.GROUND, n_src)
    want = pyoracle.transform(src0, T)
    m0, d0, f0 = pyoracle.correspond(want, tgt, 1.0, True, 20.0, nn_mode=1)
    assert (f0 & 2).sum() > 10
    for c in ctxs.values():
        try:
            for stop in (0, 30):
                c.set_option(abi.OPT_DEBUG_STOP, stop)
                src = c.transform(src0, T)
                for k in abi.POINT_DTYPE.names:
                    assert np.array_equal(src[k].view(np.uint32), want[k].view(np.uint32)), k
                m1, d1, f1 = c.correspond(src, tgt, 1.0, True, 20.0)
                assert np.array_equal(m0, m1)
                assert np.array_equal(d0[m0 >= 0].view(np.uint32), d1[m0 >= 0].view(np.uint32))
                assert np.array_equal(f0, f1)
        finally:
            c.set_option(abi.OPT_DEBUG_STOP, 0)
