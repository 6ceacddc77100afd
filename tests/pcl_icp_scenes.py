"""The scenes of the classical-ICP tests (tests/test_pcl_icp.py, tests/test_gpu_pcl_icp.py) and of the fixture tests/golden/pcl_icp_cases.npz: small
enough for the numpy restatement, chosen on the CPU so that together they take every path the definition has
(tests/test_pcl_icp.py::test_cases_cover_the_paths asserts which case takes which).  A case: dict(tgt, src (n, 3) float32, tgt_bound, src_bound (6,),
guess (4, 4), prm: overrides of the default parameters)."""
import numpy as np

from mulls_amd import synth
from ndt_scenes import bound_of, street

P2P, P2PL = 0, 1
EDGE_T = 1.5 * (1.0 + 2.0 ** -20)  # the cells' edges at the default distances: both are floats
EDGE_R = 2.0 * (1.0 + 2.0 ** -20)
TILE = 256  # MULLS_PCL_ICP_TILE


def crafted():
    """coordinates on a 1/8 grid (every d2 is exact), except the points put on cell faces: ties in (d2, index) from both sides, identical points, points
    on faces of both cell sizes on both sides of 0, a pair at exactly the distance, source points sharing a target point, neighbourhoods of exactly 2
    and exactly 3 points, a neighbour at exactly the radius, a collinear neighbourhood, a planar patch through z = 0 (n . p = 0) that is denser than a
    tile of the normals kernel, a generic slab"""
    rng = np.random.default_rng(23)
    slab = np.concatenate([rng.integers(-40, 40, (220, 2)), rng.integers(-6, 7, (220, 1))], axis=1).astype(np.float64) / 8.0 + [0.0, -9.0, -1.0]
    dense = np.array([[4.0 + i / 8.0, 4.0 + j / 8.0, 0.0] for i in range(20) for j in range(20)])  # 400 points within 2.375 m: > TILE neighbours
    line = np.array([[-6.0 + 0.25 * i, 6.0, 1.0] for i in range(17)])
    same = np.tile([[-3.5, 2.5, 0.5]], (6, 1))
    pair2 = np.array([[20.0, 20.0, 5.0], [21.0, 20.0, 5.0]])  # two neighbours each
    trio = np.array([[30.0, 0.0, 0.0], [32.0, 0.0, 0.0], [31.0, 0.5, 0.0]])  # (30, 0, 0) and (32, 0, 0) are 2 m apart: three neighbours each
    faces = np.array([[s * k * e, y, 2.0] for e, y in ((EDGE_T, 1.0), (EDGE_R, -1.0)) for s in (-1.0, 1.0) for k in (1.0, 2.0)])
    ties = np.array([[0.0, 0.0, 3.0], [1.0, 0.0, 3.0], [10.0, 0.0, 0.0], [-10.0, -10.0, 2.0], [-14.0, -10.0, 2.0]])
    tgt = np.concatenate([slab, dense, line, same, pair2, trio, faces, ties])
    tgt = tgt[rng.permutation(len(tgt))].astype(np.float32)
    src = np.concatenate([
        slab[::2] + [0.125, -0.125, 0.125], dense[::7] + [0.0, 0.0, 0.125], line[::3] + [0.0, 0.125, 0.0], same[:3] + [0.125, 0.0, 0.0], same[:2] + [0.125, 0.0, 0.0],
        faces + [0.0, 0.0, 0.25],
        [[0.5, 0.0, 3.25]],  # as far from (0, 0, 3) as from (1, 0, 3): the lower target index wins
        [[11.5, 0.0, 0.0]],  # exactly 1.5 m from (10, 0, 0): kept
        [[-10.5, -10.0, 2.0], [-9.5, -10.0, 2.0]],  # as far from (-10, -10, 2) on both sides: reciprocity keeps the lower source index
        [[-14.25, -10.0, 2.0], [-14.5, -10.0, 2.0]],  # reciprocity keeps the closer
        trio[:1] + [0.25, 0.0, 0.25]])
    src = src[rng.permutation(len(src))].astype(np.float32)
    return tgt, src


def plane_target():
    """every target point on z = 0: all normals parallel, so the point-to-plane system is singular"""
    g = np.arange(-3.0, 3.01, 0.5)
    tgt = np.array([[x, y, 0.0] for x in g for y in g], np.float32)
    src = (tgt[::3].astype(np.float64) + [0.125, 0.0, 0.25]).astype(np.float32)
    return tgt, src


def late_loss():
    """three source points paired with one target point; the first step moves their centroid onto it and one of them beyond the distance"""
    tgt = np.array([[0.0, 0.0, 0.0], [50.0, 0.0, 0.0], [0.0, 50.0, 0.0], [50.0, 50.0, 5.0]], np.float32)
    src = np.array([[1.375, 0.0, 0.0], [1.375, 0.125, 0.0], [-1.0, 0.0, 0.0]], np.float32)
    return tgt, src


def build_cases():
    cases = {}
    eye = np.eye(4)

    def add(name, tgt, src, guess=eye, tgt_bound=None, src_bound=None, **prm):
        cases[name] = dict(tgt=np.ascontiguousarray(tgt, np.float32), src=np.ascontiguousarray(src, np.float32),
                           tgt_bound=bound_of(tgt) if tgt_bound is None else np.asarray(tgt_bound, np.float64),
                           src_bound=bound_of(src) if src_bound is None else np.asarray(src_bound, np.float64), guess=np.asarray(guess, np.float64), prm=prm)

    A, B, T_gt = street(3, 1500, 400, (0.3, 0.05, 3.0))
    A, B = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(B, np.float32)
    add("street", A, B)
    add("street_recip", A, B, use_reciprocal_correspondence=1)
    add("street_plane", A, B, metrics=P2PL, te=2)
    add("street_plane_recip", A, B, metrics=P2PL, use_reciprocal_correspondence=1)
    add("street_max_iter", A, B, max_iter_num=3)
    add("street_rel_mse", A, B, euclidean_fitness_epsilon=1e-2)
    add("street_plane_rel_mse", A, B, metrics=P2PL, euclidean_fitness_epsilon=1e-2)
    G = synth.se3(0.25, 0.02, 0.0, yaw=np.deg2rad(2.5))
    add("street_guess", A, B, guess=G)
    near = eye.copy()
    near[0, 1], near[1, 0], near[0, 3], near[2, 2] = 4e-7, -4e-7, 9e-7, 1.0 + 5e-7
    add("street_near_identity", A, B, guess=near)
    add("street_no_crop", A, B, apply_intersection_filter=0)
    add("street_tight", A, B, guess=T_gt)  # starts at the truth
    A2, B2, _ = street(8, 3000, 4500, (0.2, -0.1, -2.0), n_az=(420, 900))  # more than MULLS_NDT_TREE source points
    add("street_large", A2, B2, metrics=P2PL, use_reciprocal_correspondence=1)
    add("lifted", A, B[:64] + np.float32([0.0, 0.0, 300.0]), apply_intersection_filter=0)  # no pair at iteration 0
    add("empty", A, B[:64] + np.float32([500.0, 0.0, 0.0]))  # nothing left after the crop
    sub = (A[::4].astype(np.float64) @ np.linalg.inv(synth.se3(0.05, 0.02, 0.0, yaw=np.deg2rad(0.3)))[:3, :3].T
           + np.linalg.inv(synth.se3(0.05, 0.02, 0.0, yaw=np.deg2rad(0.3)))[:3, 3]).astype(np.float32)
    add("exact_subset", A, sub)
    add("abs_mse", A, sub, transformation_epsilon=0.0, euclidean_fitness_epsilon=0.0, max_iter_num=30)  # neither TRANSFORM nor REL_MSE can fire
    ct, cs = crafted()
    add("crafted", ct, cs, use_reciprocal_correspondence=1, apply_intersection_filter=0)
    add("crafted_one_way", ct, cs, apply_intersection_filter=0)
    add("crafted_plane", ct, cs, metrics=P2PL, use_reciprocal_correspondence=1, apply_intersection_filter=0)
    pt, ps = plane_target()
    add("singular", pt, ps, metrics=P2PL, apply_intersection_filter=0)
    lt, ls = late_loss()
    add("late_loss", lt, ls, apply_intersection_filter=0)
    three = (A[[10, 500, 900]].astype(np.float64) + [0.125, 0.0625, 0.03125]).astype(np.float32)
    add("three_pairs", A, three, apply_intersection_filter=0)
    add("two_pairs", A, three[:2], apply_intersection_filter=0)
    return cases, T_gt
