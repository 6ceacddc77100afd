"""The scenes of the GICP tests (tests/test_gicp.py, tests/test_gpu_gicp.py) and of the fixture tests/golden/gicp_cases.npz: small enough for the numpy
restatement, chosen on the CPU so that together they take every path the definition has (tests/test_gicp.py::test_cases_cover_the_paths asserts which
case takes which).  A case: dict(tgt, src (n, 3) float32, tgt_bound, src_bound (6,), guess (4, 4), prm: overrides of the default parameters)."""
import numpy as np

from mulls_amd import synth
from ndt_scenes import bound_of, street


def crafted():
    """coordinates on a 1/8 grid: a planar lattice around the origin with points on voxel faces (x / res - 0.5 integral) on both sides of 0 and many
    ties in (d2, index); a line (collinear neighbourhoods: two equal eigenvalues); 25 identical points (more than k: the index decides) and 3 more;
    single points far from everything (voxels of one point, neighbours past any ring walk); a generic slab"""
    rng = np.random.default_rng(17)
    ax = np.arange(-2.0, 2.01, 0.5)
    lattice = np.array([[x, y, 0.0] for x in ax for y in ax])  # 81 points: x = -1.5, -0.5, 0.5, 1.5 lie on voxel faces
    line = np.array([[4.0 + 0.125 * i, 3.5, 1.0] for i in range(33)])
    same = np.tile([[-3.5, 2.5, 0.5]], (25, 1))
    same3 = np.tile([[6.25, -2.125, 0.75]], (3, 1))
    lonely = np.array([[10.25, -4.75, 2.125], [-9.125, 6.5, -1.25], [0.5, 11.5, 3.5]])
    slab = np.concatenate([rng.integers(-32, 32, (150, 2)), rng.integers(-2, 3, (150, 1))], axis=1).astype(np.float64) / 8.0 + [0.0, -5.0, -1.0]
    tgt = np.concatenate([lattice, line, same, same3, lonely, slab])
    tgt = tgt[rng.permutation(len(tgt))].astype(np.float32)
    part = np.concatenate([lattice[::2], line[::2], same[:22], lonely[:1], slab[::2]])
    src = (part + [0.125, -0.125, 0.0]).astype(np.float32)
    src = src[rng.permutation(len(src))]
    return tgt, src


def build_cases():
    cases = {}
    eye = np.eye(4)

    def add(name, tgt, src, guess=eye, tgt_bound=None, src_bound=None, **prm):
        cases[name] = dict(tgt=np.ascontiguousarray(tgt, np.float32), src=np.ascontiguousarray(src, np.float32),
                           tgt_bound=bound_of(tgt) if tgt_bound is None else np.asarray(tgt_bound, np.float64),
                           src_bound=bound_of(src) if src_bound is None else np.asarray(src_bound, np.float64), guess=np.asarray(guess, np.float64), prm=prm)

    A, B, T_gt = street(3, 1500, 400, (0.3, 0.05, 3.0))
    add("street", A, B)
    G = synth.se3(0.25, 0.02, 0.0, yaw=np.deg2rad(2.5))
    add("street_guess", A, B, guess=G)
    near = eye.copy()
    near[0, 1], near[1, 0], near[0, 3], near[2, 2] = 4e-7, -4e-7, 9e-7, 1.0 + 5e-7
    add("street_near_identity", A, B, guess=near)
    add("street_crop", A, B, apply_intersection_filter=1)
    add("street_2m", A, B, voxel_resolution=2.0)
    add("street_half", A, B, voxel_resolution=0.5)
    add("street_k5", A, B, k_correspondences=5)
    add("street_k32", A, B, k_correspondences=32)
    add("street_max_iter", A, B, max_iterations=3)
    add("street_tight", A, B, guess=T_gt)  # starts at the truth
    A2, B2, _ = street(8, 3000, 1200, (0.2, -0.1, -2.0), n_az=(420, 260))
    add("street_large", A2, B2)
    ct, cs = crafted()
    add("crafted", ct, cs)
    add("exact_k", A, B[:20])
    add("k_plus_1", A, B[:21])
    # 19 source points inside the target's box, the others 500 m away: the crop leaves 19
    far = np.concatenate([B[:19], B[19:60] + np.float32([500.0, 0.0, 0.0])]).astype(np.float32)
    add("too_few", A, far, guess=G, apply_intersection_filter=1)
    # the source 300 m above every voxel; the loop starts from r = 0, so the pose it keeps is the guess
    add("no_overlap", A, B[:64] + np.float32([0.0, 0.0, 300.0]), guess=G, start_rotvec=[0.0, 0.0, 0.0])
    rng = np.random.default_rng(5)
    out_t = np.array([[80.0, 70.0, 40.0], [-85.0, 60.0, 35.0], [75.0, -90.0, 50.0], [-70.0, -75.0, 45.0]]) + rng.uniform(-1, 1, (4, 3))
    out_s = np.array([[82.0, -66.0, 38.0], [-77.0, 71.0, 42.0], [64.0, 88.0, 55.0]]) + rng.uniform(-1, 1, (3, 3))
    add("outliers", np.concatenate([A, out_t]), np.concatenate([B, out_s]))
    return cases, T_gt
