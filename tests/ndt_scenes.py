"""The scenes of the NDT tests (tests/test_ndt.py, tests/test_gpu_ndt.py) and of the fixture tests/golden/ndt_cases.npz: small enough for the numpy
restatement, chosen on the CPU so that together they take every path the issue lists (tests/test_ndt.py::test_cases_cover_the_paths asserts which case
takes which).  A case: dict(tgt, src (n, 3) float32, tgt_bound, src_bound (6,), guess (4, 4), prm: overrides of the default parameters)."""
import numpy as np

from mulls_amd import synth


def bound_of(P, pad=0.0):
    P = np.asarray(P, np.float64)
    return np.concatenate([P.min(axis=0) - pad, P.max(axis=0) + pad])


def street(seed, n_tgt, n_src, motion, n_az=(260, 140)):
    """two scans of one synthetic street: the target at the origin, the source after `motion` (tx, ty, yaw in degrees); -> tgt, src, T_gt"""
    sc = synth.Scene(seed)
    A = synth.raycast(sc, synth.se3(0, 0, sc.sensor_height), n_beams=16, n_az=n_az[0], seed=seed + 1)["xyz"]
    pose = synth.se3(motion[0], motion[1], sc.sensor_height, yaw=np.deg2rad(motion[2]))
    B = synth.raycast(sc, pose, n_beams=16, n_az=n_az[1], seed=seed + 2)["xyz"]
    rng = np.random.default_rng(seed)
    A = A[np.sort(rng.choice(len(A), min(n_tgt, len(A)), replace=False))]
    B = B[np.sort(rng.choice(len(B), min(n_src, len(B)), replace=False))]
    return A, B, np.linalg.inv(synth.se3(0, 0, sc.sensor_height)) @ pose


def crafted():
    """a target of hand-made leaves (1 m cells, coordinates on a 1/8 grid so that every sum is exact) next to a patch of generic ones, and a source
    with points in and around them and beyond the grid on every side"""
    rng = np.random.default_rng(11)
    g = lambda n, k: rng.integers(1, 8, (n, k)).astype(np.float64) / 8.0
    parts = []
    planar = np.concatenate([g(8, 2), np.full((8, 1), 0.5)], axis=1) + [2.0, 2.0, 0.0]  # cell (2, 2, 0): z constant, 8 points
    planar[:4, 0], planar[:4, 1] = [2.125, 2.875, 2.125, 2.875], [2.125, 2.125, 2.875, 2.875]
    linear = np.concatenate([np.arange(8)[:, None] / 8.0 + 0.0625, np.full((8, 2), 0.5)], axis=1) + [4.0, 2.0, 0.0]  # cell (4, 2, 0): a line along x
    same = np.tile([[6.5, 2.5, 0.5]], (6, 1))  # cell (6, 2, 0): six identical points
    five = rng.uniform(0.1, 0.9, (5, 3)) + [2.0, 4.0, 0.0]  # cell (2, 4, 0): 5 points
    six = rng.uniform(0.1, 0.9, (6, 3)) + [4.0, 4.0, 0.0]  # cell (4, 4, 0): 6 points
    parts += [planar, linear, same, five, six]
    for cx in range(0, 9):  # generic leaves: a rough floor at z in (-1, 0) and a wall at y in (6, 7)
        for cy in range(0, 6):
            parts.append(rng.uniform(0.05, 0.95, (7, 3)) * [1, 1, 0.3] + [cx, cy, -1.0])
        parts.append(rng.uniform(0.05, 0.95, (9, 3)) * [1, 0.3, 1] + [cx, 6.0, 0.0])
    tgt = np.concatenate(parts).astype(np.float32)
    tgt = tgt[rng.permutation(len(tgt))]
    inside = rng.uniform([0, 0, -1], [9, 7, 1], (150, 3))
    near = np.concatenate([p + rng.normal(0, 0.1, p.shape) for p in (planar, linear, same, five, six)])
    beyond = np.array([[-3.0, 3, 0], [12.5, 3, 0], [4, -3.5, 0], [4, 10.5, 0], [4, 3, -4.5], [4, 3, 4.5], [-2.5, -2.5, -2.5], [11.5, 9.5, 3.5]])
    src = np.concatenate([inside, near, beyond]).astype(np.float32)
    src = (src.astype(np.float64) + [0.04, -0.03, 0.02]).astype(np.float32)
    return tgt, src


def sparse_target(seed=5, n=500):
    """no cell holds six points"""
    rng = np.random.default_rng(seed)
    return rng.uniform([-60, -60, -5], [60, 60, 15], (n, 3)).astype(np.float32)


def build_cases():
    cases = {}
    eye = np.eye(4)

    def add(name, tgt, src, guess=eye, tgt_bound=None, src_bound=None, **prm):
        cases[name] = dict(tgt=np.ascontiguousarray(tgt, np.float32), src=np.ascontiguousarray(src, np.float32),
                           tgt_bound=bound_of(tgt) if tgt_bound is None else np.asarray(tgt_bound, np.float64),
                           src_bound=bound_of(src) if src_bound is None else np.asarray(src_bound, np.float64), guess=np.asarray(guess, np.float64), prm=prm)

    A, B, T_gt = street(3, 1500, 400, (0.3, 0.05, 3.0))
    add("street", A, B)
    add("street_inner", A, B, transformation_epsilon=0.2)  # step_min = step_max: the inner loop of the line search runs
    add("street_max_iter", A, B, transformation_epsilon=0.002, max_iterations=2)
    add("street_direct1", A, B, search_method=3)
    add("street_direct26", A, B, search_method=1)
    add("street_2m", A, B, resolution=2.0)
    add("street_no_crop", A, B, apply_intersection_filter=0)
    G = synth.se3(0.25, 0.02, 0.0, yaw=np.deg2rad(2.5))
    add("street_guess", A, B, guess=G)
    near = eye.copy()
    near[0, 1], near[1, 0], near[0, 3], near[2, 2] = 4e-7, -4e-7, 9e-7, 1.0 + 5e-7
    add("street_near_identity", A, B, guess=near)
    A2, B2, _ = street(8, 3000, 1200, (0.2, -0.1, -2.0), n_az=(420, 260))
    add("street_large", A2, B2, transformation_epsilon=0.01)
    add("street_tight", A, B, guess=T_gt)  # starts at the truth
    ct, cs = crafted()
    wide = np.array([-100.0, -100, -100, 100, 100, 100])
    add("crafted", ct, cs, tgt_bound=wide, src_bound=wide)
    add("crafted_26", ct, cs, tgt_bound=wide, src_bound=wide, search_method=1)
    sp = sparse_target()
    add("no_leaves", sp, B[:64], guess=G, apply_intersection_filter=0)
    return cases, T_gt
