"""The scenes of the FPFH / SAC-IA tests (tests/test_fpfh.py, tests/test_gpu_fpfh.py) and of the fixture tests/golden/fpfh_cases.npz: small enough for
the numpy restatement, each named for the edge it reaches (tests/test_fpfh.py asserts that it does).

fpfh_cases() -> name -> dict(pts, nrm (n, 3) float32, search_radius).
sac_cases() -> name -> dict(tgt, tgt_nrm, src, src_nrm, prm: overrides of the default parameters); sac_truth() -> the known motion of `sac_recovery`."""
import numpy as np

import fpfh_restated as fr
import reg_edges
from mulls_amd import synth

F32 = np.float32
SIZES = (63, 64, 65, 255, 256, 257)
EDGE = 1.0 * (1.0 + 2.0 ** -20)  # the cells' edge at search_radius = 0.5
RECOVERY_SPACING = 0.25  # metres: 1 500 points on 8 m x 8 m, (64 / 1500)^0.5 = 0.21 between neighbours on the plane, more along the slopes


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def random_normals(rng, n):
    return unit(rng.normal(size=(n, 3)))


def case(pts, nrm, search_radius=0.5):
    return dict(pts=np.ascontiguousarray(pts, F32).reshape(-1, 3), nrm=np.ascontiguousarray(nrm, F32).reshape(-1, 3), search_radius=search_radius)


def sizes():
    """six balls of 63 .. 257 points, each inside one cell and 8 m from the next (every point of a ball of m has k = m; the ball of 257 fills one cell
    with more than 256 points), and a ball of 70 centred on a cell face (its points lie in two cells); the order permuted"""
    rng = np.random.default_rng(5)
    parts = []
    for i, m in enumerate(SIZES + (70,)):
        d = rng.normal(size=(m, 3))
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.3 * rng.uniform(0, 1, (m, 1)) ** (1 / 3))
        centre = [8.0 * i + 0.5, 0.5, 0.5] if m != 70 else [56.0 * EDGE, 0.5, 0.5]
        parts.append(d + centre)
    pts = np.concatenate(parts)
    perm = rng.permutation(len(pts))
    return case(pts[perm], random_normals(rng, len(pts)))


def bin_edges():
    """isolated pairs p = (0, 0, 0) with normal (0, 0, 1) and q = (0.5, 0, 0), 10 m apart: v = (0, -1, 0), w = (1, 0, 0).  n_q = -+v: f2 = +-1; n_q =
    (0, 0, -1): f1 = +pi; n_q = (-0, -0, -1) with n_p = (-0, 0, 1): w . n_q = -0 and f1 = -pi; both normals along dp: f3 = +-1 and |v| = 0, the pair adds nothing; n_q = (0, -c, s) with c the
    float next to 2 * 3 / 11 - 1 and its two float neighbours: f2 next to the inner edge between bins 2 and 3, on both sides.  Then EXACT_EDGES: pairs
    with q = p + (0.375, 0.5, 0) (f4 = 0.625 exactly, no swap) whose normals were searched on the CPU so that a feature lies exactly on an inner edge,
    11 x == k in double: the floats' different exponents give the dot products some 50 significant bits"""
    c0 = F32(2.0 * 3.0 / 11.0 - 1.0)
    near = [np.nextafter(c0, F32(-1)), c0, np.nextafter(c0, F32(1))]
    nq = [(0, -1, 0), (0, 1, 0), (0, 0, -1), (-0.0, -0.0, -1.0), (1, 0, 0), (-1, 0, 0)] + [(0.0, -float(c), float(np.sqrt(1.0 - float(c) ** 2))) for c in near]
    np_ = [(0, 0, 1)] * 3 + [(-0.0, 0, 1)] + [(1, 0, 0), (1, 0, 0)] + [(0, 0, 1)] * 3
    pts, nrm = [], []
    for j, (a, b) in enumerate(zip(np_, nq)):
        pts += [[10.0 * j, 20.0, 0.0], [10.0 * j + 0.5, 20.0, 0.0]]
        nrm += [a, b]
    for j, (a, b, _, _) in enumerate(EXACT_EDGES):
        pts += [[10.0 * (j + len(nq)), 20.0, 0.0], [10.0 * (j + len(nq)) + 0.375, 20.5, 0.0]]
        nrm += [a, b]
    return case(pts, np.array(nrm, F32))


# (n_p, n_q, the feature: 1 is f2, 2 is f3, the edge k): the query is the first point of the pair
EXACT_EDGES = (((-0.15151516, 3.3866276e-09, 1.0), (0.0, 0.0, 1.0), 2, 5),
               ((0.0, 1.0, 1.0), (-0.6626081466674805, 3.093507316975774e-08, 1.4318117885444605e-15), 1, 3))
N_EDGE_PAIRS = 9  # the pairs of bin_edges before EXACT_EDGES


def fpfh_cases():
    rng = np.random.default_rng(3)
    out = {}
    out["one"] = case([[1.0, 2.0, 3.0]], [[0.0, 0.0, 1.0]])
    out["two"] = case([[0.0, 0.0, 0.0], [0.5, 0.25, 0.0]], random_normals(rng, 2))
    out["three"] = case([[0.0, 0.0, 0.0], [0.5, 0.25, 0.0], [50.0, 0.0, 0.0]], random_normals(rng, 3))  # the third has no neighbour: all zeros
    base = rng.uniform(0, 1.5, (12, 3))
    dup = np.concatenate([base, base[:4], base[:2], [[30.0, 0.0, 0.0]] * 3])  # copies of points (d2 = 0, f4 = 0), and three records at one isolated place
    out["duplicates"] = case(dup, random_normals(rng, len(dup)))
    pts = np.concatenate([rng.uniform(0, 1.5, (20, 3)), [[20.0, 0.0, 0.0], [20.5, 0.0, 0.0]]])
    nrm = random_normals(rng, len(pts))
    nrm[3] = nrm[11] = 0.0  # zero normals among neighbours
    nrm[20], nrm[21] = [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]  # an isolated pair: a normal along dp (|v| = 0) and a zero normal
    out["normals"] = case(pts, nrm)
    one = F32(1.0)
    pts = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, float(np.nextafter(one, F32(2))), 0.0], [0.0, 0.0, -float(np.nextafter(one, F32(0)))]]
    out["radius_edge"] = case(pts, random_normals(rng, 4))  # from the first: exactly at the radius (in), a float ulp beyond (out), a float ulp inside (in)
    out["sizes"] = sizes()
    out["bin_edges"] = bin_edges()
    dense = reg_edges.gicp_dense()[0]  # 2 000 points in 1 960 cells of 1 m: a table of 4 096 slots at a load of 0.48, long probe runs, a wrap
    out["dense_table"] = case(dense, random_normals(rng, len(dense)))
    return out


# ---- SAC-IA

def bumpy(seed, n, side):
    """n points on z = 0.6 sin(1.3 x) cos(0.9 y) + 0.3 sin(2.1 x + y) + 0.25 cos(2.7 y) over [0, side]^2, with the surface's unit normals"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    z = 0.6 * np.sin(1.3 * x) * np.cos(0.9 * y) + 0.3 * np.sin(2.1 * x + y) + 0.25 * np.cos(2.7 * y)
    zx = 0.6 * 1.3 * np.cos(1.3 * x) * np.cos(0.9 * y) + 0.3 * 2.1 * np.cos(2.1 * x + y)
    zy = -0.6 * 0.9 * np.sin(1.3 * x) * np.sin(0.9 * y) + 0.3 * np.cos(2.1 * x + y) - 0.25 * 2.7 * np.sin(2.7 * y)
    return np.stack([x, y, z], axis=1).astype(F32), unit(np.stack([-zx, -zy, np.ones(n)], axis=1))


def moved(pts, nrm, M):
    """the cloud and its normals under the rigid motion M, stored as float32"""
    return (pts.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(F32), (nrm.astype(np.float64) @ M[:3, :3].T).astype(F32)


def sac_truth():
    return synth.se3(1.5, -0.8, 0.4, yaw=np.deg2rad(25.0))


def sac(tgt, tgt_nrm, src, src_nrm, **prm):
    return dict(tgt=np.ascontiguousarray(tgt, F32), tgt_nrm=np.ascontiguousarray(tgt_nrm, F32), src=np.ascontiguousarray(src, F32),
                src_nrm=np.ascontiguousarray(src_nrm, F32), prm=prm)


def small_pair(seed=9):
    """80 target points on a 2.5 m patch; the source: 60 of them under the inverse of a small motion"""
    T, Tn = bumpy(seed, 80, 2.5)
    rng = np.random.default_rng(seed + 1)
    sel = np.sort(rng.choice(80, 60, replace=False))
    S, Sn = moved(T[sel], Tn[sel], np.linalg.inv(synth.se3(0.3, 0.1, 0.05, yaw=np.deg2rad(8.0))))
    return T, Tn, S, Sn


def threshold_case(error_function):
    """max_correspondence_distance is the float squared distance that source point 5 has under hypothesis 2: e == thr there"""
    T, Tn, S, Sn = small_pair()
    prm = dict(search_radius=0.4, max_iterations=6, seed=4, error_function=error_function)
    detail = {}
    fr.fpfhsac(T, Tn, S, Sn, fr.fpfhsac_default_params(**prm), detail)
    thr = float(detail["e"][2][5])
    assert thr > 0.0
    return sac(T, Tn, S, Sn, max_correspondence_distance=thr, **prm)


def sac_cases():
    out = {}
    T, Tn, S, Sn = small_pair()
    out["sac_default"] = sac(T, Tn, S, Sn, search_radius=0.4)  # the infinite range: hypothesis 0 wins
    out["sac_three"] = sac(T, Tn, S[:3], Sn[:3], search_radius=0.4, max_iterations=4, max_correspondence_distance=0.5)
    out["sac_few_targets"] = sac(T[:7], Tn[:7], S[:30], Sn[:30], search_radius=0.4, max_correspondence_distance=0.5)  # k_eff = 7
    grid = np.array([[3.0 * i, 3.0 * j, 0.0] for i in range(5) for j in range(4)])  # nobody has a neighbour: every descriptor is zero
    up = np.tile([[0.0, 0.0, 1.0]], (20, 1))
    out["sac_equal_descriptors"] = sac(grid, up, grid[:10] + [0.5, 0.25, 0.0], up[:10], search_radius=0.4, max_correspondence_distance=4.0, seed=2)
    out["sac_halving"] = sac(T, Tn, S[:8], Sn[:8], search_radius=0.4, min_sample_distance=1000.0, max_iterations=3, max_correspondence_distance=0.5)
    for it in (1, 64, 65):
        out["sac_it%d" % it] = sac(T, Tn, S, Sn, search_radius=0.4, max_iterations=it, max_correspondence_distance=0.25, k_correspondences=3, seed=it)
    out["sac_chunks"] = sac(T[:24], Tn[:24], S[:8], Sn[:8], search_radius=0.4, max_iterations=1030, max_correspondence_distance=0.25, k_correspondences=3,
                            seed=8)  # past the 1 024 hypotheses whose distances are held at a time
    out["sac_equal_error"] = sac(T, Tn, S, Sn, search_radius=0.4, max_iterations=8, max_correspondence_distance=1e-12, seed=3)  # every term is 1
    out["sac_threshold_truncated"] = threshold_case(fr.TRUNCATED)
    out["sac_threshold_huber"] = threshold_case(fr.HUBER)
    near = np.array([[3.0 * i, 3.0 * j, 0.0] for i in range(4) for j in range(3)])
    far = near[:6] + [1e20, 0.0, 0.0]  # a hypothesis with a pair out there leaves source points whose float d2 overflows: e = inf, e / inf = NaN
    both = np.concatenate([far[:3], near, far[3:]])
    up = np.tile([[0.0, 0.0, 1.0]], (len(both), 1))
    out["sac_nan_errors"] = sac(both, up, near[:8] + [0.5, 0.25, 0.0], up[:8], search_radius=1e16, max_iterations=12, seed=5)  # errors 0 .. 2 are NaN: 3 wins
    out["sac_huber"] = sac(T, Tn, S, Sn, search_radius=0.4, max_iterations=12, max_correspondence_distance=0.05, error_function=fr.HUBER, seed=6)
    A, An = bumpy(21, 1500, 8.0)
    rng = np.random.default_rng(22)
    sel = np.sort(rng.choice(1500, 1200, replace=False))
    B, Bn = moved(A[sel], An[sel], np.linalg.inv(sac_truth()))
    out["sac_recovery"] = sac(A, An, B, Bn, **RECOVERY)
    return out


RECOVERY = dict(search_radius=0.4, k_correspondences=2, max_iterations=120, min_sample_distance=2.0, max_correspondence_distance=0.05, seed=1)
