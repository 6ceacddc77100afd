"""mulls_gicp restated in numpy from reading upstream (cregistration.hpp:1024-1098 and :788-815, baseline_reg/fast_vgicp_impl.hpp, fast_vgicp_voxel.h,
fast_gicp_utility.h as omp_gicp configures them) and the definition in include/mulls_hip.h: double arithmetic in the stated orders, float where the
definition says float, sin / atan2 correctly rounded through mpmath (memoised), brute-force neighbours.  Nothing here was compared with fast_gicp,
Sophus, Eigen or PCL themselves: none is a dependency of this repository.  This module is the yardstick of tests/test_gicp.py and of the fixture
tests/golden/gicp_cases.npz (tests/golden/make_gicp_golden.py), which tests/test_gpu_gicp.py compares the device with."""
import math

import mpmath
import numpy as np

import ndt_restated as nr
from ndt_restated import DBL_MAX, _rot, crop, sin_cr, tree_sum  # noqa: F401

STOP_NONE, STOP_CONVERGED, STOP_MAX_ITERATIONS, STOP_SINGULAR = range(4)
START = float(np.float32(0.005773503))


def atan2_cr(y, x):
    key = ("atan2", y, x)
    v = nr._memo.get(key)
    if v is None:
        with mpmath.workprec(240):
            v = nr._memo[key] = float(mpmath.atan2(mpmath.mpf(y), mpmath.mpf(x)))
    return v


def default_params(**kw):
    p = dict(voxel_resolution=1.0, k_correspondences=20, max_iterations=64, rotation_epsilon=2e-3, transformation_epsilon=5e-4, apply_intersection_filter=0,
             fitness_score_thre=10.0, using_voxel_gicp=1, start_rotvec=[START] * 3)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


# ---- a point's covariance

def neighbours(P, k):
    """(n, 3) float32 -> (n, k) indices: smallest by (float squared distance ((dx dx + dy dy) + dz dz), index)"""
    P = np.ascontiguousarray(P, np.float32)
    out = np.empty((len(P), k), np.int64)
    idx = np.arange(len(P))
    for i in range(len(P)):
        d = P - P[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out[i] = np.lexsort((idx, d2))[:k]
    return out


def plane_covariance(S):
    """S: scatter, xx xy xz yy yz zz -> C likewise"""
    A = {(0, 0): float(S[0]), (0, 1): float(S[1]), (0, 2): float(S[2]), (1, 1): float(S[3]), (1, 2): float(S[4]), (2, 2): float(S[5])}
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(60):
        off = A[(0, 1)] * A[(0, 1)] + A[(0, 2)] * A[(0, 2)] + A[(1, 2)] * A[(1, 2)]
        if not off >= 1e-300:
            break
        _rot(A, V, 0, 1, 2)
        _rot(A, V, 0, 2, 1)
        _rot(A, V, 1, 2, 0)
    e = [A[(0, 0)], A[(1, 1)], A[(2, 2)]]
    order = sorted(range(3), key=lambda c: (-e[c], c))  # descending, ties by column index ascending
    v = [[V[0][c], V[1][c], V[2][c]] for c in order]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    return [(v[0][a] * v[0][b] + v[1][a] * v[1][b]) + 0.01 * (v[2][a] * v[2][b]) for a, b in pairs], [e[c] for c in order]


def point_covariance(Q):
    """Q: (k, 3) the neighbours in their order -> 6 doubles"""
    Q = [[float(v) for v in row] for row in np.asarray(Q, np.float64)]
    k = len(Q)
    s = [0.0, 0.0, 0.0]
    for q in Q:
        s[0] += q[0]
        s[1] += q[1]
        s[2] += q[2]
    m = [s[0] / float(k), s[1] / float(k), s[2] / float(k)]
    S = [0.0] * 6
    for q in Q:
        d = [q[0] - m[0], q[1] - m[1], q[2] - m[2]]
        S[0] += d[0] * d[0]
        S[1] += d[0] * d[1]
        S[2] += d[0] * d[2]
        S[3] += d[1] * d[1]
        S[4] += d[1] * d[2]
        S[5] += d[2] * d[2]
    return plane_covariance(S)[0]


def covariances(P, k):
    P = np.ascontiguousarray(P, np.float32)
    nb = neighbours(P, k)
    return np.array([point_covariance(P[nb[i]]) for i in range(len(P))], np.float64).reshape(len(P), 6)


# ---- the voxel map

def voxel_coords(P, resolution):
    """(n, 3) float32 -> (n, 3) int64 and ok (n,): floor(x / resolution - 0.5) in float, inside [-2^20, 2^20)"""
    with np.errstate(all="ignore"):
        q = np.floor(np.asarray(P, np.float32) / np.float32(resolution) - np.float32(0.5))
    ok = ((q >= -1048576.0) & (q < 1048576.0)).all(axis=1)
    return np.where(ok[:, None], q, 0).astype(np.int64), ok


def knn_coords(P, edge):
    """the cells of the neighbour search, of the voxels' edge: (n, 3) float32 -> (n, 3) int64 and ok (n,): floor(x (1 / edge)) in double, inside
    [-2^20, 2^20).  The last accepted coordinate is not voxel_coords': at 1 m, x = -1048576 and x = 1048575.875 here, -1048575.5 and 1048576.25 there."""
    q = np.floor(np.asarray(P, np.float32).astype(np.float64) * (1.0 / float(np.float32(edge))))
    ok = ((q >= -1048576.0) & (q < 1048576.0)).all(axis=1)
    return np.where(ok[:, None], q, 0).astype(np.int64), ok


def pack(c):
    return (int(c[0]) + 1048576) | ((int(c[1]) + 1048576) << 21) | ((int(c[2]) + 1048576) << 42)


def table_log2(n_tgt):
    """the library's table: a power of two >= max(2 n_tgt, 1024)"""
    lg = 10
    while (1 << lg) < 2 * n_tgt:
        lg += 1
    return lg


def home_slot(key, lg):
    m = 2 ** 64 - 1
    z = key
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z = z ^ (z >> 31)
    return z >> (64 - lg)


class VoxelMap:
    pass


def build_voxels(tgt, C, resolution):
    """None when a coordinate is outside the key's range"""
    coords, ok = voxel_coords(tgt, resolution)
    if not ok.all():
        return None
    vm = VoxelMap()
    vm.index, means, covs, ns = {}, [], [], []
    groups = {}
    for i, c in enumerate(coords):
        groups.setdefault(pack(c), []).append(i)  # ascending point index
    t64 = tgt.astype(np.float64)
    for key, grp in groups.items():
        s, q = [0.0] * 3, [0.0] * 6
        for i in grp:
            for a in range(3):
                s[a] += float(t64[i, a])
            for a in range(6):
                q[a] += float(C[i, a])
        n = float(len(grp))
        vm.index[key] = len(means)
        means.append([v / n for v in s])
        covs.append([v / n for v in q])
        ns.append(len(grp))
    vm.mean, vm.cov, vm.n = np.array(means, np.float64), np.array(covs, np.float64), np.array(ns, np.int64)
    vm.n_voxels, vm.resolution = len(means), np.float32(resolution)
    return vm


# ---- rotations

def so3_exp(w):
    w = [float(v) for v in w]
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if th == 0.0:
        return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    a = sin_cr(th) / th
    s = sin_cr(th / 2.0)
    b = ((2.0 * s) * s) / (th * th)
    K = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    K2 = [-(w[1] * w[1] + w[2] * w[2]), w[0] * w[1], w[0] * w[2], w[0] * w[1], -(w[0] * w[0] + w[2] * w[2]), w[1] * w[2],
          w[0] * w[2], w[1] * w[2], -(w[0] * w[0] + w[1] * w[1])]
    return [((1.0 if k % 4 == 0 else 0.0) + a * K[k]) + b * K2[k] for k in range(9)]


def so3_log(R):
    w0, w1, w2 = (R[7] - R[5]) / 2.0, (R[2] - R[6]) / 2.0, (R[3] - R[1]) / 2.0
    c = (((R[0] + R[4]) + R[8]) - 1.0) / 2.0
    n = math.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    if n == 0.0:
        return [0.0, 0.0, 0.0]
    f = atan2_cr(n, c) / n
    return [w0 * f, w1 * f, w2 * f]


def mat3_mul(A, B):
    return [_dot3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]) for i in range(3) for j in range(3)]


# ---- an evaluation

def move(R, t, src):
    """(n, 3) float32 -> (n, 3) float64: ((R_r0 x + R_r1 y) + R_r2 z) + t_r"""
    x = src.astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([((R[3 * r] * x[:, 0] + R[3 * r + 1] * x[:, 1]) + R[3 * r + 2] * x[:, 2]) + t[r] for r in range(3)], axis=1)


def point_terms(ap, CA, mean, CB, R):
    """(m, 3), (m, 6), (m, 3), (m, 6) -> (m, 28): the upper triangle of J^T J, J^T e, e . e"""
    m = len(ap)
    out = np.zeros((m, 28))
    if m == 0:
        return out
    with np.errstate(all="ignore"):
        c = [[CA[:, 0], CA[:, 1], CA[:, 2]], [CA[:, 1], CA[:, 3], CA[:, 4]], [CA[:, 2], CA[:, 4], CA[:, 5]]]
        RC = [[_dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], c[0][j], c[1][j], c[2][j]) for j in range(3)] for i in range(3)]
        M = lambda i, j, b: CB[:, b] + _dot3(RC[i][0], RC[i][1], RC[i][2], R[3 * j], R[3 * j + 1], R[3 * j + 2])
        c00, c01, c02, c11, c12, c22 = M(0, 0, 0), M(0, 1, 1), M(0, 2, 2), M(1, 1, 3), M(1, 2, 4), M(2, 2, 5)
        k00, k01, k02 = c11 * c22 - c12 * c12, c02 * c12 - c01 * c22, c01 * c12 - c02 * c11
        k11, k12, k22 = c00 * c22 - c02 * c02, c01 * c02 - c00 * c12, c00 * c11 - c01 * c01
        det = (c00 * k00 + c01 * k01) + c02 * k02
        W = [[k00 / det, k01 / det, k02 / det], [k01 / det, k11 / det, k12 / det], [k02 / det, k12 / det, k22 / det]]
        d = [mean[:, a] - ap[:, a] for a in range(3)]
        e, J = [], []
        for i in range(3):
            e.append(_dot3(W[i][0], W[i][1], W[i][2], d[0], d[1], d[2]))
            J.append([W[i][1] * ap[:, 2] - W[i][2] * ap[:, 1], W[i][2] * ap[:, 0] - W[i][0] * ap[:, 2], W[i][0] * ap[:, 1] - W[i][1] * ap[:, 0],
                      -W[i][0], -W[i][1], -W[i][2]])
        at = 0
        for i in range(6):
            for k in range(i, 6):
                out[:, at] = _dot3(J[0][i], J[1][i], J[2][i], J[0][k], J[1][k], J[2][k])
                at += 1
        for i in range(6):
            out[:, 21 + i] = _dot3(J[0][i], J[1][i], J[2][i], e[0], e[1], e[2])
        out[:, 27] = _dot3(e[0], e[1], e[2], e[0], e[1], e[2])
    return out


def evaluate(src, C_src, vm, R, t, per_point_out=None):
    """-> the 28 sums, n_corr; per_point_out, a list, receives the (n, 28) terms the sums are taken over"""
    ap = move(R, t, src)
    with np.errstate(all="ignore"):
        coords, ok = voxel_coords(ap.astype(np.float32), vm.resolution)
    vox = np.array([vm.index.get(pack(c), -1) if o else -1 for c, o in zip(coords, ok)], np.int64)
    sel = np.flatnonzero(vox >= 0)
    per_point = np.zeros((len(src), 28))
    per_point[sel] = point_terms(ap[sel], C_src[sel], vm.mean[vox[sel]], vm.cov[vox[sel]], R)
    if per_point_out is not None:
        per_point_out.append(per_point)
    return tree_sum(per_point), len(sel)


# ---- the step

def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(v):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(v)))


def solve_step(Hu, b):
    """-> delta (6), ok"""
    L = [[0.0] * 6 for _ in range(6)]
    at = 0
    for i in range(6):
        for k in range(i, 6):
            L[k][i] = float(Hu[at])
            if k != i:
                L[i][k] = 0.0
            at += 1
    ok = True
    for j in range(6):
        s = L[j][j]
        for k in range(j):
            s -= L[j][k] * L[j][k]
        if not s > 0.0 or not math.isfinite(s):
            ok = False
        piv = _sqrt(s)
        L[j][j] = piv
        for i in range(j + 1, 6):
            v = L[i][j]
            for k in range(j):
                v -= L[i][k] * L[j][k]
            L[i][j] = _div(v, piv)
    y = [0.0] * 6
    for i in range(6):
        v = float(b[i])
        for k in range(i):
            v -= L[i][k] * y[k]
        y[i] = _div(v, L[i][i])
    delta = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k][i] * delta[k]
        delta[i] = _div(v, L[i][i])
    if not all(math.isfinite(v) for v in delta):
        ok = False
    return delta, ok


class State:
    def __init__(self, start):
        self.r, self.t = [float(np.float32(v)) for v in start], [0.0, 0.0, 0.0]
        self.R = so3_exp(self.r)
        self.loss, self.n_corr, self.iterations, self.converged, self.stop, self.running = 0.0, 0, 0, 0, STOP_NONE, 1


def advance(S, sums, n_corr, max_iterations, rotation_epsilon, transformation_epsilon):
    sums = [float(v) for v in sums]
    S.loss, S.n_corr = sums[27], int(n_corr)
    delta, ok = ([0.0] * 6, False) if not n_corr else solve_step(sums[:21], sums[21:27])
    if not ok:
        S.stop, S.running = STOP_SINGULAR, 0
        return
    E = so3_exp([-delta[0], -delta[1], -delta[2]])
    S.r = so3_log(mat3_mul(E, S.R))
    S.R = so3_exp(S.r)
    for k in range(3):
        S.t[k] -= delta[3 + k]
    E = so3_exp(delta[:3])
    mr = max(abs(E[k] - (1.0 if k % 4 == 0 else 0.0)) for k in range(9))
    mt = max(abs(delta[3 + k]) for k in range(3))
    qr, qt = mr / rotation_epsilon, mt / transformation_epsilon
    if (qr if qr > qt else qt) < 1.0:
        S.converged, S.stop, S.running = 1, STOP_CONVERGED, 0
        return
    if S.iterations + 1 >= max_iterations:
        S.stop, S.running = STOP_MAX_ITERATIONS, 0
        return
    S.iterations += 1


# ---- the whole call

def fitness_of(src, tgt, R, t):
    xp = move(R, t, src).astype(np.float32)
    d2 = np.empty(len(xp), np.float32)
    for b in range(0, len(xp), 256):
        d = xp[b:b + 256, None, :] - tgt[None, :, :]
        d2[b:b + 256] = ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).min(axis=1)
    return float(tree_sum(d2.astype(np.float64))) / float(len(xp))


def gicp(tgt, src, tgt_bound, src_bound, guess, prm=None, trace=None):
    """-> dict of mulls_gicp_result's fields (T row-major (4, 4)); None when a coordinate is outside the voxel key's range"""
    prm = prm or default_params()
    assert prm["using_voxel_gicp"]
    G = np.asarray(guess, np.float64).reshape(4, 4)
    k = prm["k_correspondences"]
    tgt_c, src_c, apply_guess = crop(tgt, src, tgt_bound, src_bound, G, prm["apply_intersection_filter"])
    res = dict(code=-3, iterations=0, converged=0, stop=STOP_NONE, n_src=len(src_c), n_tgt=len(tgt_c), n_voxels=0, n_corr=0,
               T=G.copy() if apply_guess else np.eye(4), fitness=DBL_MAX, loss=0.0)
    if len(src_c) < k or len(tgt_c) < k:
        return res
    # the refusal: a target point outside the voxel map's range, or a point of either cloud outside the range of the neighbour search's cells
    _, ok_v = voxel_coords(tgt_c, prm["voxel_resolution"])
    _, ok_t = knn_coords(tgt_c, prm["voxel_resolution"])
    _, ok_s = knn_coords(src_c, prm["voxel_resolution"])
    if not ok_v.all() or not ok_t.all() or not ok_s.all():
        return None
    C_src, C_tgt = covariances(src_c, k), covariances(tgt_c, k)
    vm = build_voxels(tgt_c, C_tgt, prm["voxel_resolution"])
    S = State(prm["start_rotvec"])
    for _ in range(prm["max_iterations"]):
        sums, n_corr = evaluate(src_c, C_src, vm, S.R, S.t)
        if trace is not None:
            trace.append((list(S.r), list(S.t), list(S.R), sums.copy(), n_corr))
        advance(S, sums, n_corr, prm["max_iterations"], prm["rotation_epsilon"], prm["transformation_epsilon"])
        if not S.running:
            break
    Tn = np.eye(4)
    Tn[:3, :3] = np.array(S.R).reshape(3, 3)
    Tn[:3, 3] = S.t
    if apply_guess:
        T = np.empty((4, 4))
        for r in range(4):
            for c in range(4):
                T[r, c] = ((Tn[r, 0] * G[0, c] + Tn[r, 1] * G[1, c]) + Tn[r, 2] * G[2, c]) + Tn[r, 3] * G[3, c]
    else:
        T = Tn
    fit = fitness_of(src_c, tgt_c, S.R, S.t)
    res.update(code=-3 if fit > float(np.float32(prm["fitness_score_thre"])) else 1, iterations=S.iterations, converged=S.converged, stop=S.stop,
               n_voxels=vm.n_voxels, n_corr=S.n_corr, T=T, fitness=fit, loss=S.loss)
    res["C_src"], res["C_tgt"], res["src_c"], res["tgt_c"] = C_src, C_tgt, src_c, tgt_c
    return res
