"""mulls_pcl_icp restated in numpy from the definition in include/mulls_hip.h, which was written from reading upstream (cregistration.hpp:882-942 and
:84-315, pca.hpp) and, for what PCL 1.8.1 does inside, from memory: double arithmetic in the stated orders, float where the definition says float,
sin / cos correctly rounded through mpmath (memoised), brute-force searches.  Nothing here was compared with PCL, FLANN or Eigen themselves: none is a
dependency of this repository.  This module is the yardstick of tests/test_pcl_icp.py and of the fixture tests/golden/pcl_icp_cases.npz
(tests/golden/make_pcl_icp_golden.py), which tests/test_gpu_pcl_icp.py compares the device with."""
import math

import numpy as np

import gicp_restated as gr
from ndt_restated import DBL_MAX, _rot, cos_cr, crop, sin_cr, tree_sum  # noqa: F401

F32 = np.float32
STOP_NONE, STOP_ITERATIONS, STOP_TRANSFORM, STOP_ABS_MSE, STOP_REL_MSE, STOP_NO_CORRESPONDENCES, STOP_SINGULAR = range(7)
POINT2POINT, POINT2PLANE, PLANE2PLANE = range(3)
NN, NS = range(2)
SVD, LM, LLS = range(3)
MARGIN = 1.0 + 2.0 ** -20  # a cell's edge over the distance it serves
SUM_S, SUM_T, SUM_H, SUM_D2, N_SUMS = 0, 3, 6, 27, 28
_dot3 = gr._dot3


def default_params(**kw):
    p = dict(max_iter_num=20, dis_thre_unit=1.5, metrics=POINT2POINT, ce=NN, te=SVD, use_reciprocal_correspondence=0, use_trimmed_rejector=0,
             neighbor_radius=2.0, apply_intersection_filter=1, fitness_score_thre=10.0, transformation_epsilon=1e-8, euclidean_fitness_epsilon=1e-5)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def dist2(a, b):
    """float32 (.., 3) arrays -> ((dx dx + dy dy) + dz dz) in float"""
    with np.errstate(all="ignore"):
        d = a.astype(F32) - b.astype(F32)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def in_range(P, dist):
    """(n, 3) float32 -> (n,) bool: the cell floor(x (1 / (dist MARGIN))) lies in [-2^20, 2^20) on every axis"""
    inv = 1.0 / (float(F32(dist)) * MARGIN)
    with np.errstate(all="ignore"):
        q = np.floor(np.asarray(P, F32).astype(np.float64) * inv)
    return ((q >= -1048576.0) & (q < 1048576.0)).all(axis=1)


# ---- correspondences

def nearest(mov, tgt):
    """-> (index of the target point smallest by (d2, index), its d2 as float32) per row of mov"""
    idx, d2 = np.empty(len(mov), np.int64), np.empty(len(mov), F32)
    for b in range(0, len(mov), 256):
        d = dist2(mov[b:b + 256, None, :], tgt[None, :, :])
        k = d.argmin(axis=1)  # the first minimum: the lower index on a tie
        idx[b:b + 256], d2[b:b + 256] = k, d[np.arange(len(k)), k]
    return idx, d2


def correspondences(mov, tgt, thr, reciprocal):
    """-> match (n_src,) int64, -1 without a pair; d2 (n_src,) float32"""
    thr = float(F32(thr))
    live = in_range(mov, thr)
    match, d2 = np.full(len(mov), -1, np.int64), np.zeros(len(mov), F32)
    if live.any():
        sel = np.flatnonzero(live)
        m, d = nearest(mov[sel], tgt)
        keep = ~(d.astype(np.float64) > thr * thr)
        match[sel[keep]], d2[sel[keep]] = m[keep], d[keep]
    if reciprocal:
        cand = np.flatnonzero(live)
        for m in np.unique(match[match >= 0]):
            first = cand[dist2(mov[cand], tgt[m][None, :]).argmin()]  # smallest by (d2 to m, index) among the moved source
            drop = (match == m) & (np.arange(len(mov)) != first)
            match[drop], d2[drop] = -1, 0.0
    return match, d2


# ---- the target's normals

def normal_of_scatter(S, p):
    A = {(0, 0): float(S[0]), (0, 1): float(S[1]), (0, 2): float(S[2]), (1, 1): float(S[3]), (1, 2): float(S[4]), (2, 2): float(S[5])}
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(60):
        off = A[(0, 1)] * A[(0, 1)] + A[(0, 2)] * A[(0, 2)] + A[(1, 2)] * A[(1, 2)]
        if not off >= 1e-300:
            break
        _rot(A, V, 0, 1, 2)
        _rot(A, V, 0, 2, 1)
        _rot(A, V, 1, 2, 0)
    e, c = A[(0, 0)], 0
    if A[(1, 1)] < e:
        e, c = A[(1, 1)], 1
    if A[(2, 2)] < e:
        e, c = A[(2, 2)], 2
    x, y, z = V[0][c], V[1][c], V[2][c]
    nrm = math.sqrt((x * x + y * y) + z * z)
    x, y, z = x / nrm, y / nrm, z / nrm
    if _dot3(x, y, z, -float(p[0]), -float(p[1]), -float(p[2])) < 0.0:
        x, y, z = -x, -y, -z
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
        return [F32(0.577)] * 3
    return [F32(x), F32(y), F32(z)]


def point_normal(Q, p):
    """Q: (k, 3) the neighbours in their order (doubles), p the point -> 3 float32"""
    Q = np.asarray(Q, np.float64).reshape(-1, 3)
    k = len(Q)
    if k < 3:
        return [F32(0.577)] * 3
    s = np.cumsum(Q, axis=0)[-1]  # (sequential: one neighbour at a time)
    m = s / float(k)
    d = Q - m[None, :]
    S = [float(np.cumsum(d[:, a] * d[:, b])[-1]) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return normal_of_scatter(S, p)


def neighbourhood(tgt, i, radius):
    r = float(F32(radius))
    return np.flatnonzero(dist2(tgt, tgt[i][None, :]).astype(np.float64) <= r * r)


def normals(tgt, radius):
    tgt = np.ascontiguousarray(tgt, F32)
    return np.array([point_normal(tgt[neighbourhood(tgt, i, radius)].astype(np.float64), tgt[i]) for i in range(len(tgt))], F32).reshape(len(tgt), 3)


# ---- the steps

def rigid_step(H, cs, ct):
    """-> R (9, row-major), t (3): csrc/ransac_math.h's decomposition in double"""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (float(v) for v in H)
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0] = (Sxx + Syy) + Szz
    A[1][1] = (Sxx - Syy) - Szz
    A[2][2] = (Syy - Sxx) - Szz
    A[3][3] = (Szz - Sxx) - Syy
    A[0][1] = A[1][0] = Syz - Szy
    A[0][2] = A[2][0] = Szx - Sxz
    A[0][3] = A[3][0] = Sxy - Syx
    A[1][2] = A[2][1] = Sxy + Syx
    A[1][3] = A[3][1] = Szx + Sxz
    A[2][3] = A[3][2] = Syz + Szy
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(10):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = gr._div(A[q][q] - A[p][p], 2.0 * apq)
                tn = gr._div(1.0, abs(theta) + gr._sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    tn = -tn
                c = gr._div(1.0, gr._sqrt(tn * tn + 1.0))
                s = tn * c
                for k in range(4):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
                for k in range(4):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
                for k in range(4):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    best, q = A[0][0], [V[r][0] for r in range(4)]
    for k in range(1, 4):
        if A[k][k] > best:
            best, q = A[k][k], [V[r][k] for r in range(4)]
    q0, qx, qy, qz = q
    nrm = gr._sqrt(((q0 * q0 + qx * qx) + qy * qy) + qz * qz)
    q0, qx, qy, qz = gr._div(q0, nrm), gr._div(qx, nrm), gr._div(qy, nrm), gr._div(qz, nrm)
    q00, qxx, qyy, qzz = q0 * q0, qx * qx, qy * qy, qz * qz
    qxy, qxz, qyz, q0x, q0y, q0z = qx * qy, qx * qz, qy * qz, q0 * qx, q0 * qy, q0 * qz
    R = [((q00 + qxx) - qyy) - qzz, 2.0 * (qxy - q0z), 2.0 * (qxz + q0y),
         2.0 * (qxy + q0z), ((q00 - qxx) + qyy) - qzz, 2.0 * (qyz - q0x),
         2.0 * (qxz - q0y), 2.0 * (qyz + q0x), ((q00 - qxx) - qyy) + qzz]
    t = [float(ct[r]) - _dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], float(cs[0]), float(cs[1]), float(cs[2])) for r in range(3)]
    return R, t


def plane_terms(s, t, n):
    """(m, 3) doubles each -> (m, 28): the upper triangle of row^T row, row^T b; column 27 stays 0"""
    out = np.zeros((len(s), N_SUMS))
    with np.errstate(all="ignore"):
        row = [s[:, 1] * n[:, 2] - s[:, 2] * n[:, 1], s[:, 2] * n[:, 0] - s[:, 0] * n[:, 2], s[:, 0] * n[:, 1] - s[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
        b = _dot3(n[:, 0], n[:, 1], n[:, 2], t[:, 0] - s[:, 0], t[:, 1] - s[:, 1], t[:, 2] - s[:, 2])
        at = 0
        for i in range(6):
            for k in range(i, 6):
                out[:, at] = 0.0 + row[i] * row[k]  # (added to a sum that starts at +0: no -0)
                at += 1
        for i in range(6):
            out[:, 21 + i] = 0.0 + row[i] * b
    return out


def plane_step(sums):
    """-> R, t, ok"""
    x, ok = gr.solve_step(sums[:21], sums[21:27])
    if not ok:
        return None, None, False
    ca, sa, cb, sb, cg, sg = cos_cr(x[0]), sin_cr(x[0]), cos_cr(x[1]), sin_cr(x[1]), cos_cr(x[2]), sin_cr(x[2])
    R = [cg * cb, (-sg) * ca + (cg * sb) * sa, sg * sa + (cg * sb) * ca,
         sg * cb, cg * ca + (sg * sb) * sa, (-cg) * sa + (sg * sb) * ca,
         -sb, cb * sa, cb * ca]
    return R, [x[3], x[4], x[5]], True


def evaluate(mov, tgt, nrm, match, d2, metric):
    """-> the 28 sums of an iteration, the number of pairs"""
    sel = np.flatnonzero(match >= 0)
    n = len(sel)
    per = np.zeros((len(mov), N_SUMS))
    s, t = mov[sel].astype(np.float64), tgt[match[sel]].astype(np.float64)
    per[sel, SUM_D2] = d2[sel].astype(np.float64)
    if metric == POINT2PLANE:
        terms = plane_terms(s, t, nrm[match[sel]].astype(np.float64))
        per[sel, :27] = terms[:, :27]
        return tree_sum(per), n
    per[sel, SUM_S:SUM_S + 3], per[sel, SUM_T:SUM_T + 3] = s, t
    sums = tree_sum(per)
    with np.errstate(all="ignore"):
        c = sums[:6] / float(n)
        sd, gd = s - c[None, :3], t - c[None, 3:6]
        for a in range(3):
            for b in range(3):
                per[sel, SUM_H + 3 * a + b] = sd[:, a] * gd[:, b]
    sums[SUM_H:SUM_H + 9] = tree_sum(per[:, SUM_H:SUM_H + 9])
    return sums, n


# ---- the loop's state

class State:
    def __init__(self):
        self.R, self.t = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
        self.Rs, self.ts = list(self.R), [0.0, 0.0, 0.0]
        self.mse, self.prev_mse = 0.0, DBL_MAX
        self.n_corr, self.iterations, self.converged, self.stop, self.running, self.moved = 0, 0, 0, STOP_NONE, 1, 0

    def row(self):
        return self.R + self.t + self.Rs + self.ts + [self.mse, self.prev_mse, self.n_corr, self.iterations, self.converged, self.stop, self.running, self.moved]


def _end(S, stop, converged):
    S.stop, S.converged, S.running = stop, converged, 0


def advance(S, metric, sums, n_corr, max_iter_num, transformation_epsilon, euclidean_fitness_epsilon):
    sums = [float(v) for v in sums]
    S.n_corr, S.moved = int(n_corr), 0
    S.mse = sums[SUM_D2] / float(n_corr) if n_corr else 0.0
    if n_corr < 3:
        return _end(S, STOP_NO_CORRESPONDENCES, 0)
    if metric == POINT2PLANE:
        Rs, ts, ok = plane_step(sums)
    else:
        dn = float(n_corr)
        Rs, ts = rigid_step(sums[SUM_H:SUM_H + 9], [v / dn for v in sums[SUM_S:SUM_S + 3]], [v / dn for v in sums[SUM_T:SUM_T + 3]])
        ok = True
    if ok and not all(math.isfinite(v) for v in Rs + ts):
        ok = False
    if not ok:
        return _end(S, STOP_SINGULAR, 0)
    Rn = gr.mat3_mul(Rs, S.R)
    tn = [_dot3(Rs[3 * r], Rs[3 * r + 1], Rs[3 * r + 2], S.t[0], S.t[1], S.t[2]) + ts[r] for r in range(3)]
    S.R, S.t, S.Rs, S.ts = Rn, tn, list(Rs), list(ts)
    S.moved = 1
    S.iterations += 1
    if S.iterations >= max_iter_num:
        return _end(S, STOP_ITERATIONS, 1)
    cos_angle = 0.5 * (((Rs[0] + Rs[4]) + Rs[8]) - 1.0)
    t2 = (ts[0] * ts[0] + ts[1] * ts[1]) + ts[2] * ts[2]
    if cos_angle >= 1.0 - transformation_epsilon and t2 <= transformation_epsilon:
        return _end(S, STOP_TRANSFORM, 1)
    d = abs(S.mse - S.prev_mse)
    if d < 1e-12:
        return _end(S, STOP_ABS_MSE, 1)
    if gr._div(d, S.prev_mse) < euclidean_fitness_epsilon:
        return _end(S, STOP_REL_MSE, 1)
    S.prev_mse = S.mse


# ---- the whole call

def fitness_of(src, tgt, R, t, fit_range):
    """-> fitness, n_fit"""
    xp = gr.move(R, t, src).astype(F32)
    _, d2 = nearest(xp, tgt)
    d2 = d2.astype(np.float64)
    counted = d2 <= float(F32(fit_range))
    n_fit = int(counted.sum())
    return (float(tree_sum(np.where(counted, d2, 0.0))) / float(n_fit) if n_fit else DBL_MAX), n_fit


def pcl_icp(tgt, src, tgt_bound, src_bound, guess, prm=None, trace=None):
    """-> dict of mulls_pcl_icp_result's fields (T row-major (4, 4)); None when a coordinate is outside the cells' range.  trace, a list, receives
    (sums, n_corr) per iteration"""
    prm = prm or default_params()
    assert prm["metrics"] in (POINT2POINT, POINT2PLANE) and prm["ce"] == NN and prm["te"] in (SVD, LLS) and not prm["use_trimmed_rejector"]
    G = np.asarray(guess, np.float64).reshape(4, 4)
    thr, metric = prm["dis_thre_unit"], prm["metrics"]
    tgt_c, src_c, apply_guess = crop(tgt, src, tgt_bound, src_bound, G, prm["apply_intersection_filter"])
    res = dict(code=-3, iterations=0, converged=0, stop=STOP_NONE, n_src=len(src_c), n_tgt=len(tgt_c), n_corr=0, n_fit=0, mse=0.0,
               T=G.copy() if apply_guess else np.eye(4), fitness=DBL_MAX)
    if len(src_c) == 0 or len(tgt_c) == 0:
        return res
    if not in_range(tgt_c, thr).all() or not in_range(src_c, thr).all() or (metric == POINT2PLANE and not in_range(tgt_c, prm["neighbor_radius"]).all()):
        return None
    nrm = normals(tgt_c, prm["neighbor_radius"]) if metric == POINT2PLANE else None
    S = State()
    mov = src_c.copy()
    for _ in range(prm["max_iter_num"]):
        match, d2 = correspondences(mov, tgt_c, thr, prm["use_reciprocal_correspondence"])
        sums, n_corr = evaluate(mov, tgt_c, nrm, match, d2, metric)
        if trace is not None:
            trace.append((sums.copy(), n_corr))
        advance(S, metric, sums, n_corr, prm["max_iter_num"], prm["transformation_epsilon"], prm["euclidean_fitness_epsilon"])
        if S.moved:
            mov = gr.move(S.Rs, S.ts, mov).astype(F32)
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
    fit, n_fit = fitness_of(src_c, tgt_c, S.R, S.t, thr)
    res.update(code=-3 if fit > float(F32(prm["fitness_score_thre"])) else 1, iterations=S.iterations, converged=S.converged, stop=S.stop,
               n_corr=S.n_corr, n_fit=n_fit, mse=S.mse, T=T, fitness=fit)
    res["src_c"], res["tgt_c"], res["normals"] = src_c, tgt_c, nrm
    return res
