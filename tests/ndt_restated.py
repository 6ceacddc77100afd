"""mulls_ndt restated in numpy from reading upstream (cregistration.hpp:945-1021, baseline_reg/ndt_omp_impl.hpp,
baseline_reg/voxel_grid_covariance_omp_impl.hpp) and the definition in include/mulls_hip.h: double arithmetic in the stated orders, float where the
definition says float, exp / sin / cos correctly rounded through mpmath (memoised), the score constants through math.log / math.exp.  Nothing here was
compared with ndt_omp or PCL themselves: neither is a dependency of this repository.  This module is the yardstick of tests/test_ndt.py and of the
fixture tests/golden/ndt_cases.npz (tests/golden/make_ndt_golden.py), which tests/test_gpu_ndt.py compares the device with."""
import math

import mpmath
import numpy as np

TREE = 4096  # MULLS_NDT_TREE
KDTREE, DIRECT26, DIRECT7, DIRECT1 = 0, 1, 2, 3
DBL_MAX = 1.7976931348623157e308

_memo = {}


def _cr(name, x):
    key = (name, x)
    v = _memo.get(key)
    if v is None:
        with mpmath.workprec(240):
            v = _memo[key] = float(getattr(mpmath, name)(mpmath.mpf(x)))
    return v


def exp_cr(x):
    if x != x:
        return x
    if x < -700.0:
        return 0.0
    if x > 700.0:
        return math.inf
    return _cr("exp", float(x))


def sin_cr(x):
    return _cr("sin", float(x))


def cos_cr(x):
    return _cr("cos", float(x))


def default_params(**kw):
    p = dict(resolution=1.0, search_method=DIRECT7, apply_intersection_filter=1, fitness_score_thre=10.0, step_size=0.1, transformation_epsilon=0.1,
             outlier_ratio=0.55, min_covar_eigvalue_mult=0.01, max_iterations=35, max_step_iterations=10, min_points_per_voxel=6)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def gauss_constants(resolution, outlier_ratio):
    c1 = 10 * (1 - outlier_ratio)
    c2 = outlier_ratio / math.pow(float(np.float32(resolution)), 3)
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    return d1, d2, d3


def is_identity(G, prec=1e-6):
    for r in range(4):
        for c in range(4):
            v = float(G[r, c])
            if r == c:
                if not abs(v - 1.0) <= min(abs(v), 1.0) * prec:
                    return False
            elif not abs(v) <= prec:
                return False
    return True


OFFSETS7 = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def offsets26():
    half = [(i, j, -1) for i in (-1, 0, 1) for j in (-1, 0, 1)] + [(i, -1, 0) for i in (-1, 0, 1)] + [(-1, 0, 0)]
    return half + [(-a, -b, -c) for a, b, c in half]


def offsets_of(method):
    return {DIRECT1: OFFSETS7[:1], DIRECT7: OFFSETS7, DIRECT26: offsets26()}[method]


# ---- a leaf

def _rot(A, V, p, q, r):
    """csrc/jacobi_rot.h: the rotation annihilating A[p][q] of a symmetric 3 x 3 kept as its upper triangle (r: the third index)"""
    key = lambda i, j: (min(i, j), max(i, j))
    apq = A[key(p, q)]
    if apq == 0.0:
        return
    app, aqq, apr, aqr = A[(p, p)], A[(q, q)], A[key(p, r)], A[key(q, r)]
    theta = (aqq - app) / (2.0 * apq)
    t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    cs = 1.0 / math.sqrt(t * t + 1.0)
    sn = t * cs
    c_pp, c_pq = cs * app - sn * apq, sn * app + cs * apq
    c_qp, c_qq = cs * apq - sn * aqq, sn * apq + cs * aqq
    c_rp, c_rq = cs * apr - sn * aqr, sn * apr + cs * aqr
    A[(p, p)] = cs * c_pp - sn * c_qp
    A[(q, q)] = sn * c_pq + cs * c_qq
    A[key(p, q)] = cs * c_pq - sn * c_qq
    A[key(p, r)] = c_rp
    A[key(q, r)] = c_rq
    for k in range(3):
        u, w = V[k][p], V[k][q]
        V[k][p], V[k][q] = cs * u - sn * w, sn * u + cs * w


def finalize_leaf(n, s, q, min_points=6, eig_mult=0.01):
    """-> dict(mean, icov (xx xy xz yy yz zz), evals, n, inflated)"""
    s = [float(v) for v in s]
    q = [float(v) for v in q]
    dn = float(n)
    m = [s[0] / dn, s[1] / dn, s[2] / dn]
    L = dict(mean=m, icov=[0.0] * 6, evals=[0.0] * 3, n=int(n), inflated=0)
    if n < min_points:
        return L
    f = (dn - 1.0) / dn
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    A = {}
    for k, (a, b) in enumerate(pairs):
        A[(a, b)] = ((q[k] - 2.0 * (s[b] * m[a])) / dn + m[b] * m[a]) * f
    c = dict(A)
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(60):
        off = A[(0, 1)] * A[(0, 1)] + A[(0, 2)] * A[(0, 2)] + A[(1, 2)] * A[(1, 2)]
        if not off >= 1e-300:
            break
        _rot(A, V, 0, 1, 2)
        _rot(A, V, 0, 2, 1)
        _rot(A, V, 1, 2, 0)
    e = [A[(0, 0)], A[(1, 1)], A[(2, 2)]]
    vec = [[V[0][k], V[1][k], V[2][k]] for k in range(3)]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        if e[b] < e[a]:
            e[a], e[b] = e[b], e[a]
            vec[a], vec[b] = vec[b], vec[a]
    if e[0] < 0.0 or e[1] < 0.0 or not e[2] > 0.0:
        L["n"] = -1
        return L
    lo = eig_mult * e[2]
    if e[0] < lo:
        e[0] = lo
        L["inflated"] = 1
        if e[1] < lo:
            e[1] = lo
            L["inflated"] = 2
        for a, b in pairs:
            c[(a, b)] = ((vec[0][a] * e[0]) * vec[0][b] + (vec[1][a] * e[1]) * vec[1][b]) + (vec[2][a] * e[2]) * vec[2][b]
    L["evals"] = list(e)
    c00, c01, c02, c11, c12, c22 = c[(0, 0)], c[(0, 1)], c[(0, 2)], c[(1, 1)], c[(1, 2)], c[(2, 2)]
    k00, k01, k02 = c11 * c22 - c12 * c12, c02 * c12 - c01 * c22, c01 * c12 - c02 * c11
    k11, k12, k22 = c00 * c22 - c02 * c02, c01 * c02 - c00 * c12, c00 * c11 - c01 * c01
    det = (c00 * k00 + c01 * k01) + c02 * k02
    with np.errstate(all="ignore"):
        L["icov"] = [float(np.float64(k) / np.float64(det)) for k in (k00, k01, k02, k11, k12, k22)]
    if any(math.isinf(v) for v in L["icov"]):
        L["n"] = -1
    return L


class Grid:
    pass


def build_grid(tgt, resolution, min_points=6, eig_mult=0.01):
    """tgt: (n, 3) float32, the cropped target.  -> Grid, or None for the grid refusals"""
    tgt = np.ascontiguousarray(tgt, np.float32)
    inv = np.float32(1.0) / np.float32(resolution)
    mn, mx = tgt.min(axis=0), tgt.max(axis=0)
    d = [int(np.float32(mx[c] - mn[c]) * inv) + 1 for c in range(3)]
    g = Grid()
    g.min_b = [int(np.floor(mn[c] * inv)) for c in range(3)]
    g.max_b = [int(np.floor(mx[c] * inv)) for c in range(3)]
    g.div_b = [g.max_b[c] - g.min_b[c] + 1 for c in range(3)]
    if d[0] * d[1] * d[2] > 2 ** 31 - 1 or g.div_b[0] * g.div_b[1] * g.div_b[2] > 2 ** 31 - 1:
        return None
    ijk = [(np.floor(tgt[:, c] * inv) - np.float32(g.min_b[c])).astype(np.int64) for c in range(3)]
    key = ijk[0] + ijk[1] * g.div_b[0] + ijk[2] * (g.div_b[0] * g.div_b[1])
    order = np.argsort(key, kind="stable")
    ks = key[order]
    cuts = np.flatnonzero(np.diff(ks)) + 1
    groups = np.split(order, cuts)
    g.index, means, icovs, ns, g.leaves = {}, [], [], [], []
    t64 = tgt.astype(np.float64)
    for grp in groups:
        s, q = [0.0, 0.0, 0.0], [0.0] * 6
        for i in grp:  # input order: the stable sort keeps it
            x, y, z = (float(v) for v in t64[i])
            s[0] += x
            s[1] += y
            s[2] += z
            q[0] += x * x
            q[1] += x * y
            q[2] += x * z
            q[3] += y * y
            q[4] += y * z
            q[5] += z * z
        L = finalize_leaf(len(grp), s, q, min_points, eig_mult)
        g.index[int(key[grp[0]])] = len(g.leaves)
        g.leaves.append(L)
        means.append(L["mean"])
        icovs.append(L["icov"])
        ns.append(L["n"])
    g.mean, g.icov, g.n = np.array(means, np.float64), np.array(icovs, np.float64), np.array(ns, np.int64)
    g.n_leaves = len(g.leaves)
    g.n_leaves_used = int((g.n >= min_points).sum())
    g.resolution, g.min_points = np.float32(resolution), min_points
    return g


# ---- an evaluation

def make_frame(p):
    p = [float(v) for v in p]
    cx, sx, cy, sy, cz, sz = cos_cr(p[3]), sin_cr(p[3]), cos_cr(p[4]), sin_cr(p[4]), cos_cr(p[5]), sin_cr(p[5])
    R = [cy * cz, -cy * sz, sy,
         cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy,
         sx * sz - cx * sy * cz, cx * sy * sz + sx * cz, cx * cy]
    t = p[:3]
    if abs(p[3]) < 10e-5:
        cx, sx = 1.0, 0.0
    if abs(p[4]) < 10e-5:
        cy, sy = 1.0, 0.0
    if abs(p[5]) < 10e-5:
        cz, sz = 1.0, 0.0
    j = [((-sx * sz + cx * sy * cz), (-sx * cz - cx * sy * sz), (-cx * cy)),
         ((cx * sz + sx * sy * cz), (cx * cz - sx * sy * sz), (-sx * cy)),
         ((-sy * cz), sy * sz, cy),
         (sx * cy * cz, (-sx * cy * sz), sx * sy),
         ((-cx * cy * cz), cx * cy * sz, (-cx * sy)),
         ((-cy * sz), (-cy * cz), 0.0),
         ((cx * cz - sx * sy * sz), (-cx * sz - sx * sy * cz), 0.0),
         ((sx * cz + cx * sy * sz), (cx * sy * cz - sx * sz), 0.0)]
    h = [((-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), sx * cy),
         ((-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), (-cx * cy)),
         ((cx * cy * cz), (-cx * cy * sz), (cx * sy)),
         ((sx * cy * cz), (-sx * cy * sz), (sx * sy)),
         ((-sx * cz - cx * sy * sz), (sx * sz - cx * sy * cz), 0.0),
         ((cx * cz - sx * sy * sz), (-sx * sy * cz - cx * sz), 0.0),
         ((-cy * cz), (cy * sz), (sy)),
         ((-sx * sy * cz), (sx * sy * sz), (sx * cy)),
         ((cx * sy * cz), (-cx * sy * sz), (-cx * cy)),
         ((sy * sz), (sy * cz), 0.0),
         ((-sx * cy * sz), (-sx * cy * cz), 0.0),
         ((cx * cy * sz), (cx * cy * cz), 0.0),
         ((-cy * cz), (cy * sz), 0.0),
         ((-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), 0.0),
         ((-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), 0.0)]
    return dict(R=R, t=t, j=j, h=h)


def transform(F, src):
    """T(p) x in double, rounded to float: (n, 3) float32"""
    x = src.astype(np.float64)
    R, t = F["R"], F["t"]
    with np.errstate(all="ignore"):
        return np.stack([(((R[3 * r] * x[:, 0] + R[3 * r + 1] * x[:, 1]) + R[3 * r + 2] * x[:, 2]) + t[r]).astype(np.float32) for r in range(3)], axis=1)


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def contribution(x, xt, C, F, d1, d2, with_hessian):
    """(m, 3) source points, (m, 3) transformed-minus-mean, (m, 6) icov -> (m, 28) terms (all zero where the pair adds nothing)"""
    m = len(x)
    out = np.zeros((m, 28))
    if m == 0:
        return out
    j, h = F["j"], F["h"]
    c = [[C[:, 0], C[:, 1], C[:, 2]], [C[:, 1], C[:, 3], C[:, 4]], [C[:, 2], C[:, 4], C[:, 5]]]
    X = [xt[:, 0], xt[:, 1], xt[:, 2]]
    x = [x[:, 0], x[:, 1], x[:, 2]]
    with np.errstate(all="ignore"):
        cx = [_dot3(c[r][0], c[r][1], c[r][2], X[0], X[1], X[2]) for r in range(3)]
        q = _dot3(X[0], X[1], X[2], cx[0], cx[1], cx[2])
        e = np.array([exp_cr(float(v)) for v in (-d2 * q) / 2.0])
        score_inc = -d1 * e
        e2 = d2 * e
        ok = ~((e2 > 1.0) | (e2 < 0.0) | (e2 != e2))
        e2 = e2 * d1
        zero, one = np.zeros(m), np.ones(m)
        J = [[one, zero, zero, zero, None, None], [zero, one, zero, None, None, None], [zero, zero, one, None, None, None]]
        J[1][3], J[2][3] = _dot3(x[0], x[1], x[2], *j[0]), _dot3(x[0], x[1], x[2], *j[1])
        J[0][4], J[1][4], J[2][4] = _dot3(x[0], x[1], x[2], *j[2]), _dot3(x[0], x[1], x[2], *j[3]), _dot3(x[0], x[1], x[2], *j[4])
        J[0][5], J[1][5], J[2][5] = _dot3(x[0], x[1], x[2], *j[5]), _dot3(x[0], x[1], x[2], *j[6]), _dot3(x[0], x[1], x[2], *j[7])
        cJ, g = [], []
        for k in range(6):
            col = [c[r][k] if k < 3 else _dot3(c[r][0], c[r][1], c[r][2], J[0][k], J[1][k], J[2][k]) for r in range(3)]
            cJ.append(col)
            g.append(_dot3(X[0], X[1], X[2], col[0], col[1], col[2]))
        out[:, 0] = np.where(ok, score_inc, 0.0)
        for k in range(6):
            out[:, 1 + k] = np.where(ok, e2 * g[k], 0.0)
        if with_hessian:
            hv = []
            for mm in range(3):
                hv.append([zero, _dot3(x[0], x[1], x[2], *h[2 * mm]), _dot3(x[0], x[1], x[2], *h[2 * mm + 1])])
            for mm in range(3):
                hv.append([_dot3(x[0], x[1], x[2], *h[6 + 3 * mm + r]) for r in range(3)])
            at = 7
            for i in range(6):
                for k in range(i, 6):
                    inner = (-d2 * g[i]) * g[k]
                    if i >= 3:
                        b = k - 3 if i == 3 else (k - 1 if i == 4 else 5)
                        inner = inner + _dot3(cx[0], cx[1], cx[2], hv[b][0], hv[b][1], hv[b][2])
                    inner = inner + (cJ[i][k] if k < 3 else _dot3(J[0][k], J[1][k], J[2][k], cJ[i][0], cJ[i][1], cJ[i][2]))
                    out[:, at] = np.where(ok, e2 * inner, 0.0)
                    at += 1
    return out


def tree_sum(terms):
    """terms: (n,) or (n, k) in point order -> the defined sum(s): strided partials of width TREE, then the pairwise tree"""
    terms = np.asarray(terms, np.float64)
    shape = terms.shape[1:]
    part = np.zeros((TREE,) + shape)
    with np.errstate(all="ignore"):
        for b in range(0, len(terms), TREE):
            chunk = terms[b:b + TREE]
            part[:len(chunk)] += chunk
        w = TREE // 2
        while w >= 1:
            part[:w] += part[w:2 * w]
            w //= 2
    return part[0]


def evaluate(src, p, grid, d1, d2, with_hessian, method=DIRECT7, frame=None, per_point_out=None):
    """the 28 sums at p; per_point_out, a list, receives the (n, 28) terms the sums are taken over"""
    F = frame if frame is not None else make_frame(p)
    xp = transform(F, src)
    n = len(src)
    per_point = np.zeros((n, 28))
    with np.errstate(all="ignore"):
        qf = np.floor(xp / grid.resolution)
    fine = (np.abs(qf) < 2.0 ** 30).all(axis=1)  # NaN and infinity fail the comparison
    ijk = np.where(fine[:, None], qf, 0).astype(np.int64)
    x64, xp64 = src.astype(np.float64), xp.astype(np.float64)
    for off in offsets_of(method):
        cell = ijk + np.array(off)
        inside = fine.copy()
        for c in range(3):
            inside &= (cell[:, c] >= grid.min_b[c]) & (cell[:, c] <= grid.max_b[c])
        key = (cell[:, 0] - grid.min_b[0]) + (cell[:, 1] - grid.min_b[1]) * grid.div_b[0] + (cell[:, 2] - grid.min_b[2]) * (grid.div_b[0] * grid.div_b[1])
        leaf = np.array([grid.index.get(int(k), -1) if ins else -1 for k, ins in zip(key, inside)], np.int64)
        sel = np.flatnonzero(leaf >= 0)
        sel = sel[grid.n[leaf[sel]] >= grid.min_points]
        if len(sel) == 0:
            continue
        li = leaf[sel]
        terms = contribution(x64[sel], xp64[sel] - grid.mean[li], grid.icov[li], F, d1, d2, with_hessian)
        with np.errstate(all="ignore"):
            per_point[sel] += terms
    if per_point_out is not None:
        per_point_out.append(per_point)
    return tree_sum(per_point)


# ---- the 6 x 6 solve

SOLVE_SWEEPS = 12


def solve6(Hu, g):
    A = [[0.0] * 6 for _ in range(6)]
    at = 0
    for i in range(6):
        for k in range(i, 6):
            A[i][k] = A[k][i] = float(Hu[at])
            at += 1
    V = [[1.0 if i == k else 0.0 for k in range(6)] for i in range(6)]
    g = [float(v) for v in g]
    nan = float("nan")

    def fsqrt(v):
        return math.sqrt(v) if v >= 0 else nan

    for _ in range(SOLVE_SWEEPS):
        for p in range(5):
            for q in range(p + 1, 6):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                with np.errstate(all="ignore"):
                    theta = float((np.float64(A[q][q]) - np.float64(A[p][p])) / np.float64(2.0 * apq))
                    t = float(np.float64(1.0 if theta >= 0 else -1.0) / (np.float64(abs(theta)) + np.sqrt(np.float64(theta) * np.float64(theta) + 1.0)))
                    cs = float(np.float64(1.0) / np.sqrt(np.float64(t) * np.float64(t) + 1.0))
                sn = t * cs
                for k in range(6):
                    u, w = A[k][p], A[k][q]
                    A[k][p], A[k][q] = cs * u - sn * w, sn * u + cs * w
                for k in range(6):
                    u, w = A[p][k], A[q][k]
                    A[p][k], A[q][k] = cs * u - sn * w, sn * u + cs * w
                A[p][q] = A[q][p] = 0.0
                for k in range(6):
                    u, w = V[k][p], V[k][q]
                    V[k][p], V[k][q] = cs * u - sn * w, sn * u + cs * w
    big = 0.0
    for k in range(6):
        m = abs(A[k][k])
        big = m if m > big else big
    thr = (6.0 * 2.0 ** -52) * big
    c = []
    for k in range(6):
        t = 0.0
        for i in range(6):
            t += V[i][k] * g[i]
        lam = A[k][k]
        if abs(lam) > thr:
            with np.errstate(all="ignore"):
                c.append(float(np.float64(t) / np.float64(lam)))
        else:
            c.append(lam if lam != lam else 0.0)
    delta = []
    for i in range(6):
        s = 0.0
        for k in range(6):
            s += V[i][k] * c[k]
        delta.append(-s)
    return delta


# ---- the Newton loop and the line search as a state that advances by one evaluation (csrc/ndt_math.h has the same text in C++)

PH_INIT, PH_MT_FIRST, PH_MT_LOOP, PH_HESS = range(4)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(v):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(v)))


class State:
    def __init__(self):
        self.p, self.xt, self.x0, self.dir = [0.0] * 6, [0.0] * 6, [0.0] * 6, [0.0] * 6
        self.score, self.g, self.H = 0.0, [0.0] * 6, [0.0] * 21
        self.phi_0 = self.d_phi_0 = self.a_l = self.f_l = self.g_l = self.a_u = self.f_u = self.g_u = self.a_t = 0.0
        self.phi_t = self.d_phi_t = self.psi_t = self.d_psi_t = self.trans_probability = 0.0
        self.phase, self.step_iterations, self.interval_converged, self.open_interval = PH_INIT, 0, 0, 0
        self.nr_iterations, self.evaluations, self.converged, self.running = 0, 1, 0, 1
        self.with_hessian, self.reversals, self.inner_steps = 1, 0, 0


def _update_interval(S, a_t, f_t, g_t):
    if f_t > S.f_l:
        S.a_u, S.f_u, S.g_u = a_t, f_t, g_t
        return False
    if g_t * (S.a_l - a_t) > 0:
        S.a_l, S.f_l, S.g_l = a_t, f_t, g_t
        return False
    if g_t * (S.a_l - a_t) < 0:
        S.a_u, S.f_u, S.g_u = S.a_l, S.f_l, S.g_l
        S.a_l, S.f_l, S.g_l = a_t, f_t, g_t
        return False
    return True


def trial_value(a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t):
    if f_t > f_l:
        z = _div(3 * (f_t - f_l), (a_t - a_l)) - g_t - g_l
        w = _sqrt(z * z - g_t * g_l)
        a_c = a_l + _div((a_t - a_l) * (w - g_l - z), (g_t - g_l + 2 * w))
        a_q = a_l - _div(0.5 * (a_l - a_t) * g_l, (g_l - _div((f_l - f_t), (a_l - a_t))))
        if abs(a_c - a_l) < abs(a_q - a_l):
            return a_c
        return 0.5 * (a_q + a_c)
    if g_t * g_l < 0:
        z = _div(3 * (f_t - f_l), (a_t - a_l)) - g_t - g_l
        w = _sqrt(z * z - g_t * g_l)
        a_c = a_l + _div((a_t - a_l) * (w - g_l - z), (g_t - g_l + 2 * w))
        a_s = a_l - _div((a_l - a_t), (g_l - g_t)) * g_l
        return a_c if abs(a_c - a_t) >= abs(a_s - a_t) else a_s
    if abs(g_t) <= abs(g_l):
        z = _div(3 * (f_t - f_l), (a_t - a_l)) - g_t - g_l
        w = _sqrt(z * z - g_t * g_l)
        a_c = a_l + _div((a_t - a_l) * (w - g_l - z), (g_t - g_l + 2 * w))
        a_s = a_l - _div((a_l - a_t), (g_l - g_t)) * g_l
        a_n = a_c if abs(a_c - a_t) < abs(a_s - a_t) else a_s
        lim = a_t + 0.66 * (a_u - a_t)
        if a_t > a_l:
            return a_n if a_n < lim else lim
        return a_n if lim < a_n else lim
    z = _div(3 * (f_t - f_u), (a_t - a_u)) - g_t - g_u
    w = _sqrt(z * z - g_t * g_u)
    return a_u + _div((a_t - a_u) * (w - g_u - z), (g_t - g_u + 2 * w))


def _clamp(a, lo, hi):
    a = hi if hi < a else a
    return lo if a < lo else a


def advance(S, sums, prm, n_src):
    mu, nu = 1.0e-4, 0.9
    step_max, step_min = prm["step_size"], prm["transformation_epsilon"] / 2
    sums = [float(v) for v in sums]
    if S.phase == PH_HESS:
        S.H = sums[7:28]
        nxt = "newton_end"
    else:
        S.score, S.g = sums[0], sums[1:7]
        if S.phase != PH_MT_LOOP:
            S.H = sums[7:28]
        if S.phase == PH_INIT:
            nxt = "newton_start"
        else:
            S.phi_t = -S.score
            d = 0.0
            for k in range(6):
                d += S.g[k] * S.dir[k]
            S.d_phi_t = -d
            S.psi_t = S.phi_t - S.phi_0 - mu * S.d_phi_0 * S.a_t
            S.d_psi_t = S.d_phi_t - mu * S.d_phi_0
            if S.phase == PH_MT_LOOP:
                if S.open_interval and (S.psi_t <= 0 and S.d_psi_t >= 0):
                    S.open_interval = 0
                    S.f_l = S.f_l + S.phi_0 - mu * S.d_phi_0 * S.a_l
                    S.g_l = S.g_l + mu * S.d_phi_0
                    S.f_u = S.f_u + S.phi_0 - mu * S.d_phi_0 * S.a_u
                    S.g_u = S.g_u + mu * S.d_phi_0
                if S.open_interval:
                    S.interval_converged = 1 if _update_interval(S, S.a_t, S.psi_t, S.d_psi_t) else 0
                else:
                    S.interval_converged = 1 if _update_interval(S, S.a_t, S.phi_t, S.d_phi_t) else 0
                S.step_iterations += 1
                S.inner_steps += 1
            nxt = "mt_check"
    for _ in range(8):
        if nxt == "mt_check":
            if not S.interval_converged and S.step_iterations < prm["max_step_iterations"] and not (S.psi_t <= 0 and S.d_phi_t <= -nu * S.d_phi_0):
                if S.open_interval:
                    S.a_t = trial_value(S.a_l, S.f_l, S.g_l, S.a_u, S.f_u, S.g_u, S.a_t, S.psi_t, S.d_psi_t)
                else:
                    S.a_t = trial_value(S.a_l, S.f_l, S.g_l, S.a_u, S.f_u, S.g_u, S.a_t, S.phi_t, S.d_phi_t)
                S.a_t = _clamp(S.a_t, step_min, step_max)
                S.xt = [S.x0[k] + S.dir[k] * S.a_t for k in range(6)]
                S.phase, S.with_hessian = PH_MT_LOOP, 0
                S.evaluations += 1
                return
            if S.step_iterations:
                S.phase, S.with_hessian = PH_HESS, 1
                S.evaluations += 1
                return
            nxt = "newton_end"
        elif nxt == "newton_end":
            S.p = [S.x0[k] + S.dir[k] * S.a_t for k in range(6)]
            if S.nr_iterations > prm["max_iterations"] or (S.nr_iterations and abs(S.a_t) < prm["transformation_epsilon"]):
                S.converged = 1
            S.nr_iterations += 1
            if S.converged:
                S.trans_probability = _div(S.score, float(n_src))
                S.running = 0
                return
            nxt = "newton_start"
        else:
            delta = solve6(S.H, S.g)
            n2 = 0.0
            for k in range(6):
                n2 += delta[k] * delta[k]
            norm = _sqrt(n2)
            if norm == 0 or norm != norm:
                S.trans_probability = _div(S.score, float(n_src))
                S.converged = 1 if norm == norm else 0
                S.running = 0
                return
            d = 0.0
            for k in range(6):
                S.dir[k] = _div(delta[k], norm)
                S.x0[k] = S.p[k]
                d += S.g[k] * S.dir[k]
            S.phi_0 = -S.score
            S.d_phi_0 = -d
            S.step_iterations = 0
            if S.d_phi_0 >= 0:
                if S.d_phi_0 == 0:
                    S.a_t = 0.0
                    nxt = "newton_end"
                    continue
                S.d_phi_0 = -S.d_phi_0
                S.dir = [-v for v in S.dir]
                S.reversals += 1
            S.a_l = S.a_u = 0.0
            S.f_l = S.phi_0 - S.phi_0 - mu * S.d_phi_0 * S.a_l
            S.g_l = S.d_phi_0 - mu * S.d_phi_0
            S.f_u = S.phi_0 - S.phi_0 - mu * S.d_phi_0 * S.a_u
            S.g_u = S.d_phi_0 - mu * S.d_phi_0
            S.interval_converged = 1 if (step_max - step_min) > 0 else 0
            S.open_interval = 1
            S.a_t = _clamp(norm, step_min, step_max)
            S.xt = [S.x0[k] + S.dir[k] * S.a_t for k in range(6)]
            S.phase, S.with_hessian = PH_MT_FIRST, 1
            S.evaluations += 1
            return
    S.running = 0


# ---- the whole call

def crop(tgt, src, tgt_bound, src_bound, guess, apply_filter):
    """-> cropped tgt, cropped (moved) src, apply_guess"""
    tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
    G = np.asarray(guess, np.float64).reshape(4, 4)
    apply_guess = not is_identity(G)
    tb, sb = np.asarray(tgt_bound, np.float64), np.asarray(src_bound, np.float64)
    if apply_guess:
        x = src.astype(np.float64)
        src = np.stack([(((G[r, 0] * x[:, 0] + G[r, 1] * x[:, 1]) + G[r, 2] * x[:, 2]) + G[r, 3]).astype(np.float32) for r in range(3)], axis=1)
        sb = np.concatenate([src.min(axis=0), src.max(axis=0)]).astype(np.float64)
    box = np.concatenate([np.where(tb[:3] > sb[:3], tb[:3], sb[:3]) - 2.0, np.where(tb[3:] < sb[3:], tb[3:], sb[3:]) + 2.0])
    if apply_filter:
        keep = lambda c: ((c.astype(np.float64) > box[:3]) & (c.astype(np.float64) < box[3:])).all(axis=1)
        tgt, src = tgt[keep(tgt)], src[keep(src)]
    return tgt, src, apply_guess


def fitness_of(src, tgt, p):
    xp = transform(make_frame(p), src)
    d2 = np.empty(len(xp), np.float32)
    for b in range(0, len(xp), 256):
        d = xp[b:b + 256, None, :] - tgt[None, :, :]
        d2[b:b + 256] = ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).min(axis=1)
    return float(tree_sum(d2.astype(np.float64))) / float(len(xp))


def pose_of(p):
    F = make_frame(p)
    T = np.eye(4)
    T[:3, :3] = np.array(F["R"]).reshape(3, 3)
    T[:3, 3] = F["t"]
    return T


def ndt(tgt, src, tgt_bound, src_bound, guess, prm=None, trace=None, with_fitness=True):
    """-> dict of mulls_ndt_result's fields (T row-major (4, 4)); None for the grid refusals.  with_fitness = False leaves the nearest-neighbour pass
    out (fitness None, code None): it is quadratic here"""
    prm = prm or default_params()
    d1, d2, d3 = gauss_constants(prm["resolution"], prm["outlier_ratio"])
    G = np.asarray(guess, np.float64).reshape(4, 4)
    tgt_c, src_c, apply_guess = crop(tgt, src, tgt_bound, src_bound, G, prm["apply_intersection_filter"])
    res = dict(code=-3, iterations=0, evaluations=0, converged=0, n_leaves=0, n_leaves_used=0, n_src=len(src_c), n_tgt=len(tgt_c),
               T=G.copy() if apply_guess else np.eye(4), fitness=DBL_MAX, trans_probability=0.0, gauss_d1=d1, gauss_d2=d2, gauss_d3=d3,
               line_search_reversals=0, inner_steps=0)
    if len(src_c) == 0 or len(tgt_c) == 0:
        return res
    grid = build_grid(tgt_c, prm["resolution"], prm["min_points_per_voxel"], prm["min_covar_eigvalue_mult"])
    if grid is None:
        return None
    S = State()
    for _ in range((prm["max_iterations"] + 2) * (prm["max_step_iterations"] + 2) + 1):
        sums = evaluate(src_c, S.xt, grid, d1, d2, S.with_hessian, prm["search_method"])
        if not S.with_hessian:
            sums[7:] = 0.0
        if trace is not None:
            trace.append((list(S.xt), S.with_hessian, S.phase, sums.copy()))
        advance(S, sums, prm, len(src_c))
        if not S.running:
            break
    Tn = pose_of(S.p)
    if apply_guess:
        T = np.empty((4, 4))
        for r in range(4):
            for c in range(4):
                T[r, c] = ((Tn[r, 0] * G[0, c] + Tn[r, 1] * G[1, c]) + Tn[r, 2] * G[2, c]) + Tn[r, 3] * G[3, c]
    else:
        T = Tn
    fit = fitness_of(src_c, tgt_c, S.p) if with_fitness else None
    res.update(code=None if fit is None else (-3 if fit > float(np.float32(prm["fitness_score_thre"])) else 1), iterations=S.nr_iterations, evaluations=S.evaluations,
               converged=S.converged, n_leaves=grid.n_leaves, n_leaves_used=grid.n_leaves_used, T=T, fitness=fit,
               trans_probability=S.trans_probability, line_search_reversals=S.reversals, inner_steps=S.inner_steps)
    res["p"] = list(S.p)
    return res
