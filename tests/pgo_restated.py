"""A numpy float64 restatement of the pose graph optimisation, written from the text in include/mulls_hip.h ("pose graph optimisation").

Everything is + - * / sqrt on float64, in the orders the header states: a 6-term sum starts from 0.0 and adds its products in ascending inner index, an
edge's contributions are added in ascending edge index, an entry's Schur updates are subtracted in ascending block column, the cost and model-decrease sums
are 256 strided partials and a pairwise tree.  numpy's element-wise operations round once each (no fused multiply-add), so vectorising over independent
entries keeps the bits; no sum goes through np.sum / np.dot / np.linalg.  The only exception is the edge check's atan2, which only decides a comparison.

solve() returns the result fields of mulls_pgo_result, the output poses, the edge flags, and what the tests want to know about the run: the smallest
distance of any accept / reject ratio from 1e-3, the largest excess of a clamped quaternion over its box before the last normalisation, and, when asked,
the relative residual of every linear system it solved.
"""
import math

import numpy as np

REGISTRATION, ADJACENT, HISTORY, SMOOTH, NONE = range(5)
TERM_NOT_RUN, TERM_MAX_ITERATIONS, TERM_FUNCTION_TOLERANCE, TERM_GRADIENT, TERM_STEP, TERM_RADIUS, TERM_NO_FREE = range(7)
TREE = 256

DEFAULTS = dict(num_iterations=100, robustify=0, use_equal_weight=0, use_diagonal_information_matrix=0, free_all_nodes=0, only_limit_translation=0,
                robust_delta=1.0, quat_tran_ratio=1000.0, t_limit=2.0, r_limit=0.05, function_tolerance=1e-16, wrong_edge_translation_thre=5.0,
                wrong_edge_rotation_thre=25.0, wrong_edge_ratio_thre=0.1)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


# ---- quaternions (x, y, z, w); every function works on arrays whose last axis is the quaternion ----
def qmul(p, q):
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    px, py, pz, pw = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    qx, qy, qz, qw = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([((pw * qx + px * qw) + py * qz) - pz * qy,
                     ((pw * qy + py * qw) + pz * qx) - px * qz,
                     ((pw * qz + pz * qw) + px * qy) - py * qx,
                     ((pw * qw - px * qx) - py * qy) - pz * qz], axis=-1)


def qconj(q):
    q = np.asarray(q, np.float64)
    return np.stack([-q[..., 0], -q[..., 1], -q[..., 2], q[..., 3]], axis=-1)


def qnormalise(q):
    q = np.asarray(q, np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])
        return q / n[..., None]


def qrot(q):
    """Eigen's toRotationMatrix; (..., 3, 3)"""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1.0 - (tyy + tzz), txy - twz, txz + twy
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = txy + twz, 1.0 - (txx + tzz), tyz - twx
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = txz - twy, tyz + twx, 1.0 - (txx + tyy)
    return R


def rot2quat(m):
    """Eigen's matrix -> quaternion of one 3 x 3, then the normalisation"""
    m = np.asarray(m, np.float64)
    q = np.zeros(4)
    t = (m[0, 0] + m[1, 1]) + m[2, 2]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return qnormalise(q)


def pose2state(T):
    T = np.asarray(T, np.float64)
    return np.concatenate([T[:3, 3], rot2quat(T[:3, :3])])


def state2pose(x):
    T = np.eye(4)
    T[:3, :3] = qrot(qnormalise(x[3:7]))
    T[:3, 3] = x[:3]
    return T


# ---- the defined sums ----
def tree_sum(terms):
    terms = np.asarray(terms, np.float64)
    p = np.zeros(TREE)
    with np.errstate(all="ignore"):
        for base in range(0, len(terms), TREE):
            c = terms[base:base + TREE]
            p[:len(c)] = p[:len(c)] + c
        w = TREE // 2
        while w >= 1:
            p[:w] = p[:w] + p[w:2 * w]
            w //= 2
    return p[0]


def absmax(x):
    """the largest |x_i|, NaN entries not counted, 0 for none"""
    x = np.abs(np.asarray(x, np.float64))
    x = x[~np.isnan(x)]
    return float(x.max()) if len(x) else 0.0


def dot6(A, B, axis_a, axis_b):
    """sum over m = 0 .. 5 of A[.., m, ..] * B[.., m, ..] from 0.0 in ascending m; A and B already broadcast-compatible, the inner index at the given axes"""
    acc = 0.0
    for m in range(6):
        acc = acc + np.take(A, m, axis=axis_a) * np.take(B, m, axis=axis_b)
    return acc


# ---- residual, Jacobians, an edge's blocks (vectorised over edges) ----
def residual(xa, xb, th, qh):
    """xa, xb (E, 7); th (E, 3); qh (E, 4) -> e (E, 6), R (E, 3, 3), v (E, 3), P, Q (E, 4)"""
    R = qrot(xa[:, 3:7])
    d = xb[:, :3] - xa[:, :3]
    v = np.stack([(R[:, 0, r] * d[:, 0] + R[:, 1, r] * d[:, 1]) + R[:, 2, r] * d[:, 2] for r in range(3)], axis=1)
    Q = qconj(qmul(qconj(xa[:, 3:7]), xb[:, 3:7]))
    P = qmul(qh, Q)
    e = np.concatenate([v - th, 2.0 * P[:, :3]], axis=1)
    return e, R, v, P, Q


def jacobians(R, v, P, Q, qh):
    E = len(v)
    Ja, Jb = np.zeros((E, 6, 6)), np.zeros((E, 6, 6))
    Rt = np.transpose(R, (0, 2, 1))
    Ja[:, :3, :3], Jb[:, :3, :3] = -Rt, Rt
    Ja[:, 0, 4], Ja[:, 0, 5] = -v[:, 2], v[:, 1]
    Ja[:, 1, 3], Ja[:, 1, 5] = v[:, 2], -v[:, 0]
    Ja[:, 2, 3], Ja[:, 2, 4] = -v[:, 1], v[:, 0]
    for c in range(3):
        Ec = np.zeros(4)
        Ec[c] = 1.0
        Ja[:, 3:, 3 + c] = qmul(P, Ec)[:, :3]
        Jb[:, 3:, 3 + c] = -qmul(qmul(qh, Ec), Q)[:, :3]
    return Ja, Jb


def weighted_square(W, e):
    u = dot6(W, e[:, None, :], 2, 2)  # u_k = sum_l W_kl e_l
    s = 0.0
    for k in range(6):
        s = s + e[:, k] * u[:, k]
    return s, u


def robust(s, robustify, delta):
    w = np.ones_like(s)
    rho = s.copy()
    if robustify:
        d2 = delta * delta
        big = s > d2
        with np.errstate(all="ignore"):
            r = np.sqrt(s)
            rho = np.where(big, (2.0 * delta) * r - d2, s)
            w = np.where(big, delta / r, 1.0)
    return rho, w


def edge_terms(X, ea, eb, th, qh, W, robustify, delta):
    e, _, _, _, _ = residual(X[ea], X[eb], th, qh)
    s, _ = weighted_square(W, e)
    return robust(s, robustify, delta)[0]


def linearise(X, ea, eb, th, qh, W, robustify, delta):
    e, R, v, P, Q = residual(X[ea], X[eb], th, qh)
    s, u = weighted_square(W, e)
    rho, w = robust(s, robustify, delta)
    Ja, Jb = jacobians(R, v, P, Q, qh)
    WJa = w[:, None, None] * dot6(W[:, :, :, None], Ja[:, None, :, :], 2, 2)
    WJb = w[:, None, None] * dot6(W[:, :, :, None], Jb[:, None, :, :], 2, 2)
    wu = w[:, None] * u
    Haa = dot6(Ja[:, :, :, None], WJa[:, :, None, :], 1, 1)
    Hab = dot6(Ja[:, :, :, None], WJb[:, :, None, :], 1, 1)
    Hbb = dot6(Jb[:, :, :, None], WJb[:, :, None, :], 1, 1)
    ga = dot6(Ja, wu[:, :, None], 1, 1)
    gb = dot6(Jb, wu[:, :, None], 1, 1)
    return rho, Haa, Hab, Hbb, ga, gb


def step_node(x, d, x0, boxed, tl, rl, only_translation):
    """-> the candidate state and the clamped quaternion before the last normalisation (None when the node's quaternion is not clamped)"""
    o = np.empty(7)
    o[:3] = x[:3] + d[:3]
    q = qnormalise(qmul(x[3:7], np.array([d[3] * 0.5, d[4] * 0.5, d[5] * 0.5, 1.0])))
    raw = None
    if boxed:
        for c in range(3):
            lo, hi = x0[c] - tl, x0[c] + tl
            t = lo if o[c] < lo else o[c]
            o[c] = hi if t > hi else t
        if not only_translation:
            dot = ((q[0] * x0[3] + q[1] * x0[4]) + q[2] * x0[5]) + q[3] * x0[6]
            if dot < 0.0:
                q = -q
            q = q.copy()
            for c in range(4):
                lo, hi = x0[3 + c] - rl, x0[3 + c] + rl
                t = lo if q[c] < lo else q[c]
                q[c] = hi if t > hi else t
            raw = q.copy()
            q = qnormalise(q)
    o[3:7] = q
    return o, raw


# ---- classes and limits ----
def classify(fixed, stable, edges, p):
    """-> used (indices of the used edges), early, cls (0 fixed, 1 boxed, 2 free per node), limits (n, 2)"""
    n = len(fixed)
    used = [k for k, e in enumerate(edges) if e[2] not in (NONE, HISTORY)]
    early = n - int(sum(1 for f in fixed if f)) > len(used)
    reg = [edges[k][0] for k in used if edges[k][2] == REGISTRATION]
    with_reg, m = len(reg) > 0, (min(reg) if reg else 0)
    stable_index = m if with_reg else 0
    cls, lim = np.zeros(n, np.int32), np.zeros((n, 2))
    for i in range(n):
        if (with_reg and i <= m) or fixed[i]:
            continue
        if p["free_all_nodes"]:
            cls[i] = 2
            continue
        f = 1.0
        if stable[i]:
            stable_index = i
        else:
            f = float(i - stable_index)
        cls[i] = 1
        lim[i] = f * p["t_limit"], f * p["r_limit"]
    return used, early, cls, lim


def weight_matrix(info, p):
    W = np.zeros((6, 6))
    if p["use_equal_weight"]:
        r = float(np.float32(p["quat_tran_ratio"]))
        W[np.arange(6), np.arange(6)] = [1.0, 1.0, 1.0, r * r, r * r, r * r]
    elif p["use_diagonal_information_matrix"]:
        W[np.arange(6), np.arange(6)] = np.diag(info)
    else:
        W = 0.5 * (info + info.T)
    return W


# ---- the block skyline solve ----
def skyline(unk, used_ab, U):
    first = list(range(U))
    for a, b in used_ab:
        ua, ub = unk[a], unk[b]
        if ua < 0 or ub < 0:
            continue
        first[max(ua, ub)] = min(first[max(ua, ub)], min(ua, ub))
    colmax = list(range(U))
    for u in range(U):
        for j in range(first[u], u):
            colmax[j] = u
    return first, colmax


def cholesky_solve(A, g, first, colmax, U):
    """A: dict (i, j) -> 6 x 6 block of H + D, j in first[i] .. i.  -> delta (6 U) or None when a pivot is not positive and finite"""
    L = {}
    with np.errstate(all="ignore"):
        for j in range(U):
            rows = [i for i in range(j, colmax[j] + 1) if first[i] <= j]
            S = {}
            for i in rows:
                s = A[(i, j)].copy()
                for k in range(max(first[i], first[j]), j):
                    s = s - dot6(L[(i, k)][:, None, :], L[(j, k)][None, :, :], 2, 2)
                S[i] = s
            D = S[j]
            Ljj = np.zeros((6, 6))
            for c in range(6):
                for r in range(c, 6):
                    x = D[r, c]
                    for m in range(c):
                        x = x - Ljj[r, m] * Ljj[c, m]
                    if r == c:
                        if not (x > 0.0) or not np.isfinite(x):
                            return None
                        Ljj[c, c] = np.sqrt(x)
                    else:
                        Ljj[r, c] = x / Ljj[c, c]
            L[(j, j)] = Ljj
            for i in rows[1:]:
                s, l = S[i], np.zeros((6, 6))
                for c in range(6):
                    x = s[:, c].copy()
                    for m in range(c):
                        x = x - l[:, m] * Ljj[c, m]
                    l[:, c] = x / Ljj[c, c]
                L[(i, j)] = l
        y = (-g).reshape(U, 6).copy()
        for j in range(U):
            Ljj = L[(j, j)]
            for r in range(6):
                x = y[j, r]
                for m in range(r):
                    x = x - Ljj[r, m] * y[j, m]
                y[j, r] = x / Ljj[r, r]
            for i in range(j + 1, colmax[j] + 1):
                if first[i] <= j:
                    y[i] = y[i] - dot6(L[(i, j)], y[j][None, :], 1, 1)
        for k in range(U - 1, -1, -1):
            Lkk = L[(k, k)]
            for r in range(5, -1, -1):
                x = y[k, r]
                for m in range(r + 1, 6):
                    x = x - Lkk[m, r] * y[k, m]
                y[k, r] = x / Lkk[r, r]
            for j in range(first[k], k):
                y[j] = y[j] - dot6(L[(k, j)], y[k][:, None], 0, 0)
    return y.reshape(-1)


def check_edges(poses, edges, p):
    t_thre = float(np.float32(p["wrong_edge_translation_thre"]))
    r_thre = float(np.float32(p["wrong_edge_rotation_thre"])) / 180.0 * math.pi
    wrong = np.zeros(len(edges), np.uint8)
    n_wrong = correct_reg = checked = 0
    for k, (a, b, typ, T, _) in enumerate(edges):
        if typ not in (REGISTRATION, ADJACENT):
            continue
        checked += 1
        A, B = poses[a], poses[b]
        d = B[:3, 3] - A[:3, 3]
        R, t = np.empty((3, 3)), np.empty(3)
        for r in range(3):
            for c in range(3):
                R[r, c] = (A[0, r] * B[0, c] + A[1, r] * B[1, c]) + A[2, r] * B[2, c]
            t[r] = (A[0, r] * d[0] + A[1, r] * d[1]) + A[2, r] * d[2]
        dd = T[:3, 3] - t
        Rd, td = np.empty((3, 3)), np.empty(3)
        for r in range(3):
            for c in range(3):
                Rd[r, c] = (R[0, r] * T[0, c] + R[1, r] * T[1, c]) + R[2, r] * T[2, c]
            td[r] = (R[0, r] * dd[0] + R[1, r] * dd[1]) + R[2, r] * dd[2]
        q = rot2quat(Rd)
        tn = np.sqrt((td[0] * td[0] + td[1] * td[1]) + td[2] * td[2])
        vn = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        ang = 2.0 * math.atan2(vn, abs(q[3]))
        if tn > t_thre or ang > r_thre:
            n_wrong += 1
            wrong[k] = 1
        elif typ == REGISTRATION:
            correct_reg += 1
    with np.errstate(all="ignore"):
        ratio = np.float64(n_wrong) / np.float64(checked)
    ok = not (ratio > float(np.float32(p["wrong_edge_ratio_thre"])) or correct_reg == 0)
    return wrong, n_wrong, correct_reg, int(ok)


def solve(poses, fixed, stable, edges, p=None, check_systems=False):
    """poses (n, 4, 4); fixed, stable (n,); edges: list of (a, b, type, T (4, 4), info (6, 6)); p: params().
    check_systems: every linear system solved is also assembled densely, and |(H + D) delta + g| / (|H + D|_2 |delta| + |g|) goes to solve_residuals"""
    p = p or params()
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    n = len(poses)
    used, early, cls, lim = classify(fixed, stable, edges, p)
    out = dict(status=1, termination=TERM_NOT_RUN, iterations=0, successful_steps=0, n_free=0, n_boxed=0, n_fixed=0, n_edges_used=len(used),
               initial_cost=0.0, final_cost=0.0, min_ratio_distance=np.inf, max_box_excess=-np.inf, solve_residuals=[])

    def finish(P):
        out["poses"] = P
        out["edge_wrong"], out["wrong_edges"], out["correct_reg_edges"], out["edges_ok"] = check_edges(P, edges, p)
        return out

    if early:
        out["status"] = -1
        return finish(poses.copy())
    out["n_fixed"], out["n_boxed"], out["n_free"] = int((cls == 0).sum()), int((cls == 1).sum()), int((cls == 2).sum())
    if n == 0:
        out["termination"] = TERM_NO_FREE
        return finish(poses.copy())
    X0 = np.stack([pose2state(T) for T in poses])
    X = X0.copy()
    E = len(used)
    ea = np.array([edges[k][0] for k in used], np.int64)
    eb = np.array([edges[k][1] for k in used], np.int64)
    es = [pose2state(edges[k][3]) for k in used]
    th = np.array([s[:3] for s in es]).reshape(E, 3)
    qh = np.array([s[3:] for s in es]).reshape(E, 4)
    W = np.array([weight_matrix(np.asarray(edges[k][4], np.float64).reshape(6, 6), p) for k in used]).reshape(E, 6, 6)
    robustify, delta = int(p["robustify"]), float(np.float32(p["robust_delta"]))
    node = [i for i in range(n) if cls[i] != 0]
    unk = -np.ones(n, np.int64)
    unk[node] = np.arange(len(node))
    U = len(node)
    adj = [[] for _ in range(n)]
    for k in range(E):
        adj[ea[k]].append(k)
        adj[eb[k]].append(k)
    first, colmax = skyline(unk, list(zip(ea, eb)), U)

    with np.errstate(all="ignore"):
        lin = linearise(X, ea, eb, th, qh, W, robustify, delta)
        cost = 0.5 * tree_sum(lin[0])
    out["initial_cost"] = out["final_cost"] = float(cost)
    if not np.isfinite(cost):
        out["status"] = -2
        return finish(poses.copy())
    radius, nu, iterations, relin = 1e4, 2.0, 0, False
    while True:
        if U == 0:
            out["termination"] = TERM_NO_FREE
            break
        if iterations >= p["num_iterations"]:
            out["termination"] = TERM_MAX_ITERATIONS
            break
        with np.errstate(all="ignore"):
            if relin:
                lin = linearise(X, ea, eb, th, qh, W, robustify, delta)
            _, Haa, Hab, Hbb, ga, gb = lin
            g = np.zeros((U, 6))
            A, diag = {}, np.zeros((U, 6))
            for ui in range(U):
                i = node[ui]
                for k in adj[i]:
                    g[ui] = g[ui] + (ga[k] if ea[k] == i else gb[k])
                for uj in range(first[ui], ui + 1):
                    j = node[uj]
                    acc = np.zeros((6, 6))
                    for k in adj[i]:
                        i_is_a = ea[k] == i
                        if ui == uj:
                            acc = acc + (Haa[k] if i_is_a else Hbb[k])
                        elif (eb[k] if i_is_a else ea[k]) == j:
                            acc = acc + (Hab[k] if i_is_a else Hab[k].T)
                    if ui == uj:
                        h = np.diag(acc).copy()
                        lo = np.where(h > 1e-6, h, 1e-6)
                        d = np.where(lo < 1e32, lo, 1e32) / radius
                        diag[ui] = d
                        acc[np.arange(6), np.arange(6)] = h + d
                    A[(ui, uj)] = acc
            g = g.reshape(-1)
            gmax = absmax(g)
            if gmax <= 1e-10:
                out["termination"] = TERM_GRADIENT
                break
            iterations += 1
            dl = cholesky_solve(A, g, first, colmax, U)
            ok, rr = False, 0.0
            if dl is not None:
                if check_systems:
                    M = np.zeros((6 * U, 6 * U))
                    for (bi, bj), blk in A.items():
                        if bi == bj:
                            low = np.tril(blk)
                            M[6 * bi:6 * bi + 6, 6 * bj:6 * bj + 6] = low + np.tril(blk, -1).T
                        else:
                            M[6 * bi:6 * bi + 6, 6 * bj:6 * bj + 6] = blk
                            M[6 * bj:6 * bj + 6, 6 * bi:6 * bi + 6] = blk.T
                    out["solve_residuals"].append(float(np.linalg.norm(M @ dl + g) / (np.abs(np.linalg.eigvalsh(M)).max() * np.linalg.norm(dl) + np.linalg.norm(g))))
                if absmax(dl) <= 1e-8:
                    out["termination"] = TERM_STEP
                    break
                C = X.copy()
                for ui in range(U):
                    i = node[ui]
                    C[i], raw = step_node(X[i], dl[6 * ui:6 * ui + 6], X0[i], cls[i] == 1, lim[i, 0], lim[i, 1], p["only_limit_translation"])
                    if raw is not None:
                        out["max_box_excess"] = max(out["max_box_excess"], float(np.max(np.abs(raw - X0[i, 3:7]) - lim[i, 1])))
                cp = 0.5 * tree_sum(edge_terms(C, ea, eb, th, qh, W, robustify, delta))
                md = -0.5 * tree_sum(dl * (g - diag.reshape(-1) * dl))
                if np.isfinite(cp) and md > 0.0:
                    rr = (cost - cp) / md
                    ok = bool(rr > 1e-3)
                    out["min_ratio_distance"] = min(out["min_ratio_distance"], abs(float(rr) - 1e-3))
            if ok:
                old = cost
                u = 2.0 * rr - 1.0
                f = 1.0 - (u * u) * u
                third = 1.0 / 3.0
                rad = radius / (third if third > f else f)
                radius = rad if rad < 1e16 else 1e16
                nu = 2.0
                X, cost, relin = C, cp, True
                out["successful_steps"] += 1
                if abs(old - cp) <= p["function_tolerance"] * old:
                    out["termination"] = TERM_FUNCTION_TOLERANCE
                    break
            else:
                radius = radius / nu
                nu = 2.0 * nu
                relin = False
                if radius < 1e-32:
                    out["termination"] = TERM_RADIUS
                    break
    out["iterations"], out["final_cost"] = iterations, float(cost)
    return finish(np.stack([state2pose(x) for x in X]))
