"""The definition of mulls_coarse_reg_teaser (include/mulls_hip.h) restated in numpy, written from that text and not from the C++:
the test reference of tests/test_teaser.py (CPU: the product's own host code and arithmetic, built for the CPU) and tests/test_gpu_teaser.py (the device).

Elementwise operations only on the defined sums (no np.dot, no np.sum): the 4096 strided partial sums are one vector, added to step by step, and the
pairwise tree halves it.  The graph is built in row blocks.  The maximum clique comes from another algorithm than the product's (a Bron-Kerbosch
enumeration of all maximal cliques with a pivot and a size cut, then the smallest list), so the lexicographic rule is checked and not copied.

TEASER++ is not available where these tests run: nothing here was compared with TEASER++ itself."""
import sys

import numpy as np

PARTIALS = 4096
MAX_ITER, FACTOR, COST_THRESHOLD = 100, 1.4, 0.005
F = np.float64


# ------------------------------------------------------------------------------------------------------------------------------------ graph and clique
def graph(t, s, noise_bound, block=256):
    """bool (N, N): edge {i, j} iff | |s_j - s_i| - |t_j - t_i| | <= 2 noise_bound sqrt(1); NaN: no edge; no diagonal"""
    n = len(t)
    S, T = s[:, :3].astype(F), t[:, :3].astype(F)
    beta = (F(2.0) * F(np.float32(noise_bound))) * np.sqrt(F(1.0))
    adj = np.zeros((n, n), bool)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, block):
            d = []
            for Pn in (S, T):
                dx, dy, dz = (Pn[None, :, k] - Pn[i0:i0 + block, None, k] for k in range(3))
                d.append(np.sqrt((dx * dx + dy * dy) + dz * dz))
            adj[i0:i0 + block] = np.abs(d[0] - d[1]) <= beta
    adj[np.arange(n), np.arange(n)] = False
    return adj


def core_numbers(adj):
    n = len(adj)
    deg = adj.sum(1).astype(np.int64)
    alive = np.ones(n, bool)
    core = np.zeros(n, np.int64)
    k = 0
    big = n + 1
    for _ in range(n):
        v = int(np.argmin(np.where(alive, deg, big)))
        k = max(k, int(deg[v]))
        core[v] = k
        alive[v] = False
        deg[adj[v] & alive] -= 1
    return core


def maximum_cliques(adj):
    """every maximum clique as a sorted list (Bron-Kerbosch with a pivot; a branch that cannot reach the best size so far is cut)"""
    n = len(adj)
    nb = [set(np.flatnonzero(adj[i]).tolist()) for i in range(n)]
    best, found = [1 if n else 0], [[i] for i in range(n)] if not adj.any() else []
    if found:
        return found
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 3 * n + 1000))

    def bk(R, Pc, X):
        if len(R) + len(Pc) < best[0]:
            return
        if not Pc:
            if not X:
                if len(R) > best[0]:
                    best[0] = len(R)
                    del found[:]
                if len(R) == best[0]:
                    found.append(sorted(R))
            return
        u = max(Pc | X, key=lambda x: len(nb[x] & Pc))
        for v in sorted(Pc - nb[u]):
            bk(R + [v], Pc & nb[v], X & nb[v])
            Pc.discard(v)
            X.add(v)

    core = core_numbers(adj)
    order = sorted(range(n), key=lambda v: (-core[v], v))  # dense part first: the cut bites early
    seen = set()
    for v in order:
        bk([v], nb[v] - seen, nb[v] & seen)
        seen.add(v)
    return found


def smallest_maximum_clique(adj):
    return min(maximum_cliques(adj))


# ------------------------------------------------------------------------------------------------------------------------------------------- rotation
def horn_rot(H):
    """Horn's 4 x 4 of H (H[a][b] = sum w s_a t_b), ten cyclic Jacobi sweeps, largest diagonal entry's column as a unit quaternion, R (3, 3)"""
    with np.errstate(all="ignore"):
        H = [F(v) for v in np.asarray(H, F).reshape(9)]
        Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = H
        A = [[F(0)] * 4 for _ in range(4)]
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
        V = [[F(1) if r == c else F(0) for c in range(4)] for r in range(4)]
        for _ in range(10):
            for p in range(3):
                for q in range(p + 1, 4):
                    apq = A[p][q]
                    if apq == 0.0:
                        continue
                    theta = (A[q][q] - A[p][p]) / (F(2) * apq)
                    t = F(1) / (np.abs(theta) + np.sqrt(theta * theta + F(1)))
                    if theta < 0.0:
                        t = -t
                    c = F(1) / np.sqrt(t * t + F(1))
                    s = t * c
                    for k in range(4):
                        akp, akq = A[k][p], A[k][q]
                        A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
                    for k in range(4):
                        apk, aqk = A[p][k], A[q][k]
                        A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
                    for k in range(4):
                        vkp, vkq = V[k][p], V[k][q]
                        V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
        j = 0
        for k in range(1, 4):
            if A[k][k] > A[j][j]:
                j = k
        q0, qx, qy, qz = V[0][j], V[1][j], V[2][j], V[3][j]
        nrm = np.sqrt(((q0 * q0 + qx * qx) + qy * qy) + qz * qz)
        q0, qx, qy, qz = q0 / nrm, qx / nrm, qy / nrm, qz / nrm
        q00, qxx, qyy, qzz = q0 * q0, qx * qx, qy * qy, qz * qz
        qxy, qxz, qyz, q0x, q0y, q0z = qx * qy, qx * qz, qy * qz, q0 * qx, q0 * qy, q0 * qz
        two = F(2)
        return np.array([[((q00 + qxx) - qyy) - qzz, two * (qxy - q0z), two * (qxz + q0y)],
                         [two * (qxy + q0z), ((q00 - qxx) + qyy) - qzz, two * (qyz - q0x)],
                         [two * (qxz - q0y), two * (qyz + q0x), ((q00 - qxx) - qyy) + qzz]], F)


def strided_tree_sum(terms):
    """4096 partial sums (partial p adds terms p, p + 4096, ... ascending, from 0), then p[t] += p[t + s], s = 2048 .. 1"""
    m = len(terms)
    steps = -(-m // PARTIALS) if m else 0
    pad = np.zeros(steps * PARTIALS, F)
    pad[:m] = terms  # (a partial never is -0.0, so a +0.0 behind the end changes nothing)
    acc = np.zeros(PARTIALS, F)
    for row in pad.reshape(steps, PARTIALS):
        acc = acc + row
    s = PARTIALS // 2
    while s:
        acc = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


def residuals(R, a, b):
    d = [b[:, r] - ((R[r, 0] * a[:, 0] + R[r, 1] * a[:, 1]) + R[r, 2] * a[:, 2]) for r in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def gnc(cs, ct, noise_bound):
    """cs, ct: (C, 3) float32 clique points.  Returns R, cost, iterations, the exit (1: mu <= 0, 2: cost, 0: the limit) and the rotation inlier count"""
    C = len(cs)
    ia, ib = np.triu_indices(C, 1)  # a < b, a outer, b inner
    S, T = cs.astype(F), ct.astype(F)
    a, b = S[ib] - S[ia], T[ib] - T[ia]
    nb = F(np.float32(noise_bound))
    nb2 = nb * nb
    if nb2 < 1e-16:
        nb2 = F(1e-2)
    w = np.ones(len(ia), F)
    prev, cost, mu, stop, it = F(np.inf), F(0.0), F(0.0), 0, 0
    with np.errstate(all="ignore"):
        for it in range(MAX_ITER):
            H = [strided_tree_sum((w * a[:, p]) * b[:, q]) for p in range(3) for q in range(3)]
            R = horn_rot(H)
            r = residuals(R, a, b)
            if it == 0:
                mu = F(1.0) / ((F(2.0) * r.max()) / nb2 - F(1.0))
                if mu <= 0:
                    stop = 1
                    break
            cost = strided_tree_sum(w * r)
            th1, th2 = ((mu + F(1)) / mu) * nb2, (mu / (mu + F(1))) * nb2
            mid = np.sqrt(((nb2 * mu) * (mu + F(1))) / r) - mu
            w = np.where(r >= th1, F(0), np.where(r <= th2, F(1), mid))
            if np.abs(cost - prev) < COST_THRESHOLD:
                stop = 2
                break
            mu, prev = F(FACTOR) * mu, cost
    return R, cost, it + 1, stop, int((w >= 0.5).sum())


# ---------------------------------------------------------------------------------------------------------------------------------------- translation
def tls(x, rng):
    """TEASER's scalar TLS estimate with one range"""
    x = np.asarray(x, F)
    rng = F(rng)
    ends = sorted([(x[i] - rng, 0, i) for i in range(len(x))] + [(x[i] + rng, 1, i) for i in range(len(x))], key=lambda e: (e[0], e[1], e[2])) \
        if not np.isnan(x).any() else sorted([(F(0), c, i) for i in range(len(x)) for c in (0, 1)], key=lambda e: (e[1], e[2]))
    with np.errstate(all="ignore"):
        w = F(1.0) / (rng * rng)
        excluded = F(0.0)
        for _ in range(len(x)):
            excluded = excluded + rng
        sw = swx = swx2 = F(0.0)
        best, est = F(np.inf), F(0.0)
        for _, closing, i in ends:
            wx = w * x[i]
            if not closing:
                sw, swx, swx2, excluded = sw + w, swx + wx, swx2 + wx * x[i], excluded - rng
            else:
                sw, swx, swx2, excluded = sw - w, swx - wx, swx2 - wx * x[i], excluded + rng
            xhat = swx / sw
            cost = (((sw * xhat) * xhat + swx2) - (F(2.0) * swx) * xhat) + excluded
            if cost < best:
                best, est = cost, xhat
    return est


def translation(cs, ct, R, noise_bound):
    S, T = cs.astype(F), ct.astype(F)
    rng = F(np.float32(noise_bound))
    x = [T[:, a] - ((R[a, 0] * S[:, 0] + R[a, 1] * S[:, 1]) + R[a, 2] * S[:, 2]) for a in range(3)]
    that = np.array([tls(x[a], rng) for a in range(3)], F)
    with np.errstate(all="ignore"):
        inl = (np.abs(x[0] - that[0]) <= rng) & (np.abs(x[1] - that[1]) <= rng) & (np.abs(x[2] - that[2]) <= rng)
    return that, int(inl.sum())


# ------------------------------------------------------------------------------------------------------------------------------------------- the call
def restate(t, s, noise_bound=0.2, min_inlier_num=8):
    """t, s: (N, >= 3) float32 target / source points, pair i = row i of each.  The result fields of mulls_teaser_result that the definition fixes."""
    out = dict(status=-1, n_edges=0, max_core=0, clique_size=0, clique_exact=1, gnc_iterations=0, n_rotation_inliers=0, n_translation_inliers=0,
               cost=0.0, T=np.eye(4), clique=np.zeros(0, np.int64), gnc_exit=-1, n_maximum_cliques=0)
    if len(t) != len(s) or len(t) <= 3:
        return out
    adj = graph(t, s, noise_bound)
    out["n_edges"] = int(adj.sum()) // 2
    out["max_core"] = int(core_numbers(adj).max())
    cliques = maximum_cliques(adj)
    clique = np.array(min(cliques), np.int64)
    out["n_maximum_cliques"] = len(cliques)
    out["clique"], out["clique_size"] = clique, len(clique)
    if len(clique) <= 1:
        out["clique"] = clique[:1]
        return out
    cs, ct = s[clique, :3], t[clique, :3]
    R, cost, iters, stop, n_rot = gnc(cs, ct, noise_bound)
    if stop == 1:
        n_rot = len(clique) * (len(clique) - 1) // 2
    that, n_tr = translation(cs, ct, R, noise_bound)
    out.update(gnc_iterations=iters, n_rotation_inliers=n_rot, n_translation_inliers=n_tr, cost=float(cost), gnc_exit=stop)
    out["status"] = 1 if n_rot >= 2 * min_inlier_num else (0 if n_rot >= min_inlier_num else -1)
    if out["status"] >= 0:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, that
        out["T"] = T
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------ input sets
def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def planted(seed, n, outlier_share, noise_bound=0.2, box=60.0, noise=0.1):
    """n pairs, round(n (1 - outlier_share)) of them one rigid motion with at most noise * noise_bound of uniform noise per axis, the rest unrelated points
    of the box.  Returns t, s (n, 4) float32, the 4 x 4 motion and the planted mask; the pairs are shuffled."""
    rng = np.random.default_rng(seed)
    n_in = int(round(n * (1.0 - outlier_share)))
    R, tr = rotation(rng), rng.uniform(-10, 10, 3)
    s = rng.uniform(-box, box, (n, 3))
    t = rng.uniform(-box, box, (n, 3))
    t[:n_in] = s[:n_in] @ R.T + tr + rng.uniform(-noise * noise_bound, noise * noise_bound, (n_in, 3))
    order = rng.permutation(n)
    mask = np.zeros(n, bool)
    mask[:n_in] = True
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, tr
    pad = rng.uniform(0, 5, (n, 1))
    return (np.concatenate([t, pad], 1).astype(np.float32)[order], np.concatenate([s, pad], 1).astype(np.float32)[order], T, mask[order])


def complete(seed, n, noise_bound=0.2):
    """every pair consistent: one motion, small noise"""
    return planted(seed, n, 0.0, noise_bound)[:2]


def two_cliques(seed=3, k=6):
    """two disjoint consistent groups of k pairs (two motions), far apart: two maximum cliques of equal size; the smaller list must win"""
    a, b = planted(seed, k, 0.0, 0.2, box=20.0), planted(seed + 1, k, 0.0, 0.2, box=20.0)
    t = np.concatenate([b[0], a[0]])
    s = np.concatenate([b[1] + np.float32(500.0), a[1]])  # (the shift keeps the groups' mutual distances inconsistent)
    return t, s


PLANTED = [(40, 0.5), (40, 0.9), (200, 0.5), (200, 0.9), (1000, 0.5), (1000, 0.9)]
EDGE_SIZES = [31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4097, 8192]


def min_inlier(name):
    """min_inlier_num of a set: 3 for the planted ones (four planted pairs are six measurements: status 1 needs 2 min_inlier_num of them), else the default"""
    return 3 if name.startswith("planted_") else 8


def planted_seed(n, share):
    return 1000 + n + int(100 * share)


def input_sets(demo=None):
    """{name: (t, s, noise_bound)}: everything the fixture pins"""
    out = {}
    for n, share in PLANTED:
        t, s, _, _ = planted(planted_seed(n, share), n, share)
        out["planted_%d_%d" % (n, int(100 * share))] = (t, s, 0.2)
    for n in EDGE_SIZES:
        share = 0.5 if n < 100 else 1.0 - 24.0 / n  # a planted clique of 24 among sparse outliers
        t, s, _, _ = planted(2000 + n, n, share, box=100.0)
        out["size_%d" % n] = (t, s, 0.2)
    t, s = complete(7, 300)
    out["complete_300"] = (t, s, 0.2)
    t, s = two_cliques()
    out["two_cliques"] = (t, s, 0.2)
    rng = np.random.default_rng(11)
    t, s = rng.uniform(-100, 100, (40, 4)).astype(np.float32), rng.uniform(-1, 1, (40, 4)).astype(np.float32)
    s[:, :3] = (np.arange(40)[:, None] * 1000.0 + s[:, :3]).astype(np.float32)  # source points 1 km apart, targets within 350 m: no edge
    out["no_edge"] = (t, s, 0.2)
    t2, s2 = t.copy(), s.copy()
    t2[5, :3], t2[9, :3] = (0, 0, 0), (4000.05, 0, 0)  # |s_9 - s_5| is 4000 +- 2: made consistent below
    s2[5, :3], s2[9, :3] = (5000, 0, 0), (9000, 0, 0)
    out["single_edge"] = (t2, s2, 0.2)
    t, s = planted(31, 60, 0.5)[:2]
    out["exit_mu"] = (t, s.copy(), 0.2)
    t, s, T, m = planted(32, 60, 0.5, noise=0.0)
    out["exit_mu_exact"] = (t, s, 0.2)
    t, s = planted(33, 80, 0.5, noise_bound=0.2, noise=0.9)[:2]
    out["exit_cost"] = (t, s, 0.2)
    rng = np.random.default_rng(34)
    s, t = rng.uniform(-5e5, 5e5, (12, 4)).astype(np.float32), rng.uniform(-5e5, 5e5, (12, 4)).astype(np.float32)
    # nine unrelated pairs inside a box smaller than the bound (all consistent, none fitted: residuals of the bound's order) and three far pairs that
    # are a mirror image of each other: every distance kept, no rotation fits, max r / nb2 about 10^16, so mu stays below 1 for all 100 iterations
    s[9:, :3] = np.diag([1e14, 1e14, 1e14])
    t[9:, :3] = np.diag([1e14, 1e14, -1e14])
    out["exit_limit"] = (t, s, 1e6)
    t, s = planted(41, 64, 0.5)[:2]
    for k, v in ((3, np.nan), (10, np.inf), (20, -np.inf)):
        t[k, 0] = v
        s[k + 1, 2] = v
    out["nonfinite_64"] = (t, s, 0.2)
    if demo is not None:
        for name in DEMO_LISTS:
            a, b = (0, 15) if name.endswith("0_15") else (15, 0)
            pr = demo[name + "_pairs"]
            kt, ks = xyzw_of(demo["kpts_%d" % a]), xyzw_of(demo["kpts_%d" % b])
            for nb in (0.25, 1.0):
                out["demo_%s_nb%d" % (name, int(100 * nb))] = (kt[pr[:, 0]], ks[pr[:, 1]], nb)
    return out


DEMO_LISTS = ["recip_0_15", "recip_15_0", "fixed300_0_15", "fixed300_15_0"]


def xyzw_of(raw):
    """x, y, z, data[3] of (n, 48) byte records"""
    return np.ascontiguousarray(raw[:, :16]).view(np.float32).reshape(-1, 4).copy()


def records(xyzw):
    raw = np.zeros((len(xyzw), 48), np.uint8)
    raw[:, :16] = np.ascontiguousarray(xyzw[:, :4], np.float32).view(np.uint8).reshape(-1, 16)
    return raw
