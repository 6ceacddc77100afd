"""numpy restatement of mulls_coarse_reg_ransac's definition (include/mulls_hip.h), written from that text and independent of the C++:
the test reference of tests/test_ransac.py and tests/test_gpu_ransac.py.

numpy's separate elementwise + - * / sqrt on float32 / float64 arrays are correctly rounded and never fused, so an expression written in the defined order
has the device's bits.  The hypotheses are built and scored as arrays (in chunks, only as far as the sequential rule reads); the draws and the refinement's
control flow are plain loops.  Also here: the seeded generators of the test inputs."""
import math

import numpy as np

RT = 256  # partial sums of a refinement fit (part of the definition)
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- generator and draws
class MT19937:
    """std::mt19937 (Matsumoto & Nishimura 1998; init_genrand seeding)"""

    def __init__(self, seed=5489):
        mt = [seed & 0xFFFFFFFF]
        for i in range(1, 624):
            mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & 0xFFFFFFFF)
        self.mt, self.at = mt, 624

    def _twist(self):
        mt = self.mt
        for i in range(624):
            y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        self.at = 0

    def __call__(self):
        if self.at >= 624:
            self._twist()
        y = self.mt[self.at]
        self.at += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        return y ^ (y >> 18)


def jacobi3_eigenvalues(a6):
    """the diagonal a cyclic Jacobi on the upper triangle leaves (double; Python floats are IEEE doubles, math.sqrt is correctly rounded)"""
    A = [[a6[0], a6[1], a6[2]], [a6[1], a6[3], a6[4]], [a6[2], a6[4], a6[5]]]
    for _ in range(60):
        off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2]
        if off < 1e-300:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if A[p][q] == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                cs = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * cs
                for k in range(3):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p], A[k][q] = cs * akp - sn * akq, sn * akp + cs * akq
                for k in range(3):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k], A[q][k] = cs * apk - sn * aqk, sn * apk + cs * aqk
                for r in range(3):
                    for c in range(r + 1, 3):
                        A[c][r] = A[r][c]
    return A[0][0], A[1][1], A[2][2]


def sample_dist_thresh(src):
    """(mean of the square roots of the eigenvalues of the source's covariance)^2; the covariance from float raw moments summed in index order"""
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    with np.errstate(all="ignore"):
        terms = [x * x, x * y, x * z, y * y, y * z, z * z, x, y, z]
        acc = [np.add.accumulate(np.concatenate([np.zeros(1, F32), t.astype(F32)]), dtype=F32)[-1] / F32(len(src)) for t in terms]
        cov = [acc[0] - acc[6] * acc[6], acc[1] - acc[6] * acc[7], acc[2] - acc[6] * acc[8], acc[3] - acc[7] * acc[7], acc[4] - acc[7] * acc[8],
               acc[5] - acc[8] * acc[8]]
    lam = jacobi3_eigenvalues([float(c) for c in cov])
    rt = [math.sqrt(v) if v >= 0 else float("nan") for v in lam]
    th = ((rt[0] + rt[1]) + rt[2]) / 3.0
    return th * th


def fisher_yates_draw(eng, shuffled):
    n = len(shuffled)
    for i in range(3):
        j = i + (eng() >> 1) % (n - i)
        shuffled[i], shuffled[j] = shuffled[j], shuffled[i]
    return shuffled[0], shuffled[1], shuffled[2]


def draws(src, want):
    """the sample of every iteration up to `want`; fewer when 1000 draws in a row are not good"""
    n = len(src)
    thresh = sample_dist_thresh(src)
    eng, shuffled, out = MT19937(12345), list(range(n)), []
    P = np.ascontiguousarray(src, F32)
    for _ in range(want):
        good = False
        for _ in range(1000):
            a, b, c = fisher_yates_draw(eng, shuffled)
            with np.errstate(all="ignore"):
                d = P[[b, c, c]] - P[[a, a, b]]
                q = d * d
                v = (q[:, 0] + q[:, 2]) + (q[:, 1] + q[:, 3])
            good = bool((v.astype(np.float64) > thresh).all())
            if good:
                break
        if not good:
            break
        out.append((a, b, c))
    return np.array(out, np.int64).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------- the estimator
def horn(H, cs, ct):
    """H (M, 9), cs / ct (M, 3), double -> (M, 12) float32: Horn's 4 x 4, ten cyclic Jacobi sweeps, unit quaternion, R, t = ct - R cs"""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (H[:, k] for k in range(9))
    M = len(H)
    A = [[None] * 4 for _ in range(4)]
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
    V = [[np.full(M, 1.0 if r == c else 0.0) for c in range(4)] for r in range(4)]
    with np.errstate(all="ignore"):
        for _ in range(10):
            for p in range(3):
                for q in range(p + 1, 4):
                    apq = A[p][q]
                    skip = apq == 0.0
                    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                    t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    t = np.where(theta < 0.0, -t, t)
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    for k in range(4):
                        akp, akq = A[k][p], A[k][q]
                        A[k][p], A[k][q] = np.where(skip, akp, c * akp - s * akq), np.where(skip, akq, s * akp + c * akq)
                    for k in range(4):
                        apk, aqk = A[p][k], A[q][k]
                        A[p][k], A[q][k] = np.where(skip, apk, c * apk - s * aqk), np.where(skip, aqk, s * apk + c * aqk)
                    for k in range(4):
                        vkp, vkq = V[k][p], V[k][q]
                        V[k][p], V[k][q] = np.where(skip, vkp, c * vkp - s * vkq), np.where(skip, vkq, s * vkp + c * vkq)
        best, qv = A[0][0], [V[r][0] for r in range(4)]
        for k in range(1, 4):
            up = A[k][k] > best
            best = np.where(up, A[k][k], best)
            qv = [np.where(up, V[r][k], qv[r]) for r in range(4)]
        q0, qx, qy, qz = qv
        nrm = np.sqrt(((q0 * q0 + qx * qx) + qy * qy) + qz * qz)
        q0, qx, qy, qz = q0 / nrm, qx / nrm, qy / nrm, qz / nrm
        q00, qxx, qyy, qzz = q0 * q0, qx * qx, qy * qy, qz * qz
        qxy, qxz, qyz, q0x, q0y, q0z = qx * qy, qx * qz, qy * qz, q0 * qx, q0 * qy, q0 * qz
        R = [[((q00 + qxx) - qyy) - qzz, 2.0 * (qxy - q0z), 2.0 * (qxz + q0y)],
             [2.0 * (qxy + q0z), ((q00 - qxx) + qyy) - qzz, 2.0 * (qyz - q0x)],
             [2.0 * (qxz - q0y), 2.0 * (qyz + q0x), ((q00 - qxx) - qyy) + qzz]]
        out = np.zeros((M, 12), F32)
        for r in range(3):
            tr = ct[:, r] - ((R[r][0] * cs[:, 0] + R[r][1] * cs[:, 1]) + R[r][2] * cs[:, 2])
            for c in range(3):
                out[:, r * 4 + c] = R[r][c].astype(F32)
            out[:, r * 4 + 3] = tr.astype(F32)
    return out


def models(src, tgt, triples):
    """the hypotheses of the sample triples: float centroids and H in the samples' order, then horn()"""
    s, t = src[triples][:, :, :3].astype(F32), tgt[triples][:, :, :3].astype(F32)  # (M, 3 samples, 3 axes)
    with np.errstate(all="ignore"):
        cs = ((s[:, 0] + s[:, 1]) + s[:, 2]) / F32(3.0)
        ct = ((t[:, 0] + t[:, 1]) + t[:, 2]) / F32(3.0)
        H = np.zeros((len(triples), 9), np.float64)
        for a in range(3):
            for b in range(3):
                h = [(s[:, k, a] - cs[:, a]) * (t[:, k, b] - ct[:, b]) for k in range(3)]
                H[:, a * 3 + b] = ((h[0] + h[1]) + h[2]).astype(np.float64)
    return horn(H, cs.astype(np.float64), ct.astype(np.float64))


def resid2(m, src, tgt):
    """(M, 12) float models x (N, 4) pairs -> (M, N) float squared distances of T (s, 1) to (t, 1)"""
    m = m.astype(F32)
    sx, sy, sz = (src[:, k].astype(F32)[None, :] for k in range(3))
    with np.errstate(all="ignore"):
        d = []
        for r in range(3):
            p = ((m[:, 4 * r, None] * sx + m[:, 4 * r + 1, None] * sy) + m[:, 4 * r + 2, None] * sz) + m[:, 4 * r + 3, None]
            d.append(p - tgt[:, r].astype(F32)[None, :])
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def threshold(noise_bound):
    nb = float(F32(noise_bound))
    return nb * nb


def strided_tree_sum(vals, mask):
    """sum of vals[i] (N, C doubles) over mask in the defined order: RT strided partial sums in ascending index, then p[t] += p[t + s], s = RT/2 .. 1"""
    n, c = vals.shape
    rows = (n + RT - 1) // RT
    v = np.zeros((rows * RT, c))
    v[:n] = vals
    m = np.zeros(rows * RT, bool)
    m[:n] = mask
    v, m = v.reshape(rows, RT, c), m.reshape(rows, RT)
    acc = np.zeros((RT, c))
    with np.errstate(all="ignore"):
        for r in range(rows):
            acc = np.where(m[r][:, None], acc + v[r], acc)
        s = RT // 2
        while s:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s //= 2
    return acc[0]


def fit(src, tgt, mask):
    """the refinement's estimator: double centroids, double H of the demeaned pairs, horn()"""
    S, T = src[:, :3].astype(np.float64), tgt[:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        cen = strided_tree_sum(np.concatenate([S, T], 1), mask) / float(int(mask.sum()))
        sd, gd = S - cen[None, :3], T - cen[None, 3:]
        H = strided_tree_sum(np.stack([sd[:, r] * gd[:, c] for r in range(3) for c in range(3)], 1), mask)
    return horn(H[None, :], cen[None, :3], cen[None, 3:])[0]


# ---------------------------------------------------------------------------------------------------------------- the sequential rule
def stop_k(best, n):
    w = float(best) * (1.0 / float(n))
    p = 1.0 - math.pow(w, 3.0)
    eps = np.finfo(np.float64).eps
    p = min(1.0 - eps, max(eps, p))
    return math.log(1.0 - 0.99) / math.log(p)


def sequential(count_of, n_hyp, n, max_iter):
    """PCL's loop, one hypothesis at a time -> (iterations, best_iteration)"""
    iterations, best, best_it, k = 0, None, -1, 1.0
    while iterations < k:
        if iterations >= n_hyp:
            break
        c = count_of(iterations)
        if best is None or c > best:
            best, best_it = c, iterations
            k = stop_k(best, n)
        iterations += 1
        if iterations > max_iter:
            break
    return iterations, best_it


def pick(counts, n, max_iter):
    """the order-free form: every count is known; records by a prefix maximum, the first iteration at which the stopping test fires, the last record before it"""
    counts = np.asarray(counts, np.int64)
    if len(counts) == 0:
        return 0, -1
    run = np.maximum.accumulate(counts)
    kk = {int(b): stop_k(int(b), n) for b in np.unique(run)}
    k = np.array([kk[int(b)] for b in run])
    done = np.arange(1, len(counts) + 1)
    stop = ~(done < k) | (done > max_iter)
    stop[-1] = True  # no further sample
    last = int(np.argmax(stop))
    return last + 1, int(np.argmax(counts[: last + 1]))


# ---------------------------------------------------------------------------------------------------------------- the whole call
def restate(tgt, src, noise_bound=0.2, min_inlier_num=8, max_iter_num=20000, refine=1, chunk=None, tri=None):
    """tgt, src: (N, 4) float32 (x, y, z, data[3]).  Returns a dict: status, iterations, best_iteration, refine_iterations, n_inliers, inliers, T (4 x 4
    float64 of the float matrix) and margin: the smallest relative distance of a squared residual of the winning / refined models to its threshold.
    tri: draws(src, m) of an m > max_iter_num computed before (the sequence does not depend on the other arguments)."""
    tgt, src = np.ascontiguousarray(tgt, F32), np.ascontiguousarray(src, F32)
    n = len(tgt)
    assert len(src) == n
    out = dict(status=-1, iterations=0, best_iteration=-1, refine_iterations=0, n_inliers=0, inliers=np.zeros(0, np.int64), T=np.eye(4), margin=np.inf,
               oscillating=False)

    def status_of(cnt):
        return 1 if cnt >= 2 * min_inlier_num else (0 if cnt >= min_inlier_num else -1)

    def pass_through():
        out.update(status=status_of(n), n_inliers=n, inliers=np.arange(n, dtype=np.int64), T=np.eye(4))
        return out

    if n < 3:
        return pass_through()
    thr = threshold(noise_bound)
    want = max(max_iter_num, 0) + 1
    tri = draws(src, want) if tri is None else tri[:want]
    if len(tri) == 0:
        return pass_through()
    chunk = chunk or max(16, min(4096, (1 << 22) // n))
    cache = {}

    def count_of(i):
        c0 = i // chunk
        if c0 not in cache:
            m = models(src, tgt, tri[c0 * chunk:(c0 + 1) * chunk])
            cache[c0] = (m, (resid2(m, src, tgt).astype(np.float64) < thr).sum(1))
        return int(cache[c0][1][i % chunk])

    out["iterations"], best_it = sequential(count_of, len(tri), n, max_iter_num)
    out["best_iteration"] = best_it
    model = cache[best_it // chunk][0][best_it % chunk]

    def select(m, th):
        d2 = resid2(m[None, :], src, tgt)[0].astype(np.float64)
        with np.errstate(all="ignore"):
            out["margin"] = min(out["margin"], float(np.nanmin(np.abs(d2 - th) / th))) if th > 0 and np.isfinite(d2).any() else out["margin"]
        return d2 < th, d2

    mask, _ = select(model, thr)
    if refine:
        error_threshold, sizes = float(F32(noise_bound)), []
        prev, rounds, changed, oscillating, emptied, m = mask, 0, False, False, False, model
        while True:
            m = fit(src, tgt, prev)
            sizes.append(int(prev.sum()))
            new, d2 = select(m, error_threshold * error_threshold)
            rounds += 1
            if not new.any():
                emptied = True
                break
            sel = np.sort(d2[new].astype(F32))
            variance = 2.1981 * float(sel[len(sel) >> 1])
            error_threshold = math.sqrt(min(thr, 9.0 * variance))
            prev, new = new, prev
            if int(new.sum()) != int(prev.sum()):
                if len(sizes) >= 4 and sizes[-1] == sizes[-3] and sizes[-2] == sizes[-4]:
                    oscillating = True
                    break
                changed = True
            else:
                changed = bool((new != prev).any())
            if not (changed and rounds < 1000):
                break
        out["refine_iterations"], out["oscillating"] = rounds, oscillating
        if emptied or (not oscillating and changed):
            return out  # status -1, nothing passes
        if not oscillating:
            mask, model = prev, m
    if int(mask.sum()) < 3:
        return pass_through()
    cnt = int(mask.sum())
    out.update(status=status_of(cnt), n_inliers=cnt, inliers=np.flatnonzero(mask).astype(np.int64))
    if out["status"] >= 0:
        T = np.eye(4)
        T[:3, :] = model.astype(np.float64).reshape(3, 4)
        out["T"] = T
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def records(xyzw):
    """(N, 4) float32 -> (N, 48) uint8 point records: x, y, z, data[3] in the first 16 bytes, the rest zero"""
    raw = np.zeros((len(xyzw), 48), np.uint8)
    raw[:, :16] = np.ascontiguousarray(xyzw, F32).view(np.uint8).reshape(len(xyzw), 16)
    return raw


def xyzw_of(raw):
    return np.ascontiguousarray(raw[:, :16]).view(F32).reshape(len(raw), 4).copy()


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def planted(seed, n, ratio, sigma=0.05):
    """n pairs, a fraction `ratio` of them related by one rigid transform (Gaussian noise sigma on the target), the rest uniform in the scene's box.
    Returns tgt, src (N, 4) float32, the 4 x 4 transform, the planted inlier mask."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-40.0, -40.0, -3.0]), np.array([40.0, 40.0, 10.0])
    src = rng.uniform(lo, hi, (n, 3))
    R = rotation(rng.normal(size=3) * [0.2, 0.2, 1.0], rng.uniform(0.2, 1.2))
    t = rng.uniform([-8, -8, -0.5], [8, 8, 0.5])
    tgt = src @ R.T + t + rng.normal(0, sigma, (n, 3))
    inl = np.zeros(n, bool)
    inl[rng.permutation(n)[: int(round(ratio * n))]] = True
    tgt[~inl] = rng.uniform(lo, hi, (int((~inl).sum()), 3))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    w = rng.uniform(0, 8, (2, n))
    return (np.concatenate([tgt, w[0][:, None]], 1).astype(F32), np.concatenate([src, w[1][:, None]], 1).astype(F32), T, inl)


def coincident(n):
    """every source point the same point: no sample is good"""
    src = np.tile(np.array([[3.0, -2.0, 1.0, 0.5]], F32), (n, 1))
    tgt = np.random.default_rng(n).uniform(-5, 5, (n, 4)).astype(F32)
    return tgt, src


def collinear(seed, n):
    """sources on one line (data[3] too).  Two eigenvalues of their covariance are zero up to rounding; for this generator's seed in input_sets() one of them
    comes out of the float covariance and the Jacobi sweeps slightly NEGATIVE, its square root is NaN, sample_dist_thresh is NaN and no sample is good: the
    pass-through outcome.  That hinges on the sign of a rounding error (with a non-negative one the samples would pass and the fits be rank deficient); the
    fixture pins it."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-30, 30, n)
    src = np.stack([1.0 + 0.6 * u, -2.0 + 0.8 * u, 0.5 + 0.0 * u, 0.1 * u], 1)
    tgt = src + np.array([2.0, 1.0, 0.0, 0.0]) + rng.normal(0, 0.02, (n, 4))
    return tgt.astype(F32), src.astype(F32)


def unrelated(seed, n):
    """two independent uniform clouds: with a small bound no model has three inliers"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-40, 40, (n, 4)).astype(F32), rng.uniform(-40, 40, (n, 4)).astype(F32)


def rotation_angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, c))))


# ---------------------------------------------------------------------------------------------------------------- the sets both test files use
SIZES = (3, 8, 64, 517, 2840, 4097, 65536)
ITERS = (1, 100, 20000)
DEMO_LISTS = ("recip_0_15", "nn_0_15", "fixed2000_0_15", "fixed300_0_15")


def with_nan(tgt, src, in_src):
    tgt, src = tgt.copy(), src.copy()
    (src if in_src else tgt)[[5, 77, 300], [0, 1, 2]] = np.nan
    return tgt, src


def input_sets(demo_npz=None):
    """name -> (tgt, src, noise_bound, the max_iter_num values to run): every input set the GPU tests reuse"""
    sets = {}
    for n in SIZES:
        t, s, _, _ = planted(1000 + n, n, 0.5)  # stops within tens of iterations
        sets["half_%d" % n] = (t, s, 0.5, ITERS)
    for n, seed in ((64, 2064), (517, 2517), (2840, 4842), (4097, 6098)):  # seeds under which the threshold guard of tests/test_ransac.py holds
        t, s, _, _ = planted(seed, n, 0.4, sigma=0.12)  # residuals on both sides of the bound: the refinement takes several rounds
        sets["noisy_%d" % n] = (t, s, 0.3, (100, 20000))
    for n in (517, 2840):
        t, s, _, _ = planted(3000 + n, n, 0.02)  # runs to max_iter_num
        sets["sparse_%d" % n] = (t, s, 0.5, (100, 20000))
    for n in (0, 1, 2):
        t, s, _, _ = planted(4000 + n, n, 1.0)
        sets["tiny_%d" % n] = (t, s, 0.5, (100,))
    sets["coincident_64"] = coincident(64) + (0.5, (100,))
    sets["collinear_200"] = collinear(7, 200) + (0.2, (100,))
    sets["unrelated_300"] = unrelated(8, 300) + (0.01, (100,))  # fewer than three inliers; refined: the fit selects nothing
    t, s, _, _ = planted(5000, 517, 0.5)
    sets["nan_src_517"] = with_nan(t, s, True) + (0.5, (100,))
    sets["nan_tgt_517"] = with_nan(t, s, False) + (0.5, (100,))
    if demo_npz is not None:
        kt, ks = xyzw_of(demo_npz["kpts_0"]), xyzw_of(demo_npz["kpts_15"])
        for name in DEMO_LISTS:
            pr = demo_npz[name + "_pairs"]
            sets["demo_" + name] = (kt[pr[:, 0]], ks[pr[:, 1]], 1.0, (100, 20000))  # 4 x keypoint_nms_radius (test/mulls_reg.cpp:107, :179)
    return sets


def case_name(set_name, max_iter, refine):
    return "%s_i%d_r%d" % (set_name, max_iter, refine)


def restate_set(tgt, src, bound, iters):
    """{(max_iter, refine): restate(...)} of one input set, its draws made once"""
    tri = draws(src, max(iters) + 1) if len(src) >= 3 else None
    return {(it, rf): restate(tgt, src, bound, 8, it, rf, tri=tri) for it in iters for rf in (0, 1)}
