"""numpy restatement of mulls_fpfh and mulls_coarse_reg_fpfhsac as include/mulls_hip.h defines them, written from that text: every operation in the
order and precision the definition says, atan2 correctly rounded through mpmath (memoised, tests/gicp_restated.py's; the IEEE special cases through
math.atan2, whose results there are exact constants), brute-force neighbours and brute-force nearest descriptors.  Nothing here was compared with PCL,
FLANN or Eigen themselves: none is a dependency of this repository.  This module is the yardstick of tests/test_fpfh.py and of the fixture
tests/golden/fpfh_cases.npz (tests/golden/make_fpfh_golden.py), which tests/test_gpu_fpfh.py compares the device with."""
import math

import numpy as np

import gicp_restated as gr
import ransac_restated as rr
from ndt_restated import tree_sum

F32 = np.float32
MARGIN = 1.0 + 2.0 ** -20
PI = float.fromhex("0x1.921fb54442d18p+1")
INV_2PI = 1.0 / (2.0 * PI)
BINS, DIMS = 11, 33
TRUNCATED, HUBER = 0, 1
MAX_POINTS = 1 << 24
MAX_CELL_POINTS = 16384  # MULLS_FPFH_MAX_CELL_POINTS


def fpfh_default_params(**kw):
    p = dict(search_radius=1.0)
    p.update(kw)
    return p


def fpfhsac_default_params(**kw):
    p = dict(search_radius=1.0, nr_samples=3, k_correspondences=15, max_iterations=10, min_sample_distance=0.0, max_correspondence_distance=float("inf"),
             error_function=TRUNCATED, seed=0)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def atan2_cr(y, x):
    if y == 0.0 or x == 0.0 or y != y or x != x or math.isinf(y) or math.isinf(x):
        return math.atan2(y, x)
    return gr.atan2_cr(y, x)


def dist2(a, b):
    """float32 (.., 3) -> float32: ((dx dx + dy dy) + dz dz)"""
    with np.errstate(all="ignore"):
        d = a.astype(F32) - b.astype(F32)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dot3(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross3(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2], u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def radius_of(search_radius):
    return float(F32(2.0) * F32(search_radius))


def cells_of(pts, r):
    """-> the (n, 3) float64 cell coordinates, and whether every one fits [-2^20, 2^20)"""
    inv_edge = 1.0 / (r * MARGIN)
    with np.errstate(all="ignore"):
        q = np.floor(pts.astype(np.float64) * inv_edge)
    return q, bool(((q >= -1048576.0) & (q < 1048576.0)).all())


def neighbourhood(pts, i, r):
    """the indices of the points within the radius of point i, itself included, ascending; their float32 d2"""
    d = dist2(pts, pts[i][None, :])
    idx = np.flatnonzero(d.astype(np.float64) <= r * r)
    return idx, d[idx]


def pair_features(p, n_p, Q, NQ):
    """the features of p against the rows of Q (normals NQ), in double: f (m, 3) = f1 f2 f3, ok (m,) whether the pair adds anything"""
    with np.errstate(all="ignore"):
        p, n_p, Q, NQ = (np.asarray(a, F32).astype(np.float64) for a in (p, n_p, Q, NQ))
        m = len(Q)
        dp = Q - p[None, :]
        f4 = np.sqrt(dot3(dp, dp))
        ok = f4 != 0.0
        a = np.broadcast_to(n_p, (m, 3))
        a1, a2 = dot3(a, dp) / f4, dot3(NQ, dp) / f4
        swap = np.abs(a1) < np.abs(a2)
        n1, n2 = np.where(swap[:, None], NQ, a), np.where(swap[:, None], a, NQ)
        dp = np.where(swap[:, None], -dp, dp)
        f3 = np.where(swap, -a2, a1)
        v = cross3(dp, n1)
        nv = np.sqrt(dot3(v, v))
        ok = ok & (nv != 0.0)
        v = v / nv[:, None]
        w = cross3(n1, v)
        f2 = dot3(v, n2)
        y, x = dot3(w, n2), dot3(n1, n2)
        f1 = np.array([atan2_cr(float(y[k]), float(x[k])) if ok[k] else 0.0 for k in range(m)], np.float64).reshape(m)
    return np.stack([f1, f2, f3], axis=1), ok


def bins_of(f):
    """(m, 3) features -> (m, 3) bins 0 .. 10, and which rows are free of NaN"""
    with np.errstate(all="ignore"):
        good = ~np.isnan(f).any(axis=1)
        g = np.where(good[:, None], f, 0.0)
        b = np.stack([np.floor(11.0 * ((g[:, 0] + PI) * INV_2PI)), np.floor(11.0 * ((g[:, 1] + 1.0) * 0.5)), np.floor(11.0 * ((g[:, 2] + 1.0) * 0.5))], axis=1)
    return np.clip(b, 0, BINS - 1).astype(np.int64), good


def spfh_counts(pts, nrm, r):
    """-> counts (n, 33) int64, k (n,) int64, contributed (n,) int64: the pairs that added something"""
    n = len(pts)
    counts, ks, used = np.zeros((n, DIMS), np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        idx, _ = neighbourhood(pts, i, r)
        ks[i] = len(idx)
        idx = idx[idx != i]
        if not len(idx):
            continue
        f, ok = pair_features(pts[i], nrm[i], pts[idx], nrm[idx])
        b, good = bins_of(f)
        b = b[ok & good]
        used[i] = len(b)
        for s in range(3):
            counts[i, BINS * s:BINS * (s + 1)] = np.bincount(b[:, s], minlength=BINS)
    return counts, ks, used


def spfh_of_counts(counts, ks):
    with np.errstate(all="ignore"):
        out = ((counts.astype(np.float64) * 100.0) / (ks.astype(np.float64) - 1.0)[:, None]).astype(F32)
    out[ks <= 1] = 0.0
    return out


def normalise(acc):
    """(.., 33) double sums -> (.., 33) float32"""
    out = np.zeros(acc.shape, F32)
    with np.errstate(all="ignore"):
        for s in range(3):
            a = acc[..., BINS * s:BINS * (s + 1)]
            tot = a[..., 0].copy()
            for b in range(1, BINS):
                tot = tot + a[..., b]
            h = (a * (100.0 / tot)[..., None]).astype(F32)
            h = np.where((tot != 0.0)[..., None], h, F32(0.0))
            out[..., BINS * s:BINS * (s + 1)] = np.where(np.isfinite(h), h, F32(0.0))
    return out


def weighted_sums(pts, spfh, r):
    """-> (n, 33) double: over the neighbours with d2 != 0, in the order of the 27 cells (x fastest) and ascending index inside a cell"""
    n = len(pts)
    cells, _ = cells_of(pts, r)
    acc = np.zeros((n, DIMS), np.float64)
    for i in range(n):
        idx, d2 = neighbourhood(pts, i, r)
        keep = d2 != 0.0
        idx, d2 = idx[keep], d2[keep]
        if not len(idx):
            continue
        off = (cells[idx] - cells[i][None, :]).astype(np.int64)
        assert (np.abs(off) <= 1).all()  # the 27-cell walk is exact
        cell = 9 * (off[:, 2] + 1) + 3 * (off[:, 1] + 1) + (off[:, 0] + 1)
        order = np.lexsort((idx, cell))
        terms = spfh[idx[order]].astype(np.float64) * (1.0 / d2[order].astype(np.float64))[:, None]
        acc[i] = np.add.accumulate(terms, axis=0)[-1]  # one after the other, from the first term
    return acc


def fpfh(pts, nrm, search_radius, detail=None):
    """pts, nrm: (n, 3) float32 -> hist (n, 33) float32, k (n,) ; None when a coordinate is outside the cells' range or a cell is too full.  detail, a dict, receives the
    counts, the pairs that contributed, SPFH and the weighted sums"""
    pts, nrm = np.ascontiguousarray(pts, F32).reshape(-1, 3), np.ascontiguousarray(nrm, F32).reshape(-1, 3)
    assert np.isfinite(pts).all() and np.isfinite(nrm).all()
    r = radius_of(search_radius)
    cells, ok = cells_of(pts, r)
    if not ok or np.unique(cells, axis=0, return_counts=True)[1].max() > MAX_CELL_POINTS:
        return None
    counts, ks, used = spfh_counts(pts, nrm, r)
    spfh = spfh_of_counts(counts, ks)
    acc = weighted_sums(pts, spfh, r)
    if detail is not None:
        detail.update(counts=counts, used=used, spfh=spfh, acc=acc)
    return normalise(acc), ks.astype(np.uint32)


# ---- SAC-IA

def draw_all(src, k_eff, iterations, min_sample_distance, seed, nr_samples=3):
    """-> samples (iterations, 3), ranks (iterations, 3), min_sample_distance as the halving rule left it"""
    eng, n = rr.MT19937(seed), len(src)
    min_d = F32(min_sample_distance)
    samples, ranks = np.zeros((iterations, nr_samples), np.int64), np.zeros((iterations, nr_samples), np.int64)
    for it in range(iterations):
        chosen, rejected = [], 0
        while len(chosen) < nr_samples:
            i = eng() % n
            ok = True
            for j in chosen:
                with np.errstate(all="ignore"):
                    ok = i != j and not (np.sqrt(dist2(src[i], src[j])) < min_d)
                if not ok:
                    break
            if ok:
                chosen.append(i)
                rejected = 0
            else:
                rejected += 1
                if rejected >= 3 * n:
                    min_d = F32(0.5) * min_d
                    rejected = 0
        samples[it] = chosen
        ranks[it] = [eng() % k_eff for _ in range(nr_samples)]
    return samples, ranks, float(min_d)


def desc_dist2(a, B):
    """float32 (33,), (m, 33) -> (m,) float32: the differences squared and added in bin order"""
    with np.errstate(all="ignore"):
        d = B - a[None, :]
        s = np.zeros(len(B), F32)
        for k in range(DIMS):
            s = s + d[:, k] * d[:, k]
    return s


def similar(src_hist, tgt_hist, samples, ranks, k_eff):
    corr = np.zeros(samples.shape, np.int64)
    for it in range(samples.shape[0]):
        for s in range(samples.shape[1]):
            d = desc_dist2(src_hist[samples[it, s]], tgt_hist)
            order = np.lexsort((np.arange(len(d)), d))[:k_eff]
            corr[it, s] = order[ranks[it, s]]
    return corr


def error_terms(e, thr, error_function):
    """float32 squared distances, the float range -> the double terms"""
    E, T = e.astype(np.float64), float(F32(thr))
    with np.errstate(all="ignore"):
        if error_function == HUBER:
            return np.where(E <= T, (0.5 * E) * E, (0.5 * T) * (2.0 * np.abs(E) - T))
        return np.where(E <= T, E / T, 1.0)


def first_hypothesis(errs):
    """the lowest error, the first among equals; a NaN error comes after every number, NaNs among themselves by index"""
    errs = np.asarray(errs, np.float64)
    return min(range(len(errs)), key=lambda h: (bool(np.isnan(errs[h])), 0.0 if np.isnan(errs[h]) else errs[h], h))


def nearest_d2(xp, tgt):
    d2 = np.empty(len(xp), F32)
    for b in range(0, len(xp), 256):
        d2[b:b + 256] = dist2(xp[b:b + 256, None, :], tgt[None, :, :]).min(axis=1)
    return d2


def fpfhsac(tgt, tgt_nrm, src, src_nrm, prm=None, detail=None):
    """-> dict of mulls_fpfhsac_result's fields (T row-major (4, 4)); None when a coordinate is outside the cells' range"""
    prm = prm or fpfhsac_default_params()
    tgt, src = np.ascontiguousarray(tgt, F32).reshape(-1, 3), np.ascontiguousarray(src, F32).reshape(-1, 3)
    assert len(src) >= 3 and len(tgt) >= 1 and prm["nr_samples"] == 3 and 1 <= prm["k_correspondences"] <= 64 and 1 <= prm["max_iterations"] <= 65536
    fs, ft = fpfh(src, src_nrm, prm["search_radius"]), fpfh(tgt, tgt_nrm, prm["search_radius"])
    if fs is None or ft is None:
        return None
    hs, ht = fs[0], ft[0]
    iters, k_eff = prm["max_iterations"], min(prm["k_correspondences"], len(tgt))
    samples, ranks, min_d = draw_all(src, k_eff, iters, prm["min_sample_distance"], prm["seed"])
    corr = similar(hs, ht, samples, ranks, k_eff)
    M = rr.models(src[samples.reshape(-1)], tgt[corr.reshape(-1)], np.arange(3 * iters).reshape(-1, 3))  # (iters, 12) float32
    errs, e_all = np.zeros(iters), []
    for h in range(iters):
        m = M[h].astype(np.float64).reshape(3, 4)
        xp = gr.move(m[:, :3].reshape(-1), m[:, 3], src).astype(F32)
        e = nearest_d2(xp, tgt)
        e_all.append(e)
        errs[h] = float(tree_sum(error_terms(e, prm["max_correspondence_distance"], prm["error_function"])))
    best = first_hypothesis(errs)
    T = np.eye(4)
    T[:3, :] = M[best].astype(np.float64).reshape(3, 4)
    fitness = float(tree_sum(e_all[best].astype(np.float64))) / float(len(src))
    if detail is not None:
        detail.update(samples=samples, ranks=ranks, corr=corr, models=M, errors=errs, min_d=min_d, src_hist=hs, tgt_hist=ht, e=e_all)
    return dict(best_iteration=best, iterations=iters, n_src=len(src), n_tgt=len(tgt), best_error=float(errs[best]), fitness=fitness, T=T)
