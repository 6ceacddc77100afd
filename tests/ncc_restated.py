"""numpy restatement of CRegistration::find_feature_correspondence_ncc (include/common/cregistration.hpp:409-601) — a helper of the tests, not a test.

Checked bit for bit against the reference's own lines on the fixture tests/golden/ncc_demo.npz (tests/test_ncc.py).  The Nt x Ns table is formed in row
chunks, so that 16 k x 12 k key points fit in memory.  Equal distances of the fixed-number mode are ordered by ascending flat index i * Ns + j (a stable
sort): the definition include/mulls_hip.h gives where upstream's unstable std::sort leaves the order open."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
INT_MIN = -(2 ** 31)
CHUNK_ENTRIES = 1 << 22  # table entries formed at a time


def fields(raw):
    """data[3], normal[0], normal[1], normal[3], intensity of (n, 48) uint8 records"""
    f = np.ascontiguousarray(raw).view(np.float32).reshape(len(raw), 12)
    return dict(h=f[:, 3], n0=f[:, 4], n1=f[:, 5], n3=f[:, 7], inten=f[:, 8])


def make_records(h, n0, n1, n3, inten, rng=None):
    """(n, 48) uint8 key-point records with the five fields the descriptor reads; the bytes it does not read are random when rng is given"""
    n = len(h)
    f = np.zeros((n, 12), np.float32) if rng is None else rng.normal(0, 10, (n, 12)).astype(np.float32)
    f[:, 3], f[:, 4], f[:, 5], f[:, 7], f[:, 8] = h, n0, n1, n3, inten
    return f.view(np.uint8).reshape(n, 48)


def f2i(x):
    """(int)x as the reference's x86 build evaluates it: truncation, INT_MIN for NaN and for values outside the int range"""
    x = np.asarray(x, np.float32)
    ok = (x >= np.float32(-2147483648.0)) & (x < np.float32(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, x, 0)).astype(np.int64), INT_MIN)


def intensity_range(inten):
    """intensity_min / intensity_max as the loop of :433-442 leaves them (min_(a, b) = a < b ? a : b): the plain min(FLT_MAX, .) / max(0, .) without a
    NaN; a NaN replaces the running value and is replaced by the next one"""
    lo, hi = FLT_MAX, np.float32(0)
    nan = np.nonzero(np.isnan(inten))[0]
    if len(nan):
        rest = inten[nan[-1] + 1:]
        if len(rest) == 0:
            return np.float32(np.nan), np.float32(np.nan)
        return rest.min(), rest.max()
    return min(lo, inten.min()), max(hi, inten.max())


def descriptors(raw, imin, imax):
    d = fields(raw)
    out = np.zeros((len(raw), 11), np.float32)
    q = lambda a, b: np.trunc(a / b).astype(np.int64)  # C++ int division truncates toward zero (|a| < 2^31: exact in double) ...
    r = lambda a, b: a - q(a, b) * b  # ... and % takes the sign of the dividend
    for base, key in ((0, "n0"), (4, "n1")):
        c = f2i(d[key])
        out[:, base + 0] = q(c, 1000000)
        out[:, base + 1] = q(r(c, 1000000), 10000)
        out[:, base + 2] = q(r(c, 10000), 100)
        out[:, base + 3] = r(c, 100)
    with np.errstate(all="ignore"):
        t = (d["inten"] - np.float32(imin)) / (np.float32(imax) - np.float32(imin))  # float
        out[:, 8] = (t.astype(np.float64) * 255.0).astype(np.float32)  # * 255.0 in double, narrowed by the store
        out[:, 9] = d["n3"] * np.float32(100)
        out[:, 10] = d["h"] * np.float32(30)
    return out


def table(T, S):
    """d(i, j) of :504-505: a float accumulator from +0, the eleven terms in k order"""
    dt = np.zeros((len(T), len(S)), np.float32)
    with np.errstate(all="ignore"):
        for k in range(11):
            dt += np.abs(T[:, k][:, None] - S[:, k][None, :])
    return dt


def restate(traw, sraw, fixed_num_corr=False, corr_num=2000, reciprocal_on=True):
    """-> (ok, pairs): the reference's bool and the (n, 2) int64 index pairs (target, source) in its push_back order"""
    nt, ns = len(traw), len(sraw)
    none = np.zeros((0, 2), np.int64)
    if nt < 10 or ns < 10:
        return False, none
    imin, imax = intensity_range(fields(traw)["inten"])
    T, S = descriptors(traw, imin, imax), descriptors(sraw, imin, imax)
    step = max(1, CHUNK_ENTRIES // ns)
    if not fixed_num_corr:
        col, row, colmin = np.zeros(nt, np.int64), np.zeros(nt, np.float32), np.full(ns, FLT_MAX, np.float32)
        for a in range(0, nt, step):
            dt = table(T[a:a + step], S)
            dd = np.where(dt < FLT_MAX, dt, FLT_MAX)  # `dist < min_dist_row` from FLT_MAX: NaN, inf and FLT_MAX itself never win
            c = dd.argmin(1)  # the first of the smallest
            col[a:a + step], row[a:a + step] = c, dd[np.arange(len(dd)), c]
            colmin = np.minimum(colmin, dd.min(0))
        keep = ~(row > colmin[col]) if reciprocal_on else np.ones(nt, bool)
        i = np.nonzero(keep)[0]
        return True, np.stack([i, col[i]], 1)
    if nt * ns > 2 ** 31 - 1 or corr_num > 65536:
        raise ValueError("unsupported")
    k = min(corr_num, nt * ns)
    if k <= 0:
        return True, none
    best_d, best_i = np.zeros(0, np.float32), np.zeros(0, np.int64)
    for a in range(0, nt, step):
        d = table(T[a:a + step], S).reshape(-1)
        idx = np.arange(len(d), dtype=np.int64) + a * ns
        ok = ~np.isnan(d)  # NaN distances are never selected
        if len(best_d) == k:
            ok &= d <= best_d[-1]
        d, idx = d[ok], idx[ok]
        if len(d) > k:
            ok = d <= np.partition(d, k - 1)[k - 1]
            d, idx = d[ok], idx[ok]
        d, idx = np.concatenate([best_d, d]), np.concatenate([best_i, idx])
        order = np.lexsort((idx, d))[:k]  # by distance, equal distances by flat index
        best_d, best_i = d[order], idx[order]
    ct, cs, out = np.zeros(nt, np.int64), np.zeros(ns, np.int64), []
    for index in best_i:
        i, j = divmod(int(index), ns)
        if ct[i] > 6 or cs[j] > 6:  # :578 — a point takes part seven times
            continue
        ct[i] += 1
        cs[j] += 1
        out.append((i, j))
    return True, np.array(out, np.int64).reshape(-1, 2)


def demo_extract_params():
    """extract_semantic_pts' arguments for the reference's demo scans: the values of tests/golden/make_demo_pair_golden.extract_params()
    (test/mulls_reg.cpp:134-143 with script/run_mulls_reg.sh's flags), copied — importing that module loads the HIP library"""
    from mulls_amd import abi

    G = abi.ground_params(min_grid_pt_num=8, grid_resolution=2.0, max_height_difference=0.25, neighbor_height_diff=1.2, max_ground_height=3.0e38,
                          ground_random_down_rate=10, ground_random_down_down_rate=2, nonground_random_down_rate=3, reliable_neighbor_grid_num_thre=0,
                          estimate_ground_normal_method=3, normal_estimation_radius=2.0, distance_weight_downsampling_method=2, standard_distance=15.0,
                          fixed_num_downsampling=0, down_ground_fixed_num=500, intensity_thre=3.4028234663852886e38, apply_grid_wise_outlier_filter=0)
    K = abi.classify_params(neighbor_searching_radius=1.0, neighbor_k=50, edge_thre=0.65, planar_thre=0.65, edge_thre_down=0.75, planar_thre_down=0.75,
                            curvature_thre=0.10)
    return abi.extract_params(ground=G, classify=K)


def random_kpts(seed, n, family="plain"):
    """seeded key-point records.  plain: codes as encode_stable_points packs them, continuous intensity / curvature / height.  quantised: every descriptor entry
    from a small alphabet of exactly representable values, so that equal distances are the rule.  bigcodes: codes beyond 2^24, negative, and outside the int
    range ((int) and % of the reference's x86 build)."""
    rng = np.random.default_rng(seed)
    if family == "quantised":
        bit = lambda: rng.integers(0, 2, n)
        n0 = (bit() * 1000000 + bit() * 10000 + bit() * 100 + bit()).astype(np.float32)
        n1 = (10100 + bit()).astype(np.float32)
        inten = rng.choice(np.array([0, 256], np.float32), n)  # range 256: (I - 0) / 256 * 255 is exact
        inten[:2] = (0, 256)
        return make_records(bit().astype(np.float32), n0, n1, bit().astype(np.float32) * np.float32(0.25), inten, rng)
    digit = lambda hi: rng.integers(0, hi, n)
    code = lambda: (digit(30) * 1000000 + digit(40) * 10000 + digit(60) * 100 + digit(99)).astype(np.float32)
    n0, n1 = code(), code()
    if family == "bigcodes":
        n0 = rng.uniform(-2.2e9, 2.2e9, n).astype(np.float32)  # beyond 2^24 (not every integer is a float), negative, a few outside the int range
        n1 = np.where(rng.random(n) < 0.5, -n1, n1 + np.float32(3.0e7)).astype(np.float32)
        n0[:4] = (3.0e9, -3.0e9, 2147483648.0, -2147483648.0)
    return make_records(rng.uniform(-2, 12, n).astype(np.float32), n0, n1, rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 255, n).astype(np.float32), rng)
