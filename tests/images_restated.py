"""The pictures of a cloud, restated (include/mulls_hip.h, "the pictures of a cloud"): CloudUtility::get_cloud_cpt (utility.hpp:800-814), CFilter::generate_2d_map
(cfilter.hpp:2751-2790) and CFilter::pointcloud_to_rangeimage (:2714-2746).

Float expressions are numpy float32 operations (one rounding each, no contraction), double ones float64.  asin and atan2 are Python's math functions per
element, the way tests/scanprep_restated.py takes them: the C library's double functions, whose result is rounded to float at once.  The device evaluates them
correctly rounded (detmath.h); the two differ by a last bit of a double at most, which moves the float with a probability of ~1e-9 per value, so the images
are compared byte for byte.  Nothing here knows of chunks, workgroups or atomics: the range image is one loop in index order, so "the highest index wins" falls
out of it, and the counts are one increment per point."""
import math

import numpy as np

from mulls_amd import abi

TREE = 4096  # MULLS_NDT_TREE
MAX_POINTS = 1 << 24  # MULLS_SCAN_MAX_POINTS
MAX_PIXELS = 1 << 26  # MULLS_IMAGE_MAX_PIXELS
F32 = np.float32


class Refused(ValueError):
    """what the library answers with MULLS_E_INVALID"""


class Unsupported(ValueError):
    """... with MULLS_E_UNSUPPORTED"""


def _points(pts):
    raw = abi.records(pts)
    if len(raw) > MAX_POINTS:
        raise Unsupported("more than 2^24 points")
    return abi.points_of(raw)


# ---- centre point -----------------------------------------------------------------------------------------------------------------------------------
def strided_tree_sum(terms):
    """MULLS_NDT_TREE's rule over float64 terms: lane l adds the terms l, l + TREE, .. in order from 0, then partial[l] += partial[l + w] for w = TREE / 2 .. 1.
    (Lanes are padded with +0.0: a partial sum that starts at +0.0 is never -0.0, so adding +0.0 leaves every value as it is.)"""
    terms = np.asarray(terms, np.float64)
    rows = np.concatenate([terms, np.zeros((-len(terms)) % TREE)]).reshape(-1, TREE)
    acc = np.zeros(TREE)
    with np.errstate(all="ignore"):
        for row in rows:
            acc = acc + row
        w = TREE // 2
        while w >= 1:
            acc[:w] = acc[:w] + acc[w:2 * w]
            w //= 2
    return float(acc[0])


def centre(pts):
    """get_cloud_cpt: the term of point i is x_i / (float)n, a float division, widened to double and added"""
    q = _points(pts)
    n = len(q)
    if n == 0:
        return np.zeros(3)
    with np.errstate(all="ignore"):
        return np.array([strided_tree_sum((q[f] / F32(n)).astype(np.float64)) for f in ("x", "y", "z")])


# ---- 2-D map image ------------------------------------------------------------------------------------------------------------------------------------
def check_image2d(p):
    if p.max_points_in_pix == p.min_points_in_pix:
        raise Refused("max == min")
    if p.map_width < 1 or p.map_height < 1 or p.map_width * p.map_height > MAX_PIXELS:
        raise Refused("size")
    if math.isnan(p.m2pix) or math.isnan(p.min_height) or math.isnan(p.max_height):
        raise Refused("NaN")
    if not 0 <= p.count_form <= 2:
        raise Refused("count_form")


def map_pixels(q, p, c):
    """per point: (kind, x, y) with kind 0 counted, 1 skipped by the height, 2 skipped by the frame — element-wise over the whole cloud"""
    W, H = p.map_width, p.map_height
    sx, sy = (F32(c[0]), F32(c[1])) if p.shift else (F32(0), F32(0))
    with np.errstate(all="ignore"):
        z = q["z"].astype(np.float64)
        by_height = (z < p.min_height) | (z > p.max_height)  # a NaN z passes
        dx = (q["x"] - sx).astype(np.float64) * p.m2pix + float(W // 2)
        dy = (-(q["y"] - sy)).astype(np.float64) * p.m2pix + float(H // 2)
        tx, ty = np.trunc(dx), np.trunc(dy)  # toward zero: (-1, 0) -> column 0
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)  # false for NaN
    kind = np.where(by_height, 1, np.where(inside, 0, 2))
    px = np.where(kind == 0, tx, 0).astype(np.int64)
    py = np.where(kind == 0, ty, 0).astype(np.int64)
    return kind, px, py


def to_8_bits(counts, p):
    """map -= min; map.convertTo(CV_8UC1, -255.0 / (max - min), 255) as the header restates it"""
    a = F32(-255.0 / float(p.max_points_in_pix - p.min_points_in_pix))
    v = (counts.astype(np.int64) - p.min_points_in_pix).astype(np.float32) * a + F32(255.0)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)  # rint: half to even


def map_image(pts, p, vectorised=False):
    """mulls_map_image_2d: (image uint8 (H, W), counts int32 (H, W), info).  vectorised: the counts by np.bincount instead of one increment per point."""
    check_image2d(p)
    q = _points(pts)
    c = centre(pts)
    kind, px, py = map_pixels(q, p, c)
    W, H = p.map_width, p.map_height
    if vectorised:
        counts = np.bincount((py * W + px)[kind == 0], minlength=W * H).astype(np.int32).reshape(H, W)
    else:
        counts = np.zeros((H, W), np.int32)
        for k, x, y in zip(kind.tolist(), px.tolist(), py.tolist()):
            if k == 0:
                counts[y, x] += 1
    info = dict(centre=c, n_counted=int((kind == 0).sum()), n_skipped_height=int((kind == 1).sum()), n_skipped_frame=int((kind == 2).sum()))
    return to_8_bits(counts, p), counts, info


# ---- range image --------------------------------------------------------------------------------------------------------------------------------------
def check_range(p):
    if p.width < 1 or p.height < 1 or p.width * p.height > MAX_PIXELS:
        raise Refused("size")
    if not (math.isfinite(p.f_up_deg) and math.isfinite(p.f_down_deg) and math.isfinite(p.max_distance)):
        raise Refused("not finite")
    if not p.max_distance > 0:
        raise Refused("max_distance")


def _m(fn, *a):
    """a math function with the C library's answer where Python raises"""
    try:
        return fn(*a)
    except (ValueError, ZeroDivisionError):
        return math.nan


def _clamp_trunc(f, size):
    return int(min(max(math.trunc(float(f)), 0), size - 1))


def range_image(pts, p):
    """mulls_range_image: the (height, width) uint8 image; one loop in index order, a later point overwrites an earlier one"""
    check_range(p)
    q = _points(pts)
    W, H = p.width, p.height
    f_up, f_down, max_d = F32(p.f_up_deg), F32(p.f_down_deg), F32(p.max_distance)
    img = np.zeros((H, W), np.uint8)
    x, y, z = q["x"], q["y"], q["z"]
    with np.errstate(all="ignore"):
        d = np.sqrt((x * x + y * y) + z * z)  # float32 throughout
        zq = z / d
        for i in range(len(q)):
            hor = F32(math.atan2(float(y[i]), float(x[i])))
            a = F32(_m(math.asin, float(zq[i])))
            ver = F32((float(a) / math.pi) * 180.0)
            u = F32((0.5 * (1 - float(hor) / math.pi)) * W)
            v = (F32(1) - (f_up - ver) / (f_up + f_down)) * F32(H)  # entirely in float
            if not (math.isfinite(float(u)) and math.isfinite(float(v))):
                continue
            col, row = _clamp_trunc(u, W), _clamp_trunc(v, H)
            quot = float(d[i] / max_d)
            img[H - 1 - row, col] = int(255.0 * (1.0 if 1.0 < quot else quot))  # min_(1.0, quot), the conversion truncates
    return img


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------------
def cloud_of(xyz, seed=0):
    """raw records with the given coordinates and every other byte random"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    raw = np.random.default_rng(seed).integers(0, 256, (len(xyz), abi.POINT_BYTES), dtype=np.uint8)
    q = abi.points_of(raw)
    q["x"], q["y"], q["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return raw


def make_scan(seed, n, r_lo=0.5, r_hi=90.0, offset=(0.0, 0.0, 0.0)):
    """n seeded points in sweep order (neighbouring indices are neighbours in azimuth), r_lo .. r_hi m, elevation -27 .. +5 degrees: past both field-of-view
    limits and past max_distance"""
    rng = np.random.default_rng(seed)
    r, az, el = rng.uniform(r_lo, r_hi, n), np.sort(rng.uniform(-np.pi, np.pi, n)), np.deg2rad(rng.uniform(-27.0, 5.0, n))
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1) + np.asarray(offset)
    return cloud_of(xyz, seed + 1)


def edge_cloud():
    """every edge case of the contract in one cloud, for a 16 x 12 map with m2pix 1, no shift, heights [-1, 2] (half sizes 8 and 6), and for the range image"""
    inf, nan = np.inf, np.nan
    xyz = [(-8.5, 0.0, 0.0),  # dx = -0.5: column 0
           (8.0, 0.0, 0.0),  # dx = width: outside
           (-9.0, 0.0, 0.0),  # dx = -1.0: outside
           (-8.999, 0.0, 0.0),  # dx just above -1: column 0
           (7.999, 0.0, 0.0),  # last column
           (0.0, 6.5, 0.0),  # dy = -0.5: row 0
           (0.0, -6.0, 0.0),  # dy = height: outside
           (0.0, 7.0, 0.0),  # dy = -1.0: outside
           (0.0, 0.0, nan),  # a NaN z is counted
           (0.0, 0.0, -1.0), (0.0, 0.0, 2.0),  # z equal to a height limit: kept
           (0.0, 0.0, np.nextafter(F32(-1.0), F32(-2.0))), (0.0, 0.0, np.nextafter(F32(2.0), F32(3.0))),  # just beyond: skipped
           (inf, 0.0, 0.0), (-inf, 0.0, 0.0), (nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, nan, 0.0), (1e30, 1e30, 0.0), (0.0, 0.0, inf), (0.0, 0.0, -inf),
           (0.0, 0.0, 0.0),  # the scanner's origin: skipped by the range image
           (1.0, 0.0, 100.0), (1.0, 0.0, -100.0),  # v beyond the rows on either side
           (-5.0, 0.0, 0.0), (-5.0, -0.0, 0.0),  # azimuth +pi and -pi: u = 0 and u = width
           (3.0, 4.0, 0.5), (3.0, 4.0, 0.5), (3.0, 4.0, 0.5)]
    return cloud_of(xyz, 99)


EDGE_MAP = dict(m2pix=1.0, map_width=16, map_height=12, min_points_in_pix=0, max_points_in_pix=2, min_height=-1.0, max_height=2.0, shift=0)
