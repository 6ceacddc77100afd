"""The raw-scan steps of CFilter and the merged-map export, restated (include/mulls_hip.h, "scan preparation" and "the merged map"):
vertical_intrinsic_calibration (cfilter.hpp:250-291), dist_filter (:806-831), random_downsample (:730-747), get_pts_timestamp_ratio_in_frame (:412-467), and per frame
of test/mulls_slam.cpp:963-990 apply_motion_compensation and pcl::transformPointCloud behind them.

Float expressions are numpy float32 operations (one rounding each, no contraction); the transcendental functions are Python's math functions per element, i.e. the
C library upstream calls — never numpy's vector arcsin / arctan2, which may be SIMD implementations with a looser bound.  The device evaluates the same
functions correctly rounded (detmath.h); the C library is within one ulp of that, and a last-bit difference of a double moves a float result with probability
~1e-9 per value: comparisons against this restatement allow one float ulp on at most 1e-4 of the points (tests/test_motion_comp.py::ulp_close's cap and reasoning)
and demand everything else identical.
"""
import math

import numpy as np

from mulls_amd import abi

DBL_MAX = 1.7976931348623157e308


class Refused(ValueError):
    """what the library answers with MULLS_E_INVALID"""


def _m(fn, *a):
    """a math function with the C library's answer where Python raises"""
    try:
        return fn(*a)
    except (ValueError, ZeroDivisionError):
        return math.nan


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def check_params(p):
    for v in (p.min_dist, p.max_dist, p.vertical_ang_correction_deg, p.scan_begin_ang_deg, p.scan_duration_ms):
        if not math.isfinite(v):
            raise Refused("a parameter is not finite")
    if not 0 <= p.timestamp_mode <= 2:
        raise Refused("timestamp_mode")


def calibrate(pts, angle_deg):
    """in place"""
    if angle_deg == 0:
        return
    if angle_deg >= 180.0:
        pts["z"] = -pts["z"]
        return
    ang = angle_deg / 180.0 * math.pi
    x, y, z = pts["x"].copy(), pts["y"].copy(), pts["z"].copy()
    with np.errstate(all="ignore"):
        dist = np.sqrt((x * x + y * y) + z * z)  # float32 throughout
    ox, oy, oz = [], [], []
    for xi, yi, zi, d in zip(x.tolist(), y.tolist(), z.tolist(), dist.tolist()):
        v = _m(math.asin, _div(zi, d) if d == 0 or d != d else zi / d)
        vc = v + ang
        cv = _m(math.cos, v)
        hs = _m(math.cos, vc) / cv if cv != 0 and cv == cv else _div(_m(math.cos, vc), cv)
        ox.append(xi * hs)
        oy.append(yi * hs)
        oz.append(d * _m(math.sin, vc))
    with np.errstate(all="ignore"):
        pts["x"], pts["y"], pts["z"] = np.array(ox, np.float64).astype(np.float32), np.array(oy, np.float64).astype(np.float32), np.array(oz, np.float64).astype(np.float32)


def dist_d2(pts):
    with np.errstate(all="ignore"):
        return (pts["x"] * pts["x"] + pts["y"] * pts["y"]).astype(np.float64)


def dist_mask(pts, min_dist, max_dist):
    d2 = dist_d2(pts)
    return (d2 < max_dist * max_dist) & (d2 > min_dist * min_dist)


def stamp_range(curv):
    """the max_ / min_ folds of utility.hpp:31-32 in the cloud's order"""
    last, first = -DBL_MAX, DBL_MAX
    for v in curv.astype(np.float64).tolist():
        last = last if last > v else v
        first = first if first < v else v
    return first, last


def time_ratio(pts, mode, duration_ms, begin_deg, info):
    if mode == 1:
        c = pts["curvature"].astype(np.float64)
        if np.isnan(c).any():
            raise Refused("a time stamp is NaN")
        first, last = stamp_range(pts["curvature"])
        dur = np.float32(duration_ms)
        with np.errstate(all="ignore"):
            actual = last - first
            if actual < float(dur) * 0.75:
                dur = np.float32(actual)
            s = (last - c) / np.float64(dur)
            m = np.where(0.0 > s, 0.0, s)
            pts["curvature"] = np.where(1.0 < m, 1.0, m).astype(np.float32)
        info.update(first=first, last=last, duration=float(dur))
    elif mode == 2:
        begin = begin_deg / 180.0 * math.pi
        two_pi = 2 * math.pi
        out = np.empty(len(pts), np.float32)
        for i in range(len(pts)):
            ang = math.atan2(float(pts["y"][i]), float(pts["x"][i]))
            if ang < 0:
                ang += two_pi
            ang += begin
            if ang >= two_pi:
                ang -= two_pi
            out[i] = np.float32((two_pi - ang) / two_pi)
        pts["curvature"] = out


def prepare(pts, p):
    """mulls_scan_prepare on a copy of a cloud (POINT_DTYPE or raw records): (kept raw (n_out, 48) records, info)"""
    check_params(p)
    raw = abi.records(pts).copy()
    info = dict(n_in=len(raw), first=DBL_MAX, last=-DBL_MAX, duration=float(np.float32(p.scan_duration_ms)))
    angle = p.vertical_ang_correction_deg if p.calib_on else 0.0

    def dist(raw):
        return raw[dist_mask(abi.points_of(raw), p.min_dist, p.max_dist)] if p.dist_filter_on else raw

    if p.calib_first:
        calibrate(abi.points_of(raw), angle)
        raw = dist(raw)
    else:
        raw = dist(raw).copy()
        calibrate(abi.points_of(raw), angle)
    info["n_after_dist"] = len(raw)
    if p.downsample_ratio > 1:
        raw = raw[:: p.downsample_ratio]
    raw = np.ascontiguousarray(raw)
    time_ratio(abi.points_of(raw), p.timestamp_mode, p.scan_duration_ms, p.scan_begin_ang_deg, info)
    info["n_out"] = len(raw)
    return raw, info


def pose_transform(raw, pose):
    """pcl::transformPointCloud: positions in double, stored as float, every other field copied"""
    raw = raw.copy()
    q = abi.points_of(raw)
    T = np.asarray(pose, np.float64)
    x, y, z = (q[f].astype(np.float64) for f in ("x", "y", "z"))
    with np.errstate(all="ignore"):
        for r, f in enumerate(("x", "y", "z")):
            q[f] = (T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3]).astype(np.float32)
    return raw


def mapper_frame(scan, pose, adjacent_tran, p, motion_compensate):
    """one frame of test/mulls_slam.cpp:963-990; motion_compensate(raw records, Tran) -> raw records is apply_motion_compensation with threshold 0 (the
    oracle's restatement, or the library's public single call for the composition check)"""
    q = abi.ScanPrepParams.from_buffer_copy(p)
    q.calib_first = 1
    raw, info = prepare(scan, q)
    if adjacent_tran is not None and len(raw):
        raw = abi.records(motion_compensate(raw, adjacent_tran))
    return pose_transform(raw, pose), info


def merged_map(frames, p, motion_compensate):
    parts = [mapper_frame(s, pose, adj, p, motion_compensate)[0] for s, pose, adj in frames]
    return (np.concatenate(parts) if parts else np.zeros((0, abi.POINT_BYTES), np.uint8)), [len(a) for a in parts]


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------
def make_scan(seed, n, r_lo=0.5, r_hi=130.0):
    """n seeded points at r_lo .. r_hi m, elevation -25 .. +3 degrees, time stamps 0 .. 100 ms in curvature in sweep order; every byte of the records set
    (the bytes between the fields too: they are to come back as they went in)"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (n, abi.POINT_BYTES), dtype=np.uint8)
    q = abi.points_of(raw)
    r, az, el = rng.uniform(r_lo, r_hi, n), np.sort(rng.uniform(-np.pi, np.pi, n)), np.deg2rad(rng.uniform(-25.0, 3.0, n))
    q["x"], q["y"], q["z"] = r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)
    for f in ("nx", "ny", "nz"):
        q[f] = rng.normal(0, 1, n)
    q["intensity"] = rng.uniform(0, 255, n)
    q["curvature"] = (az + np.pi) / (2 * np.pi) * 100.0 + rng.uniform(0, 0.01, n)
    return raw


def margin_ok(raw, p, ulps=4):
    """no point within `ulps` float ulps of a dist limit, before or after the calibration: counts must not hinge on a last bit"""
    if not p.dist_filter_on:
        return True
    clouds = [abi.points_of(raw.copy())]
    if p.calib_on:
        c = abi.points_of(raw.copy())
        calibrate(c, p.vertical_ang_correction_deg)
        clouds.append(c)
    for c in clouds:
        with np.errstate(all="ignore"):
            d2 = c["x"] * c["x"] + c["y"] * c["y"]
        d2 = d2[np.isfinite(d2)]
        for lim in (p.min_dist * p.min_dist, p.max_dist * p.max_dist):
            if (np.abs(d2.astype(np.float64) - lim) <= ulps * np.spacing(np.maximum(d2, np.float32(lim))).astype(np.float64)).any():
                return False
    return True


def make_case(seed, n, p, **kw):
    raw = make_scan(seed, n, **kw)
    if not margin_ok(raw, p):
        raise ValueError("seed %d: a point lies within 4 float ulps of a dist limit" % seed)
    return raw


# ---- comparison ------------------------------------------------------------------------------------------------------------------------------------
def assert_close(got, want, frac=1e-4):
    """record counts, order and untouched bytes identical; x, y, z, curvature equal up to one float ulp on at most `frac` of the points (NaN where NaN)"""
    got, want = abi.records(got), abi.records(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(len(got), 12), want.view(np.uint32).reshape(len(want), 12)
    moving = [0, 1, 2, 9]  # x, y, z, curvature as 4-byte words
    still = [k for k in range(12) if k not in moving]
    assert np.array_equal(g[:, still], w[:, still])
    gf, wf = g[:, moving].view(np.float32), w[:, moving].view(np.float32)
    nan = np.isnan(wf)
    assert np.array_equal(np.isnan(gf), nan)
    d = np.abs(g[:, moving].view(np.int32).astype(np.int64) - w[:, moving].view(np.int32).astype(np.int64))
    d[nan] = 0
    assert d.max(initial=0) <= 1, int(d.max())
    bad = int((d != 0).sum())  # (+0 against -0 is 2^31 apart in this measure: a different answer)
    assert bad <= max(1, int(frac * len(got))), bad
    return bad
