"""mulls_scan_prepare and mulls_mapper_* on the device against tests/scanprep_restated.py (the cap of scanprep_restated.assert_close: counts, order and
untouched bytes identical, x / y / z / curvature within one float ulp on at most 1e-4 of the values), at the edges of MULLS_SCAN_CHUNK, and against each
other: one call against one call per frame against the public single calls, byte for byte."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import scanprep_restated as sr
from mulls_amd import abi, lib, synth
from test_scanprep import SIZES, hole_cloud, mapper_frames, oracle_compensate, sweep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = abi.SCAN_CHUNK


class DevBuf:
    """a device allocation of the caller's own, straight from the HIP runtime the library runs on"""

    def __init__(self, raw):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.n, self.p = len(raw), C.c_void_p()
        raw = np.ascontiguousarray(raw)
        assert self.hip.hipMalloc(C.byref(self.p), max(raw.nbytes, 64)) == 0
        if raw.nbytes:
            assert self.hip.hipMemcpy(self.p, C.c_void_p(raw.ctypes.data), raw.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def cloud(self):
        c = abi.Cloud()
        c.pts, c.n, c.stride = self.p.value, self.n, abi.POINT_BYTES
        return c

    def download(self, n=None):
        out = np.zeros((self.n if n is None else n, abi.POINT_BYTES), np.uint8)
        if out.nbytes:
            assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free(self):
        assert self.hip.hipFree(self.p) == 0


def check_prepare(ctx, scan, p):
    got, rep = ctx.scan_prepare(scan, p)
    want, info = sr.prepare(scan, p)
    assert (rep.n_in, rep.n_after_dist, rep.n_out) == (len(scan), info["n_after_dist"], info["n_out"])
    if p.timestamp_mode == 1 and len(scan):
        assert (rep.first_timestamp, rep.last_timestamp) == (info["first"], info["last"])
        assert rep.scan_duration_used == info["duration"] or (math.isinf(rep.scan_duration_used) and math.isinf(info["duration"]))
    sr.assert_close(got, want)
    return got


@pytest.mark.parametrize("label,p", sweep(), ids=[s[0] for s in sweep()])
def test_prepare_equals_restatement(ctx_auto, label, p):
    """n in {0, 1, 63, 64, 65, C-1, C, C+1, 3C+7}, points at 0.5 - 130 m so that both limits bite; and one 32-beam synthetic scan"""
    for k, n in enumerate(SIZES):
        check_prepare(ctx_auto, sr.make_case(1000 + k, n, p), p)
    scene = synth.Scene(5)
    scan = synth.raycast(scene, synth.se3(0, 0, scene.sensor_height), 32, 300, seed=5)
    pts = abi.records(abi.make_points(scan["xyz"], scan["nrm"], scan["intensity"], scan["t"] * 100.0))
    assert sr.margin_ok(pts, p) and len(pts) > 4 * CH
    check_prepare(ctx_auto, pts, p)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("ratio", [2, 5, 8])
def test_prepare_across_chunk_edges(ctx_auto, first, ratio):
    """a middle chunk without a survivor; survivors per chunk that are no multiples of the ratio: the rank's remainder carries across the chunk edges"""
    p = abi.scan_prep_params(calib_on=1, dist_filter_on=1, calib_first=first, downsample_ratio=ratio, timestamp_mode=1, vertical_ang_correction_deg=0.195, min_dist=2.0,
                             max_dist=80.0)
    scan = hole_cloud(7, p)
    got = check_prepare(ctx_auto, scan, p)
    assert len(got) == (2 * CH - 3 + ratio - 1) // ratio and (2 * CH - 3) % ratio and (CH - 3) % ratio


def test_prepare_time_stamp_edges(ctx_auto):
    p = abi.scan_prep_params(timestamp_mode=1)
    scan = sr.make_scan(11, 300)
    q = abi.points_of(scan)
    q["curvature"] = 42.0  # equal stamps: 0 / 0, and the NaN is stored
    got = check_prepare(ctx_auto, scan, p)
    assert np.isnan(abi.points_of(got)["curvature"]).all()
    for span, replaced in ((74.0, True), (76.0, False)):  # a duration under 75 ms is replaced, a longer one is not
        q["curvature"] = np.linspace(5.0, 5.0 + span, 300)
        check_prepare(ctx_auto, scan, p)
        rep = ctx_auto.scan_prepare(scan, p)[1]
        assert (rep.scan_duration_used == 100.0) != replaced
    q["curvature"][:] = 0.0
    q["curvature"][::2] = -0.0
    check_prepare(ctx_auto, scan, p)
    # a NaN stamp: MULLS_E_INVALID, the cloud untouched — on the host path and in place
    q["curvature"] = np.linspace(0.0, 99.0, 300)
    q["curvature"][17] = np.nan
    with pytest.raises(lib.MullsError) as e:
        ctx_auto.scan_prepare(scan, p)
    assert e.value.args[1] == abi.MULLS_E_INVALID
    for dev in (False, True):
        raw, n_out = scan.copy(), C.c_uint32(7)
        buf = DevBuf(raw) if dev else None
        rc = ctx_auto.lib.mulls_scan_prepare(ctx_auto.h, buf.p if dev else C.c_void_p(raw.ctypes.data), len(raw), abi.POINT_BYTES, C.byref(p), C.byref(n_out), None)
        assert rc == abi.MULLS_E_INVALID and n_out.value == 0
        assert np.array_equal(buf.download() if dev else raw, scan)
        if dev:
            buf.free()
    # a thinned-out NaN stamp is not seen: upstream's scan runs over the cloud as it stands then
    p2 = abi.scan_prep_params(timestamp_mode=1, downsample_ratio=2)
    check_prepare(ctx_auto, scan, p2)


def test_prepare_axes_origin_and_bad_parameters(ctx_auto):
    scan = sr.make_scan(12, 9)
    q = abi.points_of(scan)
    for k, (x, y) in enumerate([(5.0, 0.0), (5.0, -0.0), (-5.0, 0.0), (-5.0, -0.0), (0.0, 5.0), (-0.0, 5.0), (0.0, -5.0), (-0.0, -5.0), (0.0, 0.0)]):
        q["x"][k], q["y"][k] = x, y
    q["z"][8] = 0.0
    for begin in (180.0, 90.0):
        p = abi.scan_prep_params(calib_on=1, vertical_ang_correction_deg=0.195, timestamp_mode=2, scan_begin_ang_deg=begin)
        got = check_prepare(ctx_auto, scan, p)
        assert np.isnan(abi.points_of(got)["x"][8])
    for field in ("min_dist", "max_dist", "vertical_ang_correction_deg", "scan_begin_ang_deg"):
        for bad in (math.nan, math.inf):
            p = abi.scan_prep_params(dist_filter_on=1)
            setattr(p, field, bad)
            with pytest.raises(lib.MullsError) as e:
                ctx_auto.scan_prepare(scan, p)
            assert e.value.args[1] == abi.MULLS_E_INVALID
    n_out = C.c_uint32(0)
    p = abi.scan_prep_params()
    assert ctx_auto.lib.mulls_scan_prepare(ctx_auto.h, C.c_void_p(scan.ctypes.data), len(scan), 64, C.byref(p), C.byref(n_out), None) == abi.MULLS_E_INVALID
    assert ctx_auto.lib.mulls_scan_prepare(ctx_auto.h, None, 0, abi.POINT_BYTES, C.byref(p), C.byref(n_out), None) == abi.MULLS_OK and n_out.value == 0


# torch brings a HIP runtime of its own: a process takes one of the two, the one loaded first, so the tensor lives in a child that imports torch first
TORCH_CHILD = r"""
import ctypes as C, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
torch.cuda.init()
assert torch.zeros(4, device="cuda:0").sum().item() == 0
import scanprep_restated as sr
from mulls_amd import abi, lib
ctx = lib.Context(0)
C_ = abi.SCAN_CHUNK
for k, p in enumerate((abi.scan_prep_params(calib_on=1, dist_filter_on=1, calib_first=0, downsample_ratio=1, timestamp_mode=2, vertical_ang_correction_deg=0.195, min_dist=2.0, max_dist=80.0),
                       abi.scan_prep_params(calib_on=1, dist_filter_on=1, calib_first=1, downsample_ratio=5, timestamp_mode=1, vertical_ang_correction_deg=-0.3, min_dist=2.0, max_dist=80.0))):
    scan = sr.make_case(80 + k, 3 * C_ + 7, p)
    want, rep = ctx.scan_prepare(scan, p)
    dev = torch.from_numpy(scan.copy()).to("cuda:0")
    torch.cuda.synchronize()
    n_out = C.c_uint32(0)
    rc = ctx.lib.mulls_scan_prepare(ctx.h, C.c_void_p(dev.data_ptr()), len(scan), abi.POINT_BYTES, C.byref(p), C.byref(n_out), None)
    assert rc == 0 and n_out.value == len(want) and 0 < len(want) < len(scan), (rc, n_out.value)
    back = dev.cpu().numpy()
    assert np.array_equal(back[: len(want)], want)  # packed at the front, the bytes of the host path
    assert np.array_equal(back[len(want):], scan[len(want):])  # behind them: what was there
ctx.close()
print("torch buffer ok")
"""


def test_host_path_and_callers_device_buffer_give_the_same_bytes():
    p = subprocess.run([sys.executable, "-c", TORCH_CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "torch buffer ok" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


# ---- the merged map ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mapped(ctx_auto):
    """frames of [0, 1, C, C+1, 2500, 4000 all outside the limits, 7000] points, mixed compensate, mixed host and device scans, distinct poses, ratio 5,
    mode 1: added in one call; the restatement's map, computed once"""
    frames, p = mapper_frames()
    bufs = {k: DevBuf(frames[k][0]) for k in (2, 4, 5)}
    mixed = [(bufs[k].cloud() if k in bufs else s, pose, adj) for k, (s, pose, adj) in enumerate(frames)]
    want, counts = sr.merged_map(frames, p, oracle_compensate)
    m = ctx_auto.mapper(len(want) + 100)
    got_counts, rep = m.add(mixed, p)
    out = dict(frames=frames, mixed=mixed, p=p, want=want, counts=counts, got_counts=got_counts, rep=rep, got=m.download(), mapper=m)
    yield out
    m.close()
    for b in bufs.values():
        b.free()


def test_mapper_one_call_equals_restatement(mapped):
    assert mapped["got_counts"] == mapped["counts"] and mapped["counts"][5] == 0 and min(mapped["counts"][k] for k in (1, 2, 3, 4, 6)) > 0
    rep = mapped["rep"]
    assert (rep.frames_added, rep.n_before, rep.n_after, rep.n_needed) == (7, 0, len(mapped["want"]), len(mapped["want"]))
    sr.assert_close(mapped["got"], mapped["want"])


def test_mapper_one_call_equals_one_call_per_frame_and_the_single_calls(ctx_auto, mapped):
    m = ctx_auto.mapper(len(mapped["want"]))
    offsets = []
    for fr in mapped["mixed"]:
        offsets.append(m.cloud().n)
        m.add([fr], mapped["p"])
    assert offsets == list(np.cumsum([0] + mapped["counts"][:-1]))
    assert np.array_equal(m.download(), mapped["got"])
    for k in (1, 4, 6):  # mulls_mapper_download from a frame's offset
        assert np.array_equal(m.download(offsets[k])[: mapped["counts"][k]], mapped["got"][offsets[k]: offsets[k] + mapped["counts"][k]])
    m.close()
    # mulls_scan_prepare -> mulls_motion_compensate -> the restated pose transform
    q = abi.ScanPrepParams.from_buffer_copy(mapped["p"])
    q.calib_first = 1
    parts = []
    for scan, pose, adj in mapped["frames"]:
        raw = ctx_auto.scan_prepare(scan, q)[0]
        if adj is not None and len(raw):
            raw = abi.records(ctx_auto.motion_compensate(raw, adj, 0.0))
        parts.append(sr.pose_transform(raw, pose))
    assert np.array_equal(np.concatenate(parts), mapped["got"])


def test_mapper_is_deterministic(ctx_auto, mapped):
    m = ctx_auto.mapper(len(mapped["want"]) + 100)
    m.add(mapped["mixed"], mapped["p"])
    assert np.array_equal(m.download(), mapped["got"])
    m.close()


def test_mapper_capacity(ctx_auto, mapped):
    frames, p, counts, total = mapped["mixed"], mapped["p"], mapped["counts"], len(mapped["want"])
    m = ctx_auto.mapper(total)  # an exact fit
    m.add(frames, p)
    assert np.array_equal(m.download(), mapped["got"])
    m.close()
    m = ctx_auto.mapper(total - 1)  # one point short: the last frame stays out, the earlier ones are intact
    with pytest.raises(lib.MullsError) as e:
        m.add(frames, p)
    assert e.value.args[1] == abi.MULLS_E_UNSUPPORTED
    rep = m.last_report
    assert (rep.frames_added, rep.n_before, rep.n_after, rep.n_needed) == (6, 0, total - counts[6], total) and m.last_counts == counts
    assert np.array_equal(m.download(), mapped["got"][: total - counts[6]])
    m.clear()  # clear, then reuse
    assert m.cloud().n == 0
    m.add(frames[:5], p)
    assert np.array_equal(m.download(), mapped["got"][: sum(counts[:5])])
    have = sum(counts[:5])
    with pytest.raises(lib.MullsError) as e:  # on top of what is there: the first frame that does not fit ends the appending, whatever would fit behind it
        m.add([frames[6], frames[1]], p)
    rep = m.last_report
    assert e.value.args[1] == abi.MULLS_E_UNSUPPORTED and (rep.frames_added, rep.n_before, rep.n_after, rep.n_needed) == (0, have, have, have + counts[6] + counts[1])
    m.add([frames[1], frames[3]], p)  # ... and the map goes on taking what fits
    assert np.array_equal(m.download(have), np.concatenate([mapped["got"][0:1], mapped["got"][sum(counts[:3]): sum(counts[:4])]]))
    other = lib.Context(0)  # a mapper of another context is refused
    rc = other.lib.mulls_mapper_add(other.h, m.h, None, 0, C.byref(p), None, None)
    c = abi.Cloud()
    assert rc == abi.MULLS_E_INVALID and other.lib.mulls_mapper_cloud(other.h, m.h, C.byref(c)) == abi.MULLS_E_INVALID
    other.close()
    m.close()
    bad = abi.scan_prep_params(timestamp_mode=1)  # a refusal of the preparation, in any frame: nothing is appended
    scan = sr.make_scan(31, 100)
    abi.points_of(scan)["curvature"][50] = np.nan
    m = ctx_auto.mapper(1000)
    with pytest.raises(lib.MullsError) as e:
        m.add([(sr.make_scan(30, 100), np.eye(4)), (scan, np.eye(4))], bad)
    assert e.value.args[1] == abi.MULLS_E_INVALID and m.cloud().n == 0
    m.close()


def test_mapper_cloud_feeds_sor(ctx_auto, mapped):
    """mulls_mapper_cloud -> mulls_sor_filter returns the bytes mulls_sor_filter returns on the downloaded host copy.  (Frames 4 and 6: the one-point frame's
    equal stamps give a NaN ratio and, compensated, NaN coordinates, which the filter refuses.)"""
    m = ctx_auto.mapper(2000)
    m.add([mapped["mixed"][4], mapped["mixed"][6]], mapped["p"])
    cloud, host = m.cloud(), m.download()
    assert cloud.n == len(host) == mapped["counts"][4] + mapped["counts"][6] > 21
    kept_d, idx_d, rep_d = ctx_auto.sor_filter(cloud)
    kept_h, idx_h, rep_h = ctx_auto.sor_filter(host)
    assert np.array_equal(kept_d, kept_h) and np.array_equal(idx_d, idx_h) and 0 < rep_d.n_kept == rep_h.n_kept < cloud.n
    m.close()


def test_mapper_real_demo_scans(ctx_auto):
    """the two real demo scans, the fixture's transform as the second pose; 0.195 degrees, limits 2 - 80 m, ratio 8, the ratio from the azimuth (KITTI has no stamps)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "demo_pair.npz"))
    T = z["pair_0_15_result"][:16].reshape(4, 4).T
    scans = [abi.records(abi.make_points(z[k][:, :3], None, z[k][:, 3])) for k in ("scan_0", "scan_15")]
    p = abi.scan_prep_params(calib_on=1, dist_filter_on=1, calib_first=1, downsample_ratio=8, timestamp_mode=2, vertical_ang_correction_deg=0.195, min_dist=2.0, max_dist=80.0)
    frames = [(scans[0], np.eye(4), None), (scans[1], T, np.linalg.inv(T) @ np.eye(4))]
    want, counts = sr.merged_map(frames, p, oracle_compensate)
    m = ctx_auto.mapper(len(want))
    got_counts, rep = m.add(frames, p)
    assert got_counts == counts and min(counts) > 5000
    sr.assert_close(m.download(), want)
    m.close()
