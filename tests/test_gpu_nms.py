"""GPU tests of mulls_non_max_suppress (CFilter::non_max_suppress, include/common/cfilter.hpp:1183-1312) through mulls_amd/lib.py, against the CPU harness
(tests/nms_harness.cpp: upstream's std::sort of the records and its sequential walk) and the fixture tests/golden/nms_cases.npz that tests/test_nms.py keeps
equal to it.

Every comparison is equality: the bytes of `out`, n_out, kept_idx and order, on both paths.  Nothing is left to a tolerance: the visiting order is one
std::sort on the host, the radius test is three correctly rounded float operations in a fixed order without contraction, and the result of the walk does not
depend on how the device schedules its rounds.

PCL is not available where these tests run: nothing here was compared with PCL itself."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nms_restated as nr
from mulls_amd import abi, lib, synth
from test_nms import build_harness, demo_keypoints, fixture, tie_records

pytestmark = pytest.mark.gpu

LIMIT = abi.NMS_LDS_MAX_POINTS


def raw_call(ctx, recs, radius=0.25, path=0, stride=None, n=None, cap=None, idx_cap=None, out=True, idx=True, order=True, report=True, n_out=True):
    """the C entry point with guard slots behind every output"""
    if isinstance(recs, abi.Cloud):
        c, n = recs, recs.n
    else:
        recs = np.ascontiguousarray(recs)
        n = len(recs) if n is None else n
        c = abi.Cloud()
        c.pts, c.n, c.stride = (recs.ctypes.data if recs.size else None), n, recs.shape[1] if stride is None else stride
    cap = n if cap is None else cap
    idx_cap = n if idx_cap is None else idx_cap
    o = np.full((cap + 1, abi.POINT_BYTES), 0xA5, np.uint8)
    i = np.full(idx_cap + 1, -7, np.int32)
    perm = np.full(n + 1, -9, np.int32)
    rep, cnt, p = abi.NmsReport(), C.c_uint32(12345), abi.nms_params(radius, path)
    rc = ctx.lib.mulls_non_max_suppress(ctx.h, C.byref(c), C.byref(p), o.ctypes.data_as(C.c_void_p) if out else None, cap if out else 0,
                                        C.byref(cnt) if n_out else None, i.ctypes.data_as(C.c_void_p) if idx else None, idx_cap if idx else 0,
                                        perm.ctypes.data_as(C.c_void_p) if order else None, C.byref(rep) if report else None)
    assert (o[cap] == 0xA5).all() and i[idx_cap] == -7 and perm[n] == -9  # nothing written past the capacities
    return rc, cnt.value, o[:cap], i[:idx_cap], perm[:n], rep


def check(ctx, recs, radius, paths=(1, 2), want=None, what=None):
    """both paths on one cloud against the harness (or a fixture's order and indices): every output; returns the reports"""
    recs = np.ascontiguousarray(recs)
    if want is None:
        _, w_idx, w_order = build_harness().suppress(recs, radius)
    else:
        w_order, w_idx = want
    w_out = recs[w_idx][:, :48]
    reps = []
    for path in paths:
        rc, n_out, o, i, perm, rep = raw_call(ctx, recs, radius, path)
        assert rc == abi.MULLS_OK, (what, path, rc, ctx.lib.mulls_last_error(ctx.h))
        assert n_out == len(w_idx) == rep.n_kept and rep.n_in == len(recs) and rep.ran == 1, (what, path, n_out, len(w_idx))
        assert np.array_equal(perm, w_order), (what, path)
        assert np.array_equal(i[:n_out], w_idx), (what, path)
        assert o[:n_out].tobytes() == w_out.tobytes(), (what, path)
        assert rep.path == (path or 2) and 1 <= rep.rounds <= len(recs) and rep.ms_total > 0
        reps.append(rep)
    return reps


def random_cloud(n, seed=None, half=None, levels=0):
    """n uniform points at a density where about a third survives 0.25 m; distinct keys, or keys quantised to `levels` values"""
    rng = np.random.default_rng(n if seed is None else seed)
    half = 0.13 * n ** (1 / 3) if half is None else half
    keys = rng.permutation(n).astype(np.float32) if not levels else np.floor(rng.uniform(0, 1, n) * levels).astype(np.float32)
    return nr.make_records(rng.uniform(-half, half, (n, 3)), keys, n)


# ---------------------------------------------------------------------------------------------------------------- gate and sizes
def test_gate(ctx_auto):
    recs = random_cloud(9, half=0.1)
    for path in (0, 1, 2):
        rc, n_out, o, i, perm, rep = raw_call(ctx_auto, recs, 0.25, path)
        assert rc == 0 and n_out == 9 and o.tobytes() == recs.tobytes() and list(i) == list(perm) == list(range(9))
        assert (rep.ran, rep.path, rep.n_in, rep.n_kept, rep.rounds) == (0, 0, 9, 9, 0)
    assert build_harness().suppress(recs, 0.25) is None
    for n in (10, 11):
        check(ctx_auto, random_cloud(n, half=0.3), 0.25, what=n)


@pytest.mark.parametrize("n", [255, 256, 257, 513, 1023, 1024, 1025])
def test_block_boundaries(ctx_auto, n):
    """around the multi-launch path's 256-point tiles and the one workgroup's 1024 lanes; half of the clouds with heavily tied keys"""
    reps = check(ctx_auto, random_cloud(n), 0.25, what=n)
    assert 0.1 * n < reps[0].n_kept < 0.7 * n
    check(ctx_auto, random_cloud(n, seed=n + 1, levels=5), 0.25, what=(n, "ties"))


@pytest.mark.parametrize("n", [LIMIT - 1, LIMIT, LIMIT + 1])
def test_one_workgroup_limit(ctx_auto, n):
    recs = random_cloud(n, levels=50)
    if n <= LIMIT:
        reps = check(ctx_auto, recs, 0.25, paths=(0, 1, 2), what=n)
        assert [r.path for r in reps] == [2, 1, 2]  # the library's own choice is the multi-launch path: it measures faster (profiles/nms_kernel_stats.txt)
    else:
        reps = check(ctx_auto, recs, 0.25, paths=(0, 2), what=n)
        assert [r.path for r in reps] == [2, 2]  # path 0 beyond the limit: the multi-launch path
        assert raw_call(ctx_auto, recs, 0.25, 1)[0] == abi.MULLS_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- shapes of the dependency relation
def test_dependency_chain(ctx_auto):
    """300 points on a line, 0.9 r apart, keys descending along it: every point's only earlier neighbour is its predecessor, so exactly the even positions
    are kept, and position i cannot be decided before position i - 1 is.  A wavefront's lanes read the states before any of them writes, so a round
    advances the chain by one position within a wavefront and by at most one more across each wavefront boundary (64 positions): the rounds a path reports
    lie between 300 - 5 and 300."""
    r = 0.25
    xyz = np.zeros((300, 3), np.float32)
    xyz[:, 0] = (np.arange(300) * (0.9 * r)).astype(np.float32)
    recs = nr.make_records(xyz, -np.arange(300, dtype=np.float32), 3)
    recs = recs[np.random.default_rng(3).permutation(300)]  # the input order is not the visiting order
    for rep in check(ctx_auto, recs, r, what="chain"):
        assert rep.n_kept == 150
        assert 295 <= rep.rounds <= 300, (rep.path, rep.rounds)
    kept = raw_call(ctx_auto, recs, r)[2][:150]
    assert np.array_equal(np.sort(nr.xyz_of(kept)[:, 0]), xyz[::2, 0])


@pytest.mark.parametrize("m", [100, 600])
def test_cluster_inside_one_radius(ctx_auto, m):
    """m points within one radius of each other next to scattered ones: 100 is more than either path's fixed list holds (8 in LDS, 32 in the multi-launch
    path), 600 asks the multi-launch path's shared pool for more than it has and reaches its direct scan"""
    rng = np.random.default_rng(m)
    xyz = np.concatenate([rng.uniform(-0.07, 0.07, (m, 3)) + [5.0, 5.0, 0.0], rng.uniform(-1.0, 1.0, (300, 3))]).astype(np.float32)
    recs = nr.make_records(xyz, rng.permutation(len(xyz)).astype(np.float32), m)
    check(ctx_auto, recs, 0.25, what=m)
    _, n_out, _, idx, _, _ = raw_call(ctx_auto, recs, 0.25)
    assert (idx[:n_out] < m).sum() == 1  # the cluster's best key alone


def test_coincident_points(ctx_auto):
    rng = np.random.default_rng(8)
    sites = rng.uniform(-2, 2, (40, 3)).astype(np.float32)
    xyz = sites[rng.integers(0, 40, 700)]
    for levels in (0, 3):
        keys = rng.permutation(700).astype(np.float32) if not levels else rng.integers(0, levels, 700).astype(np.float32)
        reps = check(ctx_auto, nr.make_records(xyz, keys, 8), 0.25, what=("coincident", levels))
        assert reps[0].n_kept <= 40
    reps = check(ctx_auto, nr.make_records(np.tile(sites[:1], (500, 1)), np.zeros(500), 9), 0.25, what="one site, one key")
    assert reps[0].n_kept == 1


def test_threshold(ctx_auto):
    """d2 < r2 is strict: two points whose float d2 equals r2 exactly are both kept; one ulp inward and the later one goes.  A negative radius acts as its
    absolute value, radius 0 keeps everything in sorted order."""
    far = np.stack([np.arange(10) * 10.0 + 100.0, np.zeros(10), np.zeros(10)], 1)
    keys = np.arange(12, dtype=np.float32)[::-1].copy()

    def pair(b):
        return nr.make_records(np.concatenate([[[0.0, 1.0, 2.0], [b, 1.0, 2.0]], far]).astype(np.float32), keys, 12)

    assert nr.r2_of(0.5) == np.float32(0.25) and np.float32(0.5) * np.float32(0.5) == np.float32(0.25)
    for radius in (0.5, -0.5):
        for rep in check(ctx_auto, pair(0.5), radius, what=("on the threshold", radius)):
            assert rep.n_kept == 12
        inward = np.nextafter(np.float32(0.5), np.float32(0))
        for rep in check(ctx_auto, pair(inward), radius, what=("one ulp inward", radius)):
            assert rep.n_kept == 11
        assert 1 not in raw_call(ctx_auto, pair(inward), radius)[3]
    recs = random_cloud(700)
    for rep in check(ctx_auto, recs, 0.0, what="radius 0"):
        assert rep.n_kept == 700 and rep.rounds == 1
    a, b = raw_call(ctx_auto, recs, 0.3), raw_call(ctx_auto, recs, -0.3)
    assert a[1] == b[1] < 700 and np.array_equal(a[3], b[3]) and a[2].tobytes() == b[2].tobytes()
    check(ctx_auto, recs, -0.3, what="negative radius")


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", sorted(nr.TIE_CASES))
def test_tie_cases_equal_fixture(ctx_auto, name):
    Z = fixture()
    check(ctx_auto, tie_records(name), nr.TIE_CASES[name][4], want=(Z[name + "_order"], Z[name + "_kept"]), what=name)


@pytest.mark.parametrize("name", ["kpts_0", "kpts_15"])
def test_demo_keypoints_equal_fixture(ctx_auto, name):
    """the reference's demo key points at upstream's 0.25 m (and at 1.0 m): 915 of 2840 and 851 of 2767 are kept"""
    Z = fixture()
    recs = demo_keypoints()[name]
    reps = check(ctx_auto, recs, 0.25, paths=(0, 1, 2), want=(Z[name + "_order"], Z[name + "_r0.25_kept"]), what=name)
    assert reps[0].n_kept == {"kpts_0": 915, "kpts_15": 851}[name]
    check(ctx_auto, recs, 1.0, want=(Z[name + "_order"], Z[name + "_r1_kept"]), what=(name, 1.0))


# ---------------------------------------------------------------------------------------------------------------- input and output forms
def test_strides_truncation_and_null_outputs(ctx_auto):
    recs = random_cloud(1500, levels=40)
    _, w_idx, w_order = build_harness().suppress(recs, 0.25)
    nk = len(w_idx)
    assert 100 < nk < 1400
    for stride in (52, 64):
        wide = np.random.default_rng(stride).integers(0, 256, (len(recs), stride), dtype=np.uint8)
        wide[:, :48] = recs
        check(ctx_auto, wide, 0.25, want=(w_order, w_idx), what=stride)
    for path in (1, 2):
        # capacities below the kept count: truncated, the full count reported
        rc, n_out, o, i, perm, rep = raw_call(ctx_auto, recs, 0.25, path, cap=50, idx_cap=7)
        assert rc == 0 and n_out == nk == rep.n_kept and np.array_equal(i, w_idx[:7]) and o.tobytes() == recs[w_idx[:50]].tobytes() and np.array_equal(perm, w_order)
        # each output absent in turn
        for absent in ("out", "idx", "order", "report", "n_out"):
            rc, n_out, o, i, perm, rep = raw_call(ctx_auto, recs, 0.25, path, **{absent: False})
            assert rc == 0, absent
            if absent != "n_out":
                assert n_out == nk
            if absent != "out":
                assert o[:nk].tobytes() == recs[w_idx].tobytes()
            if absent != "idx":
                assert np.array_equal(i[:nk], w_idx)
            if absent != "order":
                assert np.array_equal(perm, w_order)
            if absent != "report":
                assert rep.n_kept == nk and rep.path == path


def test_refusals(ctx_auto):
    recs = random_cloud(400)
    rc, n_out, _, _, _, rep = raw_call(ctx_auto, recs[:0])
    assert rc == abi.MULLS_OK and n_out == 0 and rep.n_kept == 0 and rep.ran == 0
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            x = recs.copy()
            x[137, 4 * axis:4 * axis + 4] = np.frombuffer(np.float32(bad).tobytes(), np.uint8)
            assert raw_call(ctx_auto, x)[0] == abi.MULLS_E_INVALID
            assert raw_call(ctx_auto, x[130:139])[0] == abi.MULLS_E_INVALID  # under the gate too
        assert raw_call(ctx_auto, recs, radius=bad)[0] == abi.MULLS_E_INVALID
    x = recs.copy()
    x[29, 28:32] = np.frombuffer(np.float32(np.nan).tobytes(), np.uint8)
    assert raw_call(ctx_auto, x)[0] == abi.MULLS_E_INVALID  # a NaN key: upstream's sort is undefined
    x[29, 28:32] = np.frombuffer(np.float32(np.inf).tobytes(), np.uint8)
    assert raw_call(ctx_auto, x)[0] == abi.MULLS_OK  # an infinite key sorts
    assert raw_call(ctx_auto, recs, stride=44)[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, stride=50)[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, path=3)[0] == abi.MULLS_E_INVALID
    assert raw_call(ctx_auto, recs, path=-1)[0] == abi.MULLS_E_INVALID
    # more than 2^18 points: refused before anything is read (the records behind the first 400 do not exist)
    assert raw_call(ctx_auto, recs, n=abi.NMS_MAX_POINTS + 1, cap=0, idx_cap=0, order=False)[0] == abi.MULLS_E_UNSUPPORTED
    assert raw_call(ctx_auto, recs)[0] == abi.MULLS_OK  # the context still works


def test_device_resident_clouds(ctx_auto):
    """key points in a feature block and in a local map (mulls_block_cloud, mulls_map_cloud) give the result of the same cloud downloaded and passed from the host"""
    scene = synth.Scene(7)
    scan = synth.raycast(scene, synth.se3(0, 0, scene.sensor_height), 32, 900, seed=7)
    pts = abi.make_points(scan["xyz"], np.zeros_like(scan["xyz"]), scan["intensity"], scan["t"])
    X = abi.extract_params(ground=abi.ground_params(nonground_random_down_rate=1), classify=abi.classify_params(neighbor_k=20))
    b = ctx_auto.block().extract(pts, X)
    seen = 0
    for which in (abi.EX_VERTEX, abi.EX_PILLAR + 2, abi.EX_GROUND):  # the last one is beyond the one-workgroup limit
        host = b.download(which)
        if len(host) < 10:
            continue
        seen += 1
        _, w_idx, w_order = build_harness().suppress(host, 0.25)
        for path in (0, 2):
            rc, n_out, o, i, perm, rep = raw_call(ctx_auto, b.cloud(which), 0.25, path)
            assert rc == 0 and n_out == len(w_idx) and np.array_equal(i[:n_out], w_idx) and np.array_equal(perm, w_order), (which, path)
            assert o[:n_out].tobytes() == host[w_idx].tobytes() and 0 < n_out < len(host)
        assert b.download(which).tobytes() == host.tobytes()  # the input is never modified
    assert seen >= 2
    clouds = [abi.points_of(b.download(k)) for k in (abi.EX_GROUND, abi.EX_PILLAR, abi.EX_PILLAR + 2, abi.EX_PILLAR + 1, abi.EX_PILLAR + 3, abi.EX_VERTEX)]
    m = lib.LocalMap(ctx_auto, clouds, np.eye(4))
    for cls in (abi.VERTEX, abi.FACADE):
        host = abi.records(m.download(cls))
        assert len(host) >= 10
        _, w_idx, w_order = build_harness().suppress(host, 0.25)
        kept, idx, order, rep = ctx_auto.non_max_suppress(m.cloud(cls), 0.25)
        assert np.array_equal(idx, w_idx) and np.array_equal(order, w_order) and kept.tobytes() == host[w_idx].tobytes() and rep.ran == 1
    m.close()
    b.close()


TORCH_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
torch.cuda.init()
assert torch.zeros(4, device="cuda:0").sum().item() == 0
from mulls_amd import abi, lib
from test_nms import build_harness, demo_keypoints
from test_gpu_nms import raw_call
recs = demo_keypoints()["kpts_15"]
_, w_idx, w_order = build_harness().suppress(recs, 0.25)
ctx = lib.Context(0)
dev = torch.from_numpy(recs.copy()).to("cuda:0")
pin = torch.from_numpy(recs.copy()).pin_memory()
torch.cuda.synchronize()
for x in (dev, pin):
    for path in (1, 2):
        c = abi.Cloud()
        c.pts, c.n, c.stride = x.data_ptr(), len(recs), 48
        rc, n_out, o, i, perm, rep = raw_call(ctx, c, 0.25, path)
        assert rc == 0 and n_out == len(w_idx) and np.array_equal(i[:n_out], w_idx) and np.array_equal(perm, w_order)
        assert o[:n_out].tobytes() == recs[w_idx].tobytes() and rep.path == path
assert dev.cpu().numpy().tobytes() == recs.tobytes()
wide = torch.zeros((len(recs), 64), dtype=torch.uint8, device="cuda:0")
torch.cuda.synchronize()
c = abi.Cloud()
c.pts, c.n, c.stride = wide.data_ptr(), len(recs), 64
assert raw_call(ctx, c)[0] == abi.MULLS_E_INVALID  # a device cloud whose stride is not 48
ctx.close()
print("torch clouds ok")
"""


def test_torch_device_and_pinned_tensors():
    """a cloud in a torch device tensor and in a pinned host tensor, on both paths: the host cloud's result.  (A process of its own: torch's runtime and the
    library's share the device there and nowhere else in this suite.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", TORCH_CHILD % (root, os.path.join(root, "tests"))], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "torch clouds ok" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- reuse
def test_reuse(ctx_auto, pairs_small):
    """the same call twice: the same bytes; a registration on the same context before and after gives its result unchanged; a small cloud after a large one
    and one path after the other are still right"""
    P = abi.kitti_params(dis_thre_unit=2.4)
    pair = pairs_small[0][0]  # (pair, ground-truth transform)
    T0 = list(ctx_auto.icp(pair, P)[0].T[:])
    big = random_cloud(20000, levels=100)
    a = ctx_auto.non_max_suppress(big, 0.25)
    b = ctx_auto.non_max_suppress(big, 0.25)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3].path == 2
    assert list(ctx_auto.icp(pair, P)[0].T[:]) == T0
    check(ctx_auto, random_cloud(700), 0.25, paths=(2, 1, 2, 0), what="small after large")
    assert list(ctx_auto.icp(pair, P)[0].T[:]) == T0


# ---------------------------------------------------------------------------------------------------------------- the tool
def test_mulls_reg_tool_thins_the_key_points(tmp_path, capsys):
    """tools/mulls_reg.py on the reference's two demo scans: with --is_global_reg both key-point clouds are suppressed at 0.25 * pca_neighbor_radius before
    they are matched (test/mulls_reg.cpp:145-149), fewer are left than came in, and the run goes through"""
    import importlib.util
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mulls_reg_tool", os.path.join(root, "tools", "mulls_reg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    Z = np.load(os.path.join(root, "tests", "golden", "demo_pair.npz"))
    paths = []
    for k in (0, 15):
        s = Z["scan_%d" % k]
        path = str(tmp_path / ("scan%d.pcd" % k))
        lib.write_pcd(path, abi.make_points(s[:, :3], np.zeros_like(s[:, :3]), s[:, 3]))
        paths.append(path)
    res, source = tool.main(["--point_cloud_1_path", paths[0], "--point_cloud_2_path", paths[1]])
    out = capsys.readouterr().out
    counts = re.findall(r"non_max_suppress: (target|source) key points (\d+) -> (\d+)", out)
    assert [c[0] for c in counts] == ["target", "source"]
    for _, before, after in counts:
        assert 10 <= int(after) < int(before)
    pairs = int(re.search(r"global registration: (\d+) key-point pairs", out).group(1))
    assert pairs <= int(counts[0][2])
    assert isinstance(res.code, int) and res.iters >= 1 and source in (1, 2)
    res, _ = tool.main(["--point_cloud_1_path", paths[0], "--point_cloud_2_path", paths[1], "--is_global_reg=false"])
    assert "non_max_suppress" not in capsys.readouterr().out and res.iters >= 1
