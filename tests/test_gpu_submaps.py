"""mulls_submaps_* on the device against tests/submaps_restated.py.  Every comparison is exact: counts and bytes identical, doubles equal as numbers.  Class
sizes are drawn from {0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1}, CHUNK = MULLS_SUBMAP_CHUNK, the records one bounds job covers."""
import ctypes as C
import math

import numpy as np
import pytest

import submaps_restated as R
from conftest import planes_scene, transformed_copy
from icp_compare import same_bits
from mulls_amd import abi, lib
from test_gpu_scanprep import DevBuf
from test_map import small_frames

pytestmark = pytest.mark.gpu
CH = abi.SUBMAP_CHUNK
SIZES = (0, 1, 63, 64, 65, CH - 1, CH, CH + 1)
DBL_MAX = R.DBL_MAX
EMPTY_BOX = [DBL_MAX] * 3 + [-DBL_MAX] * 3
INF, NAN = float("inf"), float("nan")


def rand_cloud(rng, n, scale=30.0, centre=(0.0, 0.0, 0.0)):
    """n raw records: every byte random, x / y / z finite"""
    raw = rng.randint(0, 256, (n, abi.POINT_BYTES)).astype(np.uint8)
    xyz = (rng.standard_normal((n, 3)) * scale + np.asarray(centre)).astype(np.float32)
    raw[:, :12] = xyz.view(np.uint8).reshape(n, 12)
    return raw


def rand_submap(rng, sizes, **kw):
    return [rand_cloud(rng, n, **kw) for n in sizes]


def rigid(yaw, t, pitch=0.0):
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    T[:3, 3] = t
    return T


def pose_of(info):
    return np.array(info.pose_lo[:]).reshape(4, 4).T.copy()


def check_views(store, sid, clouds):
    """per-class, merged and merged-without-ground views against the merge order"""
    merged = R.merge(clouds)
    for c in range(6):
        assert np.array_equal(store.download(sid, c), clouds[c]), (sid, c)
    assert np.array_equal(store.download(sid, abi.SUBMAP_MERGED), merged), sid
    assert np.array_equal(store.download(sid, abi.SUBMAP_MERGED_NO_GROUND), merged[len(clouds[0]):]), sid
    # the views are slices of one range: consecutive addresses in merge order
    base = store.cloud(sid, abi.SUBMAP_MERGED)
    assert (base.n, base.stride) == (len(merged), abi.POINT_BYTES)
    addr = base.pts or 0
    for c in R.MERGE_ORDER:
        v = store.cloud(sid, c)
        assert v.n == len(clouds[c]) and (v.pts or 0) == addr, (sid, c)
        addr += 48 * len(clouds[c])
    ng = store.cloud(sid, abi.SUBMAP_MERGED_NO_GROUND)
    assert (ng.pts or 0) == (base.pts or 0) + 48 * len(clouds[0]) and ng.n == len(merged) - len(clouds[0])


def check_info(info, clouds, pose, id_in_strip, offset):
    assert list(info.n) == [len(c) for c in clouds] and info.id_in_strip == id_in_strip and info.offset == offset
    assert info.points_needed == offset + sum(len(c) for c in clouds)
    assert np.array_equal(pose_of(info), np.asarray(pose, np.float64), equal_nan=True)
    local, posed = R.submap_bounds(R.merge(clouds), pose)
    assert list(info.local_bound) == local.tolist(), (list(info.local_bound), local)
    assert list(info.bound) == posed.tolist(), (list(info.bound), posed)


def read_device(cloud):
    """the bytes a device-resident mulls_cloud points at, read through the HIP runtime"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros((cloud.n, abi.POINT_BYTES), np.uint8)
    if out.nbytes:
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(cloud.pts), out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def test_push_and_views_host_and_device(ctx_auto):
    """1. host clouds, the same clouds from caller-owned device buffers, and both again at a stride of 64: one store content"""
    rng = np.random.RandomState(1)
    sizes = [CH + 1, 63, 0, 64, CH - 1, 1]
    clouds = rand_submap(rng, sizes)
    pose = rigid(0.4, (3.0, -2.0, 1.0), 0.1)
    store = ctx_auto.submaps(4 * sum(sizes), 4)
    infos = [store.push(clouds, pose, id_in_strip=7)]
    bufs = [DevBuf(c) for c in clouds]
    infos.append(store.push([b.cloud() for b in bufs], pose, id_in_strip=7))
    wide = [np.concatenate([c, np.full((len(c), 16), 0xEE, np.uint8)], axis=1) for c in clouds]  # 64-byte records: the 48 bytes and a tail that stays out

    def strided(ptr, n):
        c = abi.Cloud()
        c.pts, c.n, c.stride = (ptr if n else None), n, 64
        return c

    infos.append(store.push([strided(w.ctypes.data, len(w)) for w in wide], pose, id_in_strip=7))
    wbufs = [DevBuf(w) for w in wide]
    infos.append(store.push([strided(b.p.value, b.n) for b in wbufs], pose, id_in_strip=7))
    assert store.count() == (4, 4 * sum(sizes))
    for sid, info in enumerate(infos):
        check_views(store, sid, clouds)
        check_info(info, clouds, pose, 7, sid * sum(sizes))
        assert bytes(store.info(sid)) == bytes(info) and info.submaps_needed == sid + 1
    for b in bufs + wbufs:
        b.free()
    store.clear()
    assert store.count() == (0, 0)
    check_info(store.push(clouds, pose, id_in_strip=2), clouds, pose, 2, 0)
    check_views(store, 0, clouds)
    store.close()


def special_cloud(rng, n):
    raw = rand_cloud(rng, n)
    xyz = raw[:, :12].copy().view(np.float32).reshape(n, 3)
    xyz[0] = (NAN, 1.0, 2.0)
    xyz[1] = (INF, -INF, NAN)
    xyz[2] = (-INF, INF, 5.0)
    xyz[n // 2] = (NAN, NAN, NAN)
    xyz[n - 1] = (1e30, -1e30, INF)
    raw[:, :12] = xyz.view(np.uint8).reshape(n, 12)
    return raw


def test_bounds_equal_restatement(ctx_auto):
    """2. NaN and +-inf coordinates, an all-empty submap, a vertex-only submap, translations of 1e4 m, an axis only +inf touches"""
    rng = np.random.RandomState(2)
    far = rigid(2.1, (1e4, -1e4, 1e4), -0.3)
    cases = [
        (rand_submap(rng, [65, CH, 1, 0, CH + 1, 63]), far),
        ([special_cloud(rng, CH + 1), rand_cloud(rng, 64), special_cloud(rng, 65), rand_cloud(rng, 0), rand_cloud(rng, 1), special_cloud(rng, CH - 1)], far),
        (rand_submap(rng, [0] * 6), far),
        (rand_submap(rng, [0, 0, 0, 0, 0, CH + 1]), rigid(-1.0, (5.0, 6.0, 7.0))),
        (rand_submap(rng, [0, 0, 0, 0, 0, 1]), np.eye(4)),
        (rand_submap(rng, [1, 0, 0, 0, 0, 0]), far),
    ]
    only_inf = rand_cloud(rng, 64)
    xyz = only_inf[:, :12].copy().view(np.float32).reshape(64, 3)
    xyz[:, 0], xyz[:, 1] = INF, -INF
    only_inf[:, :12] = xyz.view(np.uint8).reshape(64, 12)
    cases.append(([only_inf] + rand_submap(rng, [0] * 5), np.eye(4)))
    big = rigid(0.0, (0.0, 0.0, 0.0))
    big[:3, :3] *= 1e38  # the float store overflows to +-inf
    cases.append((rand_submap(rng, [63, 0, 0, 0, 0, 65]), big))
    store = ctx_auto.submaps(sum(sum(len(c) for c in cl) for cl, _ in cases), len(cases))
    off = 0
    for k, (clouds, pose) in enumerate(cases):
        info = store.push(clouds, pose, id_in_strip=k)
        check_info(info, clouds, pose, k, off)
        off += sum(len(c) for c in clouds)
    assert list(store.info(2).local_bound) == EMPTY_BOX and list(store.info(2).bound) == EMPTY_BOX
    assert store.info(6).local_bound[0] == DBL_MAX and store.info(6).local_bound[3] == INF and store.info(6).local_bound[4] == -DBL_MAX
    store.close()


def test_push_map_is_the_local_map(ctx_auto):
    """3. after mulls_map_set and one mulls_map_update: the clouds mulls_map_download returns, the bounds of the map's report"""
    frames = small_frames(70, n_frames=2)
    m = ctx_auto.local_map(frames[0][0], frames[0][1])
    store = ctx_auto.submaps(40000, 4)
    before = store.push_map(m, id_in_strip=3)  # set, never updated: the bounds are taken from the stored records
    clouds0 = [abi.records(m.download(c)) for c in range(6)]
    check_info(before, clouds0, m.pose(), 3, 0)
    rep = m.update(frames[1][0], frames[1][1], abi.map_params(max_num_pts=10**7, kept_vertex_num=10**6, local_map_radius=45.0))
    info = store.push_map(m, id_in_strip=4)
    clouds1 = [abi.records(m.download(c)) for c in range(6)]
    assert list(info.n) == list(rep.n) and sum(info.n) > 1500
    assert list(info.local_bound) == list(rep.local_bound) and list(info.bound) == list(rep.bound)
    check_info(info, clouds1, m.pose(), 4, sum(len(c) for c in clouds0))
    check_views(store, 0, clouds0)
    check_views(store, 1, clouds1)
    # ... and with the vertex suppression of mulls_slam.cpp:462 on the way in
    kept = ctx_auto.non_max_suppress(clouds1[5], 0.25)[0]
    info = store.push_map(m, id_in_strip=5, vertex_nms_radius=0.25)
    assert np.array_equal(store.download(2, 5), kept) and 0 < len(kept) <= len(clouds1[5])
    check_info(info, clouds1[:5] + [kept], m.pose(), 5, sum(len(c) for c in clouds0) + sum(len(c) for c in clouds1))
    m.close()
    store.close()


@pytest.fixture(scope="module")
def seventy():
    """70 submaps of mixed sizes, their first poses, their new poses (one with a NaN) and the restatement's bounds under both"""
    rng = np.random.RandomState(4)
    subs = [rand_submap(rng, [SIZES[i] for i in rng.randint(0, len(SIZES), 6)], centre=rng.uniform(-50, 50, 3)) for _ in range(70)]
    subs[11] = rand_submap(rng, [0] * 6)
    subs[12] = rand_submap(rng, [0, 0, 0, 0, 0, CH])
    total = sum(len(c) for s in subs for c in s)
    assert 100000 < total < 200000
    pose0 = [rigid(rng.uniform(-3, 3), rng.uniform(-100, 100, 3)) for _ in subs]
    pose1 = [rigid(rng.uniform(-3, 3), rng.uniform(-1e4, 1e4, 3), rng.uniform(-0.2, 0.2)) for _ in subs]
    pose1[5][1, 2] = NAN
    pose1[5][0, 0] = NAN
    pose1[5][2, 3] = NAN
    merged = [R.merge(s) for s in subs]
    b0 = [R.submap_bounds(mg, P)[1].tolist() for mg, P in zip(merged, pose0)]
    b1 = [R.submap_bounds(mg, P)[1].tolist() for mg, P in zip(merged, pose1)]
    local = [R.submap_bounds(mg, np.eye(4))[0].tolist() for mg in merged]
    return subs, total, pose0, pose1, b0, b1, local


def state(store):
    n = store.count()[0]
    infos = [store.info(k) for k in range(n)]
    return [pose_of(i) for i in infos], [list(i.bound) for i in infos], [list(i.local_bound) for i in infos]


def test_set_poses(ctx_auto, seventy):
    """4. update_optimized_nodes for 70 submaps at once, per submap, on a sub-range, without update_bbx, with a NaN pose"""
    subs, total, pose0, pose1, b0, b1, local = seventy
    store = ctx_auto.submaps(total, 70)
    for k, s in enumerate(subs):
        store.push(s, pose0[k], id_in_strip=k)
    assert state(store)[1] == b0 and state(store)[2] == local
    # one call
    store.set_poses(0, pose1, update_bbx=True)
    poses, bounds, lb = state(store)
    assert bounds == b1 and lb == local and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(poses, pose1))
    assert bounds[5] == EMPTY_BOX and bounds[11] == EMPTY_BOX
    # what pushing each submap alone at that pose reports
    single = ctx_auto.submaps(max(sum(len(c) for c in s) for s in subs), 1)
    for k, s in enumerate(subs):
        assert list(single.push(s, pose1[k]).bound) == b1[k], k
        single.clear()
    single.close()
    # back, then a call per submap
    store.set_poses(0, pose0, update_bbx=True)
    assert state(store)[1] == b0
    for k in range(70):
        store.set_poses(k, [pose1[k]], update_bbx=True)
    assert state(store)[1] == b1
    # update_bbx = 0 changes the poses only
    store.set_poses(0, pose0, update_bbx=False)
    poses, bounds, lb = state(store)
    assert bounds == b1 and lb == local and all(np.array_equal(a, b) for a, b in zip(poses, pose0))
    # a sub-range touches its submaps only
    store.set_poses(0, pose1, update_bbx=True)
    store.set_poses(10, pose0[10:30], update_bbx=True)
    poses, bounds, lb = state(store)
    assert bounds == b1[:10] + b0[10:30] + b1[30:] and lb == local
    assert all(np.array_equal(poses[k], (pose0 if 10 <= k < 30 else pose1)[k], equal_nan=True) for k in range(70))
    store.set_poses(69, [pose0[69]], update_bbx=True)
    assert state(store)[1] == b1[:10] + b0[10:30] + b1[30:69] + [b0[69]]
    store.set_poses(3, [], update_bbx=True)
    # the records never moved
    for k in (0, 12, 69):
        check_views(store, k, subs[k])
    with pytest.raises(lib.MullsError) as e:
        store.set_poses(60, pose0[:11])
    assert e.value.args[1] == abi.MULLS_E_INVALID
    store.close()


def box_cloud(half):
    """the eight corners of a box around the origin as records"""
    hx, hy, hz = half
    xyz = np.array([(sx * hx, sy * hy, sz * hz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    raw = np.zeros((8, abi.POINT_BYTES), np.uint8)
    raw[:, :12] = xyz.view(np.uint8).reshape(8, 12)
    return raw


def overlap_layout(seed):
    """40 submaps: the query (39) at the origin; duplicate centres (distance ties), identical boxes at one pose (IoU ties), centres at exactly the radius"""
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-70, 70, (40, 3))
    centres[:, 2] = rng.uniform(-20, 20, 40)
    halves = rng.uniform(10, 45, (40, 3))
    yaws = rng.uniform(-0.3, 0.3, 40)
    centres[39] = 0.0
    centres[3], centres[4] = (50.0, 0.0, 0.0), (30.0, 40.0, 1.0)  # d2 = 2500 exactly in 2-D: outside the strict radius
    centres[5] = (30.0, 39.99, 0.0)
    centres[8] = centres[7]  # distance ties
    centres[10] = centres[9] = (12.0, -9.0, 2.0)
    halves[10], yaws[10] = halves[9], yaws[9]  # ... and the same box: an IoU tie
    centres[12], halves[12], yaws[12] = centres[11], halves[11], yaws[11]
    halves[13] = (0.0, 0.0, 0.0)  # a box without area
    ids = list(range(40))
    ids[20], ids[37] = 37, 20  # id_in_strip decides adjacency, not the position in the store
    clouds = [[None, None, box_cloud(halves[k]), None, None, None] for k in range(40)]
    clouds[14] = [None] * 6  # an empty submap next to the query: never an edge
    centres[14] = (5.0, 5.0, 0.0)
    poses = [rigid(yaws[k], centres[k]) for k in range(40)]
    return clouds, poses, ids


def edges_equal(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert (g.tgt_id, g.src_id) == (w["tgt_id"], w["src_id"]) and g.overlapping_ratio == w["overlapping_ratio"], (g.tgt_id, w["tgt_id"])
        assert np.array_equal(np.array(g.Trans1_2[:]).reshape(4, 4).T, w["Trans1_2"])


@pytest.mark.parametrize("seed", [21, 22])
def test_find_overlap_equals_restatement(ctx_auto, seed):
    """5. ties in distance and in IoU, the strict radius, max_neighbor 0 / 1 / 10 / beyond the count, 2-D and 3-D, too few submaps, a short output array"""
    clouds, poses, ids = overlap_layout(seed)
    store = ctx_auto.submaps(40 * 8, 40)
    for k in range(40):
        store.push([np.zeros((0, 48), np.uint8) if c is None else c for c in clouds[k]], poses[k], id_in_strip=ids[k])
    merged = [R.merge([np.zeros((0, 48), np.uint8) if c is None else c for c in cl]) for cl in clouds]
    bounds = [R.submap_bounds(merged[k], poses[k])[1] for k in range(40)]
    assert [list(store.info(k).bound) for k in range(40)] == [b.tolist() for b in bounds]
    n_seen = 0
    for two_d in (1, 0):
        for max_nb in (0, 1, 10, 100):
            for thre, iou, radius, query in ((3, 0.25, 50.0, 39), (3, 0.0, 75.0, 39), (0, 0.05, 50.0, 39), (2, 0.1, 60.0, 30), (3, 0.25, 50.0, 3), (38, 0.0, 50.0, 39),
                                             (37, 0.0, 50.0, 39)):
                kw = dict(neighbor_search_dist=radius, min_iou_thre=iou, adjacent_id_thre=thre, search_2d=two_d, max_neighbor=max_nb)
                want = R.find_overlap(poses, bounds, ids, query, **kw)
                got, n = store.find_overlap(query, abi.overlap_params(**kw))
                assert n == len(want), kw
                edges_equal(got, want)
                n_seen += n
                if n > 1:  # a short output array: the first edges, the full count
                    short, n2 = store.find_overlap(query, abi.overlap_params(**kw), cap=n - 1)
                    assert n2 == n
                    edges_equal(short, want[: n - 1])
    assert n_seen > 100
    # the layout holds what it is meant to: the centres at exactly the radius are no neighbours, the tied ones come in id order
    want = R.find_overlap(poses, bounds, ids, 39, neighbor_search_dist=50.0, min_iou_thre=-1.0, adjacent_id_thre=0, search_2d=1, max_neighbor=0)
    tgt = [e["tgt_id"] for e in want]
    assert 3 not in tgt and 4 not in tgt and 5 in tgt and 14 in tgt
    at_zero = [e["tgt_id"] for e in R.find_overlap(poses, bounds, ids, 39, neighbor_search_dist=50.0, min_iou_thre=0.0, adjacent_id_thre=0, search_2d=1, max_neighbor=0)]
    assert 14 not in at_zero and 13 not in at_zero and 9 in at_zero
    assert tgt.index(9) + 1 == tgt.index(10) and want[tgt.index(9)]["overlapping_ratio"] == want[tgt.index(10)]["overlapping_ratio"]
    store.close()


def test_pairs_into_icp_batch(ctx_auto):
    """6. three synthetic submaps of about 3 000 points: mulls_submaps_pairs into mulls_icp_batch against the same registrations from host clouds"""
    rng = np.random.default_rng(6)
    world = planes_scene(rng, n_per=850, noise=0.01)
    truth = [rigid(0.00, (0.0, 0.0, 0.0)), rigid(0.05, (1.0, 0.5, 0.0)), rigid(-0.04, (0.4, -0.6, 0.02))]
    believed = [truth[0], truth[1], truth[2] @ rigid(0.01, (0.08, -0.05, 0.01))]  # the query's pose_lo has drifted: the registrations have work to do
    subs = []
    for k in range(3):
        local = transformed_copy(world, np.linalg.inv(truth[k]))
        keep = [None if c is None else c[rng.random(len(c)) < 0.95] for c in local]
        subs.append([abi.records(c if c is not None else np.zeros(0, abi.POINT_DTYPE)) for c in keep])
    assert all(2500 < sum(len(c) for c in s) < 3500 for s in subs)
    store = ctx_auto.submaps(sum(len(c) for s in subs for c in s), 3)
    for k in range(3):
        store.push(subs[k], believed[k], id_in_strip=k)
    kw = dict(neighbor_search_dist=50.0, min_iou_thre=0.25, adjacent_id_thre=0, search_2d=1, max_neighbor=10)
    edges, n = store.find_overlap(2, abi.overlap_params(**kw))
    merged = [R.merge(s) for s in subs]
    bnd = [R.submap_bounds(merged[k], believed[k]) for k in range(3)]
    want = R.find_overlap(believed, [b[1] for b in bnd], [0, 1, 2], 2, **kw)
    assert n == 2
    edges_equal(edges, want)
    params = abi.default_params(use_more_points=1)
    dev_pairs = store.pairs(edges)
    res_dev = ctx_auto.icp_batch(edges, params, marshalled=(dev_pairs, abi.make_result_array(n)))
    host = [abi.PairData([abi.points_of(c) for c in p["tgt"]], [abi.points_of(c) for c in p["src"]], init_guess=p["init_guess"], tgt_bound=p["tgt_bound"])
            for p in R.pairs(want, subs, [b[0] for b in bnd])]
    res_host = ctx_auto.icp_batch(host, params)
    for k in range(n):
        a, b = res_dev[k], res_host[k]
        assert same_bits(a, b), k
        assert a.code == 1 and a.iters > 1
        assert (a.singular, a.cropped, list(a.crop_box)) == (b.singular, b.cropped, list(b.crop_box)) and a.confidence == b.confidence
        for c in range(6):
            assert dev_pairs[k].src_down[c].n == 0 and not dev_pairs[k].src_down[c].pts
            assert dev_pairs[k].tgt[c].n == len(subs[edges[k].tgt_id][c]) and dev_pairs[k].src[c].n == len(subs[2][c])
        assert list(dev_pairs[k].tgt_bound) == bnd[edges[k].tgt_id][0].tolist()
        assert list(dev_pairs[k].init_guess) == list(edges[k].Trans1_2)
    store.close()


def test_views_outlive_later_pushes(ctx_auto):
    """7. the arena never moves"""
    rng = np.random.RandomState(7)
    first = rand_submap(rng, [65, 1, CH + 1, 0, 63, 64])
    store = ctx_auto.submaps(40000, 16)
    store.push(first, np.eye(4))
    views = {w: store.cloud(0, w) for w in list(range(6)) + [abi.SUBMAP_MERGED, abi.SUBMAP_MERGED_NO_GROUND]}
    want = {w: read_device(v) for w, v in views.items()}
    assert np.array_equal(want[abi.SUBMAP_MERGED], R.merge(first))
    for k in range(12):
        store.push(rand_submap(rng, [SIZES[i] for i in rng.randint(0, 6, 6)]), rigid(0.1 * k, (k, 0, 0)))
    store.set_poses(0, [rigid(0.3, (1, 2, 3))] * 13)
    for w, v in views.items():
        again = store.cloud(0, w)
        assert (again.pts, again.n) == (v.pts, v.n)
        assert np.array_equal(read_device(v), want[w]), w
    store.close()


def snapshot(store):
    n, pts = store.count()
    return n, pts, [bytes(store.info(k)) for k in range(n)], [store.download(k, abi.SUBMAP_MERGED).tobytes() for k in range(n)]


def test_refusals(ctx_auto):
    """8. a full store refuses and stays as it was; bad arguments are turned away on the host"""
    rng = np.random.RandomState(8)
    a, b = rand_submap(rng, [64, 1, 0, 65, 0, 63]), rand_submap(rng, [1, 1, 1, 1, 1, 1])
    store = ctx_auto.submaps(200, 2)
    store.push(a, rigid(0.2, (1, 2, 3)), id_in_strip=5)
    before = snapshot(store)
    with pytest.raises(lib.MullsError) as e:  # 193 + 8 > 200 points
        store.push(rand_submap(rng, [8, 0, 0, 0, 0, 0]), np.eye(4))
    assert e.value.args[1] == abi.MULLS_E_UNSUPPORTED and snapshot(store) == before
    assert (store.last_info.points_needed, store.last_info.submaps_needed, list(store.last_info.n)) == (201, 2, [8, 0, 0, 0, 0, 0])
    store.push(b, np.eye(4))
    before = snapshot(store)
    assert before[:2] == (2, 199)
    with pytest.raises(lib.MullsError) as e:  # a third submap
        store.push(rand_submap(rng, [1, 0, 0, 0, 0, 0]), np.eye(4))
    assert e.value.args[1] == abi.MULLS_E_UNSUPPORTED and snapshot(store) == before
    assert (store.last_info.points_needed, store.last_info.submaps_needed) == (200, 3)
    with pytest.raises(lib.MullsError) as e:  # an empty one does not fit either
        store.push(rand_submap(rng, [0] * 6), np.eye(4))
    assert e.value.args[1] == abi.MULLS_E_UNSUPPORTED and snapshot(store) == before

    L, h = ctx_auto.lib, ctx_auto.h
    arr = (abi.Cloud * 6)()
    for c in range(6):
        arr[c].pts, arr[c].n, arr[c].stride = a[c].ctypes.data if len(a[c]) else None, len(a[c]), 48
    pose, info = abi.colmajor16(np.eye(4)), abi.SubmapInfo()
    other = lib.Context(0)
    assert L.mulls_submaps_push(other.h, store.h, arr, pose, 0, 0.0, C.byref(info)) == abi.MULLS_E_INVALID  # a store of another context
    assert L.mulls_submaps_count(other.h, store.h, None, None) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_set_poses(other.h, store.h, 0, 1, pose, 1) == abi.MULLS_E_INVALID
    other.close()
    assert L.mulls_submaps_push(h, None, arr, pose, 0, 0.0, C.byref(info)) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_push(h, store.h, None, pose, 0, 0.0, C.byref(info)) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_push(h, store.h, arr, None, 0, 0.0, C.byref(info)) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_push(h, store.h, arr, pose, 0, 0.0, None) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_push(None, store.h, arr, pose, 0, 0.0, C.byref(info)) == abi.MULLS_E_INVALID
    arr[0].stride = 44
    assert L.mulls_submaps_push(h, store.h, arr, pose, 0, 0.0, C.byref(info)) == abi.MULLS_E_INVALID  # a stride under 48
    arr[0].stride = 50
    assert L.mulls_submaps_push(h, store.h, arr, pose, 0, 0.0, C.byref(info)) == abi.MULLS_E_INVALID  # ... or no multiple of 4
    arr[0].stride = 48
    arr[1].pts = None
    assert L.mulls_submaps_push(h, store.h, arr, pose, 0, 0.0, C.byref(info)) == abi.MULLS_E_INVALID  # points and no address
    arr[1].pts = a[1].ctypes.data
    for radius in (-0.25, NAN, INF):
        assert L.mulls_submaps_push(h, store.h, arr, pose, 0, radius, C.byref(info)) == abi.MULLS_E_INVALID
    cl, n = abi.Cloud(), C.c_uint32(0)
    for sid, which in ((2, 0), (0, 8), (0, -1), (4000000000, 0)):
        assert L.mulls_submaps_cloud(h, store.h, sid, which, C.byref(cl)) == abi.MULLS_E_INVALID
        assert L.mulls_submaps_download(h, store.h, sid, which, None, 0, C.byref(n)) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_info(h, store.h, 2, C.byref(info)) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_cloud(h, store.h, 0, 0, None) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_set_poses(h, store.h, 0, 1, None, 1) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_set_poses(h, store.h, 1, 2, pose, 1) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_push_map(h, store.h, None, 0, 0.0, C.byref(info)) == abi.MULLS_E_INVALID
    P, ne = abi.overlap_params(), C.c_uint32(0)
    assert L.mulls_submaps_find_overlap(h, store.h, 2, C.byref(P), None, 0, C.byref(ne)) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_find_overlap(h, store.h, 1, None, None, 0, C.byref(ne)) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_find_overlap(h, store.h, 1, C.byref(P), None, 0, None) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_find_overlap(h, store.h, 1, C.byref(P), None, 3, C.byref(ne)) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_find_overlap(h, store.h, 1, C.byref(abi.overlap_params(neighbor_search_dist=NAN)), None, 0, C.byref(ne)) == abi.MULLS_E_INVALID
    edge, pair = abi.SubmapEdge(), abi.Pair()
    edge.tgt_id, edge.src_id = 0, 2
    assert L.mulls_submaps_pairs(h, store.h, C.byref(edge), 1, C.byref(pair)) == abi.MULLS_E_INVALID
    assert L.mulls_submaps_pairs(h, store.h, None, 1, C.byref(pair)) == abi.MULLS_E_INVALID
    assert snapshot(store) == before
    store.close()


@pytest.mark.parametrize("n", [9, 300, CH + 1])
def test_vertex_nms_on_push(ctx_auto, n):
    """9. vertex_nms_radius 0.25: the stored vertex cloud is mulls_non_max_suppress's output, byte for byte (below its gate of 10 points: the cloud as given)"""
    rng = np.random.RandomState(90 + n)
    clouds = rand_submap(rng, [65, 0, 64, 0, 1, 0])
    vertex = rand_cloud(rng, n, scale=1.0)
    vertex[:, 28:32] = rng.uniform(0.0, 1.0, n).astype(np.float32).view(np.uint8).reshape(n, 4)  # the key: normal[3]
    clouds[5] = vertex
    kept = ctx_auto.non_max_suppress(vertex, 0.25)[0]
    assert (len(kept) == n) == (n < 10)
    pose = rigid(0.5, (10.0, 20.0, 30.0))
    store = ctx_auto.submaps(2 * (130 + n), 2)
    info = store.push(clouds, pose, id_in_strip=1, vertex_nms_radius=0.25)
    stored = clouds[:5] + [kept]
    assert np.array_equal(store.download(0, 5), kept)
    check_info(info, stored, pose, 1, 0)
    check_views(store, 0, stored)
    buf = DevBuf(vertex)  # the same from a device-resident vertex cloud
    info = store.push(clouds[:5] + [buf.cloud()], pose, id_in_strip=2, vertex_nms_radius=0.25)
    buf.free()
    check_info(info, stored, pose, 2, 130 + len(kept))
    check_views(store, 1, stored)
    store.close()
