"""The device-resident local map on the inputs of tests/map_edges.py: clouds of several compaction segments (up to two trips of the segment
scan), trees of one to four search chunks with queries exactly on the removal's thresholds, neighbour lists with ties at rank K, duplicates and
a neighbour exactly on the radius, bounds of an empty map and of a cloud beyond one trip of the bounds' grid, and the C ABI by raw calls (packed
strides, short downloads, NULL arguments, device-resident sources).  The rule is the project's: device == oracle on every field of every record
of all six map clouds and all six appended frame clouds, and on every figure of the report, after every update.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import map_edges as E
from mulls_amd import abi, synth
from oracle import pyoracle
from test_gpu_map import drive
from test_gpu_map_batch import against_oracle, same_report, state
from test_map import same_cloud, small_frames

pytestmark = pytest.mark.gpu


def run(ctx, case):
    """drive() compares all twelve clouds, the report and the pose after every update, and normal[3] of the linear classes where the refresh writes it"""
    return drive(ctx, case.sequence(), lambda k: case.params[k - 1])


# ------------------------------------------------------------------------------------------------------------------------------ S: segments
def test_radius_filter_over_many_segments_then_registration(ctx_auto):
    """S(a): 66 + 2 + 2 + 1 + 1 + 4 segments through the radius filter, every keep pattern, twice; then a registration against the
    multi-segment resident map == the same registration with the map uploaded from the host."""
    case = E.scene_s("a")
    dev, clouds, reps = run(ctx_auto, case)
    assert E.segments(reps[0].n[abi.GROUND]) > 1 and E.segments(reps[1].n[abi.GROUND]) > 1
    T = synth.se3(0.2, -0.1, 0.03, 0.0, 0.0, np.deg2rad(0.5))
    src = [pyoracle.transform(clouds[c][::40], T) for c in range(6)]
    host_pair = abi.PairData(clouds, src)
    P = abi.kitti_params(dis_thre_unit=2.4)
    r_host = ctx_auto.icp(host_pair, P)[0]
    r_dev = dev.icp(src, P, tgt_bound=host_pair.tgt_bound)[0]
    assert (r_dev.code, r_dev.iters, list(r_dev.ncorr)) == (r_host.code, r_host.iters, list(r_host.ncorr))
    assert r_dev.T[:] == r_host.T[:] and r_dev.info[:] == r_host.info[:] and r_dev.sigma == r_host.sigma
    assert list(r_dev.ntgt0) == list(r_host.ntgt0) and sum(r_dev.ncorr) > 0
    dev.close()


@pytest.mark.parametrize("variant", ["b", "c"])
def test_thinning_masks_over_many_segments(ctx_auto, variant):
    """S(b): mask mode over more than 64 segments, twice on the same map; S(c): radius mode, then mask mode on what it left"""
    dev, _, reps = run(ctx_auto, E.scene_s(variant))
    assert reps[-1].n[abi.VERTEX] == E.scene_s(variant).params[-1].kept_vertex_num
    dev.close()


def test_removal_of_multi_segment_frame_clouds(ctx_auto):
    """S(d): the verdicts of an 8193-, a 300- and a 4097-point frame cloud side by side in one array, compacted in one launch set"""
    case = E.scene_s_removal()
    dev, _, reps = run(ctx_auto, case)
    assert reps[0].dynamic_removal_ran == 1
    assert all(0 < reps[0].frame_n[c] < len(case.frames[0][0][c]) for c in E.N_ORDER)
    dev.close()


def test_pca_refresh_compacts_across_a_segment_edge(ctx_auto):
    case = E.scene_s_pca()
    dev, _, reps = run(ctx_auto, case)
    assert 0 < reps[0].n[abi.PILLAR] < len(case.map_clouds[abi.PILLAR])
    dev.close()


# ------------------------------------------------------------------------------------------------------------ N: nearest tree point
@pytest.mark.parametrize("i", range(len(E.N_COMBOS)))
def test_nearest_tree_point_at_chunk_and_tile_edges(ctx_auto, i):
    case = E.scene_n(i)
    dev, _, reps = run(ctx_auto, case)
    assert reps[0].dynamic_removal_ran == 1
    dev.close()


# ------------------------------------------------------------------------------------------------------------------- P: neighbour lists
@pytest.mark.parametrize("order", E.P_ORDERS)
@pytest.mark.parametrize("n", E.P_SIZES)
def test_neighbour_lists_with_ties_duplicates_and_the_radius_itself(ctx_auto, n, order):
    case = E.scene_p(n, order)
    dev, _, reps = run(ctx_auto, case)
    assert 0 < reps[0].n[abi.PILLAR] < n and 0 < reps[0].n[abi.BEAM] < n
    dev.close()


@pytest.mark.parametrize("n", E.P_SIZES)
def test_neighbour_lists_control_without_ties(ctx_auto, n):
    run(ctx_auto, E.scene_p(n, "random", True))[0].close()


# --------------------------------------------------------------------------------------------------------------- B: bounds and empties
@pytest.mark.parametrize("name", E.B_NAMES)
def test_bounds_and_empties(ctx_auto, name):
    dev, clouds, reps = run(ctx_auto, E.scene_b(name))
    if name in ("filtered_away", "empty"):
        big = np.finfo(np.float64).max
        assert list(reps[0].local_bound) == list(reps[0].bound) == [big] * 3 + [-big] * 3 and reps[0].feature_point_num == 0
    dev.close()


# ------------------------------------------------------------------------------------------------------------------------- A: the C ABI
GUARD = 0xA5


def strided(cloud, stride=64):
    """(buffer, mulls_cloud): the records `stride` bytes apart with guard bytes between them"""
    raw = abi.records(cloud)
    buf = np.full((len(raw), stride), GUARD, np.uint8)
    buf[:, :abi.POINT_BYTES] = raw
    c = abi.Cloud()
    c.pts, c.n, c.stride = (buf.ctypes.data if len(raw) else None), len(raw), stride
    return buf, c


def raw_map(ctx):
    h = C.c_void_p()
    assert ctx.lib.mulls_map_create(ctx.h, C.byref(h)) == abi.MULLS_OK
    return h


def raw_download(ctx, fn, h, cls):
    n = C.c_uint32(0)
    assert fn(ctx.h, h, cls, None, 0, C.byref(n)) == abi.MULLS_OK  # cap 0: the size alone
    out = np.zeros(n.value, abi.POINT_DTYPE)
    if n.value:
        assert fn(ctx.h, h, cls, out.ctypes.data_as(C.c_void_p), n.value, None) == abi.MULLS_OK  # n NULL
    return out


def test_abi_strided_sources_and_untouched_inputs(ctx_auto):
    """mulls_map_set and mulls_map_update from stride-64 records (the pack path): the results are the oracle's on the plain records, and the
    caller's arrays -- guard bytes included -- are as they were"""
    ctx, lib = ctx_auto, ctx_auto.lib
    case = E.scene_n(3)
    fc, fp = case.frames[0]
    m_buf, f_buf = [strided(c) for c in case.map_clouds], [strided(c) for c in fc]
    m_arr, f_arr = (abi.Cloud * 6)(*[c for _, c in m_buf]), (abi.Cloud * 6)(*[c for _, c in f_buf])
    before = [b.copy() for b, _ in m_buf + f_buf]
    h = raw_map(ctx)
    rep = abi.MapReport()
    assert lib.mulls_map_set(ctx.h, h, m_arr, abi.colmajor16(case.map_pose)) == abi.MULLS_OK
    assert lib.mulls_map_update(ctx.h, h, f_arr, abi.colmajor16(fp), C.byref(case.params[0]), C.byref(rep)) == abi.MULLS_OK
    assert all(np.array_equal(a, b) for a, (b, _) in zip(before, m_buf + f_buf))
    clouds, appended, ro = pyoracle.map_update(case.map_clouds, case.map_pose, fc, fp, case.params[0])
    assert list(rep.n) == list(ro.n) and list(rep.frame_n) == list(ro.frame_n) and rep.feature_point_num == ro.feature_point_num
    assert list(rep.local_bound) == list(ro.local_bound) and list(rep.bound) == list(ro.bound) and rep.dynamic_removal_ran == ro.dynamic_removal_ran == 1
    for c in range(6):
        same_cloud(raw_download(ctx, lib.mulls_map_download, h, c), clouds[c])
        same_cloud(raw_download(ctx, lib.mulls_map_frame_download, h, c), appended[c])
    lib.mulls_map_destroy(ctx.h, h)


def test_abi_short_downloads(ctx_auto):
    """cap < n: exactly cap records are written, the record behind them is untouched, *n is the full size"""
    ctx, lib = ctx_auto, ctx_auto.lib
    case = E.scene_n(0)
    dev = ctx.local_map(case.map_clouds, case.map_pose)
    dev.update(case.frames[0][0], case.frames[0][1], case.params[0])
    for fn, full_of in ((lib.mulls_map_download, dev.download), (lib.mulls_map_frame_download, dev.frame_download)):
        for cls in (abi.GROUND, abi.FACADE):
            full = full_of(cls)
            assert len(full) > 40
            for cap in (1, 17, len(full) - 1):
                buf = np.full((cap + 1, abi.POINT_BYTES), GUARD, np.uint8)
                n = C.c_uint32(0)
                assert fn(ctx.h, dev.h, cls, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == abi.MULLS_OK
                assert n.value == len(full)
                assert np.array_equal(buf[:cap], abi.records(full)[:cap]) and np.all(buf[cap] == GUARD)
            n = C.c_uint32(0)
            assert fn(ctx.h, dev.h, cls, None, 0, C.byref(n)) == abi.MULLS_OK and n.value == len(full)
            assert fn(ctx.h, dev.h, cls, None, 0, None) == abi.MULLS_OK
            assert fn(ctx.h, dev.h, cls, None, 5, C.byref(n)) == abi.MULLS_E_INVALID  # records asked for, nowhere to put them
    dev.close()


def test_abi_null_arguments_and_class_range(ctx_auto):
    ctx, lib = ctx_auto, ctx_auto.lib
    case = E.scene_n(0)
    fc, fp = case.frames[0]
    keep = [abi.as_points(c) for c in case.map_clouds] + [abi.as_points(c) for c in fc]
    m_arr, f_arr = (abi.Cloud * 6)(*[abi.as_cloud(c) for c in keep[:6]]), (abi.Cloud * 6)(*[abi.as_cloud(c) for c in keep[6:]])
    pose, P, rep, h = abi.colmajor16(fp), case.params[0], abi.MapReport(), raw_map(ctx)
    out_h, cl, n, p16 = C.c_void_p(), abi.Cloud(), C.c_uint32(0), (C.c_double * 16)()
    buf = np.zeros((8, abi.POINT_BYTES), np.uint8)
    bad = abi.MULLS_E_INVALID
    assert lib.mulls_map_create(None, C.byref(out_h)) == bad and lib.mulls_map_create(ctx.h, None) == bad
    set_args = [ctx.h, h, m_arr, pose]
    upd_args = [ctx.h, h, f_arr, pose, C.byref(P), C.byref(rep)]
    for fn, args, pointers in ((lib.mulls_map_set, set_args, range(4)), (lib.mulls_map_update, upd_args, range(6)),
                               (lib.mulls_map_cloud, [ctx.h, h, 0, C.byref(cl)], (0, 1, 3)), (lib.mulls_map_pose, [ctx.h, h, p16], range(3))):
        for k in pointers:
            assert fn(*[None if j == k else a for j, a in enumerate(args)]) == bad, (fn.__name__, k)
    for fn in (lib.mulls_map_download, lib.mulls_map_frame_download):
        assert fn(None, h, 0, buf.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == bad and fn(ctx.h, None, 0, buf.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == bad
        for cls in (-1, 6, 1 << 20):
            assert fn(ctx.h, h, cls, buf.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == bad
    for cls in (-1, 6, 1 << 20):
        assert lib.mulls_map_cloud(ctx.h, h, cls, C.byref(cl)) == bad
    short = abi.map_params(used_feature_type="111")
    assert lib.mulls_map_update(ctx.h, h, f_arr, pose, C.byref(short), C.byref(rep)) == bad
    thin = abi.Cloud()
    thin.pts, thin.n, thin.stride = keep[0].ctypes.data, 4, 47  # a stride below the record
    arr = (abi.Cloud * 6)(*([thin] + [abi.as_cloud(None)] * 5))
    assert lib.mulls_map_set(ctx.h, h, arr, pose) == bad
    nowhere = abi.Cloud()
    nowhere.pts, nowhere.n, nowhere.stride = None, 4, 48
    arr = (abi.Cloud * 6)(*([nowhere] + [abi.as_cloud(None)] * 5))
    assert lib.mulls_map_update(ctx.h, h, arr, pose, C.byref(P), C.byref(rep)) == bad
    # none of it left the map unusable
    assert lib.mulls_map_set(ctx.h, h, m_arr, abi.colmajor16(case.map_pose)) == abi.MULLS_OK
    assert lib.mulls_map_update(ctx.h, h, f_arr, pose, C.byref(P), C.byref(rep)) == abi.MULLS_OK
    ro = pyoracle.map_update(case.map_clouds, case.map_pose, fc, fp, P)[2]
    assert list(rep.n) == list(ro.n) and list(rep.frame_n) == list(ro.frame_n)
    lib.mulls_map_destroy(ctx.h, h)


def test_abi_device_resident_sources_mixed_with_host_strides(ctx_auto):
    """A second map set from the first map's mulls_map_cloud clouds, updated with frame clouds that are device-resident (a third map's),
    host stride 48 and host stride 64 within one call == the all-host call == the oracle"""
    ctx = ctx_auto
    case = E.scene_n(3)
    fc, fp = case.frames[0]
    first = ctx.local_map(case.map_clouds, case.map_pose)
    second = ctx.local_map([first.cloud(c) for c in range(6)], case.map_pose)
    third = ctx.local_map(fc, fp)  # the frame's clouds, resident
    for c in range(6):
        same_cloud(second.download(c), abi.as_points(case.map_clouds[c]))
    bufs = {c: strided(fc[c]) for c in (abi.FACADE, abi.VERTEX)}
    mixed = [third.cloud(abi.GROUND), fc[abi.PILLAR], bufs[abi.FACADE][1], third.cloud(abi.BEAM), fc[abi.ROOF], bufs[abi.VERTEX][1]]
    r2 = second.update(mixed, fp, case.params[0])
    r1 = first.update(fc, fp, case.params[0])
    clouds, appended, ro = pyoracle.map_update(case.map_clouds, case.map_pose, fc, fp, case.params[0])
    for r in (r1, r2):
        assert list(r.n) == list(ro.n) and list(r.frame_n) == list(ro.frame_n) and r.feature_point_num == ro.feature_point_num
        assert list(r.local_bound) == list(ro.local_bound) and list(r.bound) == list(ro.bound) and r.dynamic_removal_ran == ro.dynamic_removal_ran
    for c in range(6):
        for m in (first, second):
            same_cloud(m.download(c), clouds[c])
            same_cloud(m.frame_download(c), appended[c])
        same_cloud(third.download(c), abi.as_points(fc[c]))  # lending its clouds changed nothing in the third map
    for m in (first, second, third):
        m.close()


# ------------------------------------------------------------------------------------------- the single call: refusals and lent device clouds
def refused_for_a_bad_cloud(ctx):
    """A map updated once, then an update whose class 3 has four points and no pointer behind three valid classes of 1, 257 and 0 records: the status, the
    text, the zeroed report, and map clouds, counts and pose as they were.  Returns what the caller may ask beyond that.
    The first update refreshes the pillars, whose cloud holds one point far from every other: it sets the report's upper x bound (the bounds are taken before
    the refresh) and the refresh drops it, so bounds carried by has_bounds differ from bounds taken from the records."""
    lib = ctx.lib
    frames = small_frames(90, n_frames=3)
    start = [abi.as_points(c) for c in frames[0][0]]
    start[abi.PILLAR] = np.concatenate([start[abi.PILLAR], E.records(np.array([[75.0, 0.0, 1.0]]), 90)])
    m = ctx.local_map(start, frames[0][1])
    P = abi.map_params(recalculate_feature_on=1, max_num_pts=10**7, kept_vertex_num=10**6, local_map_radius=80.0)
    rep0 = m.update(frames[1][0], frames[1][1], P)
    store = ctx.submaps(40000, 4)
    info = store.push_map(m, id_in_strip=0)
    kept_x = np.concatenate([E.xyz_of(m.download(c))[:, 0] for c in range(6)])
    assert list(info.local_bound) == list(rep0.local_bound) and rep0.local_bound[3] > float(kept_x.max()) + 1.0
    before = state(m)
    sizes = [m.cloud(c).n for c in range(6)]
    fc = [abi.as_points(c) for c in frames[2][0]]
    held = [fc[0][:1], fc[abi.FACADE][:257], fc[2][:0]]  # (any records do: the call is refused before it looks at them)
    assert [len(h) for h in held] == [1, 257, 0]
    nowhere = abi.Cloud()
    nowhere.pts, nowhere.n, nowhere.stride = None, 4, 48
    arr = (abi.Cloud * 6)(*([abi.as_cloud(h) for h in held] + [nowhere, abi.as_cloud(None), abi.as_cloud(None)]))
    rep = abi.MapReport()
    C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
    rc = lib.mulls_map_update(ctx.h, m.h, arr, abi.colmajor16(frames[2][1]), C.byref(P), C.byref(rep))
    assert rc == abi.MULLS_E_INVALID
    assert lib.mulls_last_error(ctx.h) == b"cloud with points but null pointer or stride < 48"
    assert bytes(rep) == bytes(C.sizeof(rep))
    after = state(m)
    assert after[0] == before[0] and after[2] == before[2] and [m.cloud(c).n for c in range(6)] == sizes
    return m, store, before, after, rep0


def test_single_call_refused_for_a_bad_cloud_leaves_the_map_untouched(ctx_auto):
    m, store, before, after, rep0 = refused_for_a_bad_cloud(ctx_auto)
    assert after[1] == before[1]  # the frame clouds of the update before it
    info = store.push_map(m, id_in_strip=1)  # has_bounds still set: the archive carries the report's bounds, not the records'
    assert list(info.local_bound) == list(rep0.local_bound) and list(info.bound) == list(rep0.bound)
    store.close()
    m.close()


def test_single_call_with_another_maps_device_clouds_as_the_frame(ctx_auto):
    """all six frame clouds lent by another map of the context == the same update from host copies == the oracle"""
    ctx = ctx_auto
    frames = small_frames(110, n_frames=2)
    (mc, mp), (fc, fp) = frames
    P = abi.map_params(max_num_pts=1800, kept_vertex_num=130, local_map_radius=35.0, rng_seed=12, map_based_dynamic_removal_on=1, tree_mode=1,
                       tree_used="111110")
    lender = ctx.local_map(fc, fp)
    lent, hosted = ctx.local_map(mc, mp), ctx.local_map(mc, mp)
    r_lent = lent.update([lender.cloud(c) for c in range(6)], fp, P)
    r_host = hosted.update(fc, fp, P)
    same_report(r_lent, r_host)
    assert state(lent) == state(hosted) and r_lent.dynamic_removal_ran == 1
    clouds, appended, ro = pyoracle.map_update(mc, mp, fc, fp, P)
    against_oracle(lent, r_lent, clouds, appended, ro, P, fp)
    for c in range(6):
        same_cloud(lender.download(c), abi.as_points(fc[c]))
    for m in (lender, lent, hosted):
        m.close()


def test_single_call_with_the_maps_own_vertex_cloud_as_the_frame(ctx_auto):
    """the vertex frame cloud is mulls_map_cloud(map, VERTEX) of the map being updated: accepted, and the bytes of the update from a host copy of it"""
    ctx = ctx_auto
    frames = small_frames(120, n_frames=2)
    (mc, mp), (fc, fp) = frames
    P = abi.map_params(max_num_pts=10**7, kept_vertex_num=10**6, local_map_radius=60.0)
    own, hosted = ctx.local_map(mc, mp), ctx.local_map(mc, mp)
    vertex = hosted.download(abi.VERTEX)
    assert len(vertex) == own.cloud(abi.VERTEX).n > 0
    r_own = own.update(list(fc[:5]) + [own.cloud(abi.VERTEX)], fp, P)
    r_host = hosted.update(list(fc[:5]) + [vertex], fp, P)
    same_report(r_own, r_host)
    assert state(own) == state(hosted) and r_own.n[abi.VERTEX] > 0
    own.close()
    hosted.close()
