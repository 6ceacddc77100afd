"""mulls_map_update_batch against mulls_map_update: every case drives twin maps with single calls and asks for the same bytes — all six class clouds, the six
frame clouds, the pose and the report without ms_total — after every batched update, and holds at least one item per case to the oracle as test_gpu_map.drive
does.  mulls_map_update runs as a batch of one, so the twin comparison states "a batch of N equals N batches of one"; what holds both to the bytes the
separate single path left behind is tests/golden/map_update_digests.json: a SHA-256 per stream and step over state(map) and the report up to ms_total, pad
words included, recorded from single calls before that path was removed (record_digests, run by hand: see the end of this module).
Inputs are the generators that exist: test_map.small_frames / linear_frames and the scenes of tests/map_edges.py.  No tolerance anywhere."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import map_edges as E
from mulls_amd import abi, synth
from oracle import pyoracle
from test_map import linear_frames, same_cloud, small_frames

pytestmark = pytest.mark.gpu

REPORT_BYTES = abi.MapReport.ms_total.offset  # every field before ms_total; no padding in front of it


class Stream:
    """one map and the updates folded into it: steps[k] = (six frame clouds, pose, params)"""

    def __init__(self, clouds, pose, steps):
        self.clouds, self.pose, self.steps = [abi.as_points(c) for c in clouds], np.asarray(pose, np.float64), list(steps)


def of_case(case, **override):
    steps = []
    for (fc, fp), P in zip(case.frames, case.params):
        if override:
            P = clone(P, **override)
        steps.append((fc, fp, P))
    return Stream(case.map_clouds, case.map_pose, steps)


def of_frames(frames, params_of):
    return Stream(frames[0][0], frames[0][1], [(fc, fp, params_of(k)) for k, (fc, fp) in enumerate(frames[1:], 1)])


def clone(P, **kw):
    q = abi.MapParams()
    C.memmove(C.byref(q), C.byref(P), C.sizeof(q))
    for k, v in kw.items():
        if k == "tree_box":
            for i in range(6):
                q.tree_box[i] = float(v[i])
        else:
            setattr(q, k, v.encode() if isinstance(v, str) else v)
    return q


def state(m):
    """everything an update leaves behind in a map, as bytes"""
    return [m.download(c).tobytes() for c in range(6)], [m.frame_download(c).tobytes() for c in range(6)], m.pose().tobytes()


def digest(m, rep):
    """SHA-256 over everything state() returns (each part behind its length) and the report up to ms_total"""
    clouds, frames, pose = state(m)
    h = hashlib.sha256()
    for part in clouds + frames + [pose, bytes(rep)[:REPORT_BYTES]]:
        h.update(len(part).to_bytes(8, "little"))
        h.update(part)
    return h.hexdigest()


DIGEST_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_update_digests.json")
_recorded = {}


def recorded(key):
    """the digests of stream `key` ("case/index"), one per step"""
    if not _recorded:
        with open(DIGEST_FILE) as f:
            _recorded.update(json.load(f))
    return _recorded[key]


def same_report(a, b):
    assert bytes(a)[:REPORT_BYTES] == bytes(b)[:REPORT_BYTES]


def against_oracle(m, rep, clouds, appended, ro, P, pose):
    assert list(rep.n) == list(ro.n) and list(rep.frame_n) == list(ro.frame_n)
    assert rep.feature_point_num == ro.feature_point_num and rep.dynamic_removal_ran == ro.dynamic_removal_ran
    assert list(rep.local_bound) == list(ro.local_bound) and list(rep.bound) == list(ro.bound)
    for c in range(6):
        same_cloud(m.download(c), clouds[c])
        same_cloud(m.frame_download(c), appended[c])
        if P.recalculate_feature_on and c in (abi.PILLAR, abi.BEAM):
            assert np.array_equal(abi.normal3(m.download(c)), abi.normal3(clouds[c]))
    assert np.array_equal(m.pose(), pose)


# the streams of each case held to the oracle: every one
ORACLE = {"mixed": range(5), "removal": range(9), "refresh": range(7), "capacity": range(11), "seven": range(7), "random": range(4)}


def lockstep(ctx, streams, oracle=(0,), max_lockstep=0, shared=None, digests=None):
    """Every stream's k-th update as ONE batch per k; twins by single calls; the streams named in `oracle` also against pyoracle.map_update.
    shared: (index, params) — that stream passes no params of its own.  digests: a case of DIGEST_CASES (its streams in order) or one key of the recorded
    digests per stream — the batched map and the twin both have the recorded digest after every step.  Returns the per-step list of (reports, stats) and the maps."""
    if isinstance(digests, str):
        digests = ["%s/%d" % (digests, i) for i in range(len(streams))]
    maps = [ctx.local_map(s.clouds, s.pose) for s in streams]
    twins = [ctx.local_map(s.clouds, s.pose) for s in streams]
    host = {i: ([c.copy() for c in streams[i].clouds], streams[i].pose) for i in oracle}
    out = []
    for k in range(max(len(s.steps) for s in streams)):
        live = [i for i, s in enumerate(streams) if k < len(s.steps)]
        steps = [streams[i].steps[k] for i in live]
        params = [None if (shared is not None and shared[0] == i) else st[2] for i, st in zip(live, steps)]
        frames = [st[0] for st in steps]
        reps, stats = ctx.map_update_batch([maps[i] for i in live], frames, [st[1] for st in steps], params, max_lockstep=max_lockstep,
                                           shared_params=None if shared is None else shared[1])
        assert stats.n_lockstep == len(live) and stats.n_single_path == 0
        for j, i in enumerate(live):
            fc, fp, P = steps[j]
            rt = twins[i].update(fc, fp, P)
            same_report(reps[j], rt)
            assert state(maps[i]) == state(twins[i]), (k, i)
            if digests is not None:
                assert digest(maps[i], reps[j]) == digest(twins[i], rt) == recorded(digests[i])[k], (k, i, digests[i])
            if i in host:
                clouds, appended, ro = pyoracle.map_update(host[i][0], host[i][1], fc, fp, P)
                host[i] = (clouds, fp)
                against_oracle(maps[i], reps[j], clouds, appended, ro, P, fp)
        out.append((reps, stats))
    return out, maps, twins


def close(*groups):
    for g in groups:
        for m in g:
            m.close()


# ------------------------------------------------------------------------------------------------------------------------------- parameters
def mixed_streams():
    """(the last stream passes no params of its own: its steps' params are the batch's shared ones)"""
    wide = dict(max_num_pts=10**7, kept_vertex_num=10**6)
    per_stream = [
        lambda k: abi.map_params(used_feature_type="111110", local_map_radius=45.0, **wide),
        lambda k: abi.map_params(used_feature_type="101000", max_num_pts=1800, kept_vertex_num=130, local_map_radius=35.0, rng_seed=1000 + k),
        lambda k: abi.map_params(used_feature_type="111111", max_num_pts=1200, kept_vertex_num=40, local_map_radius=60.0, rng_seed=7 + k),
        lambda k: abi.map_params(local_map_radius=25.0, **wide),
    ]
    shared = abi.map_params(max_num_pts=2500, kept_vertex_num=10**6, local_map_radius=80.0, rng_seed=5)
    streams = [of_frames(small_frames(40 + 10 * i, n_frames=4), per_stream[i]) for i in range(4)]
    streams.append(of_frames(small_frames(95, n_frames=4), lambda k: shared))
    return streams


def test_mixed_parameters_three_updates_five_maps(ctx_auto):
    streams = mixed_streams()
    out, maps, twins = lockstep(ctx_auto, streams, oracle=ORACLE["mixed"], shared=(4, streams[4].steps[0][2]), digests="mixed")
    assert len(out) == 3 and out[-1][0][1].n[5] == 130 and out[-1][0][4].feature_point_num <= 2505
    close(maps, twins)


# ---------------------------------------------------------------------------------------------------------------------------- dynamic removal
def removal_streams():
    n0 = E.scene_n(0)
    no_pillars = E.Case("N(0) without map pillars", [E.empty() if c == abi.PILLAR else n0.map_clouds[c] for c in range(6)], n0.map_pose, n0.frames, n0.params)
    return [
        of_case(n0),  # tree_mode 1; frame classes of 11, 257 and 1001 points
        of_case(E.scene_n(1)),  # a facade of 10 points: not searched
        of_case(E.scene_n(2)),  # tree_mode 2
        of_case(E.scene_n(4)),  # tree_used skips the facade
        of_case(E.scene_n(5)),  # another box: no tree point inside
        of_case(E.scene_n(2), tree_mode=0),  # no tree state: the removal does not run
        of_case(n0, max_num_pts=10**7),  # fpn0 <= max_num_pts / 5: the removal does not run
        of_case(no_pillars),  # an empty map class
        of_case(E.scene_n(7), tree_box=[-8.0, -8.0, -0.5, 8.0, 8.0, 20.0]),
    ]


def test_dynamic_removal_in_one_batch(ctx_auto):
    n0 = E.scene_n(0)
    streams = removal_streams()
    out, maps, twins = lockstep(ctx_auto, streams, oracle=ORACLE["removal"], digests="removal")
    reps = out[0][0]
    assert [r.dynamic_removal_ran for r in reps] == [1, 1, 1, 1, 1, 0, 0, 1, 1]
    assert reps[1].frame_n[abi.FACADE] == 10 and reps[7].frame_n[abi.PILLAR] == len(n0.frames[0][0][abi.PILLAR])
    # the threshold queries: the kept points of the searched classes are the rule's, stated in numpy
    fc, _, P = streams[0].steps[0]
    for c in E.N_ORDER:
        keep = E.removal_verdict(E.xyz_of(fc[c]), E.xyz_of(n0.map_clouds[c]), P)[0]
        assert reps[0].frame_n[c] == int(keep.sum()) and same_cloud(maps[0].frame_download(c), abi.as_points(fc[c])[keep]) is None
    assert any(reps[0].frame_n[c] < len(fc[c]) for c in E.N_ORDER)
    close(maps, twins)


# ------------------------------------------------------------------------------------------------------------------------------- PCA refresh
def refresh_streams():
    kw = dict(max_num_pts=10**7, kept_vertex_num=10**6, local_map_radius=60.0)
    return [
        of_frames(linear_frames(310, n_frames=3), lambda k: abi.map_params(recalculate_feature_on=1, used_feature_type="111110" if k != 2 else "110010", **kw)),
        of_frames(linear_frames(320, n_frames=3), lambda k: abi.map_params(recalculate_feature_on=0, **kw)),
        of_frames(linear_frames(330, n_frames=3), lambda k: abi.map_params(recalculate_feature_on=k % 2, max_num_pts=2500, kept_vertex_num=60, rng_seed=77,
                                                                           local_map_radius=60.0)),
        of_case(E.scene_p(255, "random")),
        of_case(E.scene_p(256, "ascending")),
        of_case(E.scene_p(257, "descending")),
        of_case(E.scene_p(257, "random"), recalculate_feature_on=0),
    ]


def test_pca_refresh_mixed_on_and_off(ctx_auto):
    streams = refresh_streams()
    ties = E.neighbour_lists(E.scene_p(256, "ascending").pillar_xyz)
    assert np.any(ties["tie_at_k"])  # neighbourhoods whose rank-K candidate has an equal
    out, maps, twins = lockstep(ctx_auto, streams, oracle=ORACLE["refresh"], digests="refresh")
    reps = out[0][0]
    for j, n in ((3, 255), (4, 256), (5, 257)):
        assert 0 < reps[j].n[abi.PILLAR] < n and 0 < reps[j].n[abi.BEAM] < n
    assert reps[6].n[abi.PILLAR] == 257
    close(maps, twins)


# ---------------------------------------------------------------------------------------------------------------------------- capacity edges
def segment_edges():
    """class clouds of 4095, 8193, 4096 and 4097 records (one segment less a record, two and a record, one exactly, one and a record), half of each beyond
    the filter radius; the thinning then takes the ground down across its segment edge"""
    rng = np.random.default_rng(9990)

    def cloud(n, s):
        xyz = rng.uniform(-20.0, 20.0, (n, 3))
        xyz[::2, 0] += 100.0
        return E.records(xyz, s)

    m = [cloud(n, 9991 + c) for c, n in enumerate((4095, 8193, 4096, 4097, 1, 0))]
    f = [cloud(n, 9981 + c) for c, n in enumerate((255, 256, 257, 0, 1, 3))]
    P = abi.map_params(max_num_pts=6000, kept_vertex_num=2, local_map_radius=50.0, rng_seed=9)
    return Stream(m, E.S_POSES[0], [(f, E.S_POSES[1], P)])


def capacity_streams():
    n0 = E.scene_n(0)
    none = [E.empty() for _ in range(6)]
    return [
        of_case(E.scene_s_removal()),  # class clouds of 4095, 4096, 4097 and 8192 records, a frame pillar cloud of 8193, a facade of 4097
        of_case(E.scene_n(0)),  # trees of 1, 1023, 1024; frames of 11, 257, 1001
        of_case(E.scene_n(1)),  # trees of 1025, 2047, 2048; frames of 255, 256, 10
        of_case(E.scene_n(2)),  # trees of 2049, 4096, 4097
        of_case(E.scene_n(3)),  # trees of 6145, 4097, 2049
        of_case(E.scene_b("empty")),  # a map and a frame whose six clouds are empty
        Stream(none, np.eye(4), [(n0.frames[0][0], np.eye(4), n0.params[0])]),  # an empty map, a full frame
        Stream(n0.map_clouds, n0.map_pose, [(none, E.S_POSES[1], n0.params[0])]),  # a full map, an empty frame
        of_case(E.scene_b("nonfinite")),
        of_case(E.scene_s_pca()),  # the refresh's compaction across a segment edge
        segment_edges(),
    ]


def test_capacity_edges_side_by_side(ctx_auto):
    streams = capacity_streams()
    assert sorted(len(c) for c in streams[0].clouds)[:4] == [4095, 4096, 4097, 8192] and len(streams[0].steps[0][0][abi.PILLAR]) == 8193
    assert [len(c) for c in streams[10].clouds] == [4095, 8193, 4096, 4097, 1, 0]
    out, maps, twins = lockstep(ctx_auto, streams, oracle=ORACLE["capacity"], digests="capacity")
    big = np.finfo(np.float64).max
    assert list(out[0][0][5].local_bound) == [big] * 3 + [-big] * 3
    close(maps, twins)


# ------------------------------------------------------------------------------------------------------------------------------ independence
def seven_streams():
    removal = dict(map_based_dynamic_removal_on=1, dynamic_removal_center_radius=25.0, dynamic_dist_thre_min=0.25, dynamic_dist_thre_max=1.0, near_dist_thre=0.05,
                   tree_mode=2, tree_used="111110", tree_box=[-28.0, -14.0, -3.0, 30.0, 14.0, 8.0])
    return [
        of_case(E.scene_n(6)),
        of_frames(small_frames(200, n_frames=2), lambda k: abi.map_params(max_num_pts=900, kept_vertex_num=50, rng_seed=3)),
        of_case(E.scene_p(255, "random")),
        of_frames(small_frames(50, n_frames=2), lambda k: abi.map_params(max_num_pts=1500, kept_vertex_num=100, rng_seed=11, recalculate_feature_on=1, **removal)),
        of_case(E.scene_b("empty")),
        of_case(E.scene_n(9)),
        of_frames(linear_frames(340, n_frames=2), lambda k: abi.map_params(recalculate_feature_on=1, max_num_pts=10**7, kept_vertex_num=10**6, local_map_radius=60.0)),
    ]


def test_an_item_is_independent_of_its_batch(ctx_auto):
    S = seven_streams()
    X = 3
    alone, m1, t1 = lockstep(ctx_auto, [S[X]], oracle=(0,), digests=["seven/%d" % X])
    want, want_rep = state(m1[0]), bytes(alone[0][0][0])[:REPORT_BYTES]
    assert alone[0][0][0].dynamic_removal_ran == 1 and alone[0][1].n_groups == 1
    cut, m2, t2 = lockstep(ctx_auto, S, oracle=ORACLE["seven"], max_lockstep=3, digests="seven")
    assert cut[0][1].n_groups == 3  # cuts after 3 and 6
    assert state(m2[X]) == want and bytes(cut[0][0][X])[:REPORT_BYTES] == want_rep
    order = [5, 2, 6, 0, 4, 1, 3]
    mixed, m3, t3 = lockstep(ctx_auto, [S[i] for i in order], oracle=(), max_lockstep=0, digests=["seven/%d" % i for i in order])
    assert mixed[0][1].n_groups == 1
    for pos, i in enumerate(order):
        assert state(m3[pos]) == state(m2[i]) and bytes(mixed[0][0][pos])[:REPORT_BYTES] == bytes(cut[0][0][i])[:REPORT_BYTES]
    close(m1, t1, m2, t2, m3, t3)


# ----------------------------------------------------------------------------------------------------------------------------- lock step shown
def test_launches_and_waits_do_not_depend_on_the_group_size(ctx_auto):
    def one(seed):
        return of_frames(small_frames(seed, n_frames=2), lambda k: abi.map_params(max_num_pts=1500, kept_vertex_num=100, rng_seed=11, recalculate_feature_on=1,
                                                                                 map_based_dynamic_removal_on=1, tree_mode=1, tree_used="111110"))

    single, m1, t1 = lockstep(ctx_auto, [one(50)], oracle=(0,))
    s1 = single[0][1]
    assert single[0][0][0].dynamic_removal_ran == 1 and s1.n_syncs == 3 and s1.n_kernel_launches > 0 and s1.n_groups == 1
    six, m6, t6 = lockstep(ctx_auto, [one(50) for _ in range(6)], oracle=())
    s6 = six[0][1]
    assert (s6.n_groups, s6.n_lockstep, s6.n_syncs, s6.n_kernel_launches) == (1, 6, s1.n_syncs, s1.n_kernel_launches)
    pairs, m2, t2 = lockstep(ctx_auto, [one(50) for _ in range(6)], oracle=(), max_lockstep=2)
    s2 = pairs[0][1]
    assert (s2.n_groups, s2.n_lockstep, s2.n_syncs, s2.n_kernel_launches) == (3, 6, 3 * s1.n_syncs, 3 * s1.n_kernel_launches)
    close(m1, t1, m6, t6, m2, t2)


# --------------------------------------------------------------------------------------------------------------------------------- refusals
def raw_call(ctx, items, n, shared, results, stats=None, max_lockstep=0):
    return ctx.lib.mulls_map_update_batch(ctx.h, items, n, None if shared is None else C.byref(shared), max_lockstep, results, None if stats is None else C.byref(stats))


def test_refusals(ctx_auto):
    ctx = ctx_auto
    from mulls_amd import lib as mlib

    other = mlib.Context(0)
    frames = [small_frames(60 + 10 * i, n_frames=3) for i in range(3)]
    maps = [ctx.local_map(f[0][0], f[0][1]) for f in frames]
    twins = [ctx.local_map(f[0][0], f[0][1]) for f in frames]
    foreign = other.local_map(frames[0][0][0], frames[0][0][1])
    P = abi.map_params(max_num_pts=1800, kept_vertex_num=130, rng_seed=4)
    held = [mlib.LocalMap._clouds(f[1][0]) for f in frames]

    def items_of(which=(0, 1, 2), params=True):
        arr = (abi.MapUpdateItem * 3)()
        for j, i in enumerate(which):
            arr[j].map, arr[j].frame_down, arr[j].frame_pose_lo = maps[i].h, held[i][0], abi.colmajor16(frames[i][1][1])
            if params:
                arr[j].params = C.pointer(P)
        return arr

    before = [state(m) for m in maps]
    results = (abi.MapBatchResult * 3)()
    fill = lambda: C.memset(results, 0x5A, C.sizeof(results))
    untouched = lambda: bytes(results) == b"\x5a" * C.sizeof(results) and [state(m) for m in maps] == before
    bad = abi.MULLS_E_INVALID
    fill()
    assert raw_call(ctx, None, 3, P, results) == bad and untouched()
    assert raw_call(ctx, items_of(), 3, P, None) == bad and untouched()
    arr = items_of()
    arr[1].map = None
    assert raw_call(ctx, arr, 3, P, results) == bad and untouched()
    assert raw_call(ctx, items_of((0, 1, 0)), 3, P, results) == bad and untouched()  # a repeated map
    arr = items_of()
    arr[2].map = foreign.h
    assert raw_call(ctx, arr, 3, P, results) == bad and untouched()  # a map of another context
    arr = items_of()
    lent = (abi.Cloud * 6)(*[maps[1].cloud(c) for c in range(6)])  # item 0's frame lies in item 1's map
    arr[0].frame_down = lent
    assert raw_call(ctx, arr, 3, P, results) == bad and untouched()
    assert raw_call(ctx, items_of(params=False), 3, None, results) == bad and untouched()
    stats = abi.MapBatchStats()
    assert raw_call(ctx, None, 0, None, None, stats) == abi.MULLS_OK and stats.n_groups == 0 and untouched()  # n_items == 0
    # per-item refusals: the item's status is its single call's, its map is untouched, the others are their single calls
    short = abi.map_params(used_feature_type="111")
    nowhere = abi.Cloud()
    nowhere.pts, nowhere.n, nowhere.stride = None, 4, 48
    thin = abi.Cloud()
    thin.pts, thin.n, thin.stride = held[0][1][0].ctypes.data, 4, 47
    for spoil in ("null_frame", "short_used", "no_pointer", "stride"):
        arr = items_of()
        if spoil == "null_frame":
            arr[1].frame_down = None
        elif spoil == "short_used":
            arr[1].params = C.pointer(short)
        else:
            arr[1].frame_down = (abi.Cloud * 6)(*([nowhere if spoil == "no_pointer" else thin] + [abi.as_cloud(None)] * 5))
        k = {"null_frame": 1, "short_used": 1, "no_pointer": 2, "stride": 2}[spoil]  # a fresh pair of frames for the good items every round
        kk = min(k, 2)
        for i in (0, 2):
            arr[i].frame_down, arr[i].frame_pose_lo = mlib.LocalMap._clouds(frames[i][kk][0])[0], abi.colmajor16(frames[i][kk][1])
        snap = state(maps[1])
        assert raw_call(ctx, arr, 3, None, results) == bad and b"item 1" in ctx.lib.mulls_last_error(ctx.h)
        assert [r.status for r in results] == [abi.MULLS_OK, bad, abi.MULLS_OK] and state(maps[1]) == snap
        for i in (0, 2):
            rt = twins[i].update(frames[i][kk][0], frames[i][kk][1], P)
            same_report(results[i].report, rt)
            assert state(maps[i]) == state(twins[i])
    # after all of it a good batch still matches
    reps, stats = ctx.map_update_batch(maps, [f[2][0] for f in frames], [f[2][1] for f in frames], P)
    for i in range(3):
        same_report(reps[i], twins[i].update(frames[i][2][0], frames[i][2][1], P)) if i != 1 else None
    rt = twins[1].update(frames[1][2][0], frames[1][2][1], P)
    same_report(reps[1], rt)
    assert [state(m) for m in maps] == [state(m) for m in twins]
    clouds, appended, ro = pyoracle.map_update(frames[1][0][0], frames[1][0][1], frames[1][2][0], frames[1][2][1], P)
    against_oracle(maps[1], reps[1], clouds, appended, ro, P, frames[1][2][1])
    close(maps, twins, [foreign])
    other.close()


# ---------------------------------------------------------------------------------------------------------------- device-resident frames
def test_frames_from_feature_blocks(ctx_auto):
    """the frames as device clouds of mulls_extract_features_batch's blocks == the same frames passed from the host"""
    ctx = ctx_auto
    scene = synth.Scene(7)
    scans = []
    for k in range(3):
        scan = synth.raycast(scene, synth.se3(0.4 * k, 0.05 * k, scene.sensor_height), 32, 900, seed=7 + k)
        scans.append(abi.make_points(scan["xyz"], np.zeros_like(scan["xyz"]), scan["intensity"], scan["t"]))
    X = abi.extract_params(ground=abi.ground_params(nonground_random_down_rate=1), classify=abi.classify_params(neighbor_k=20))
    blocks, results, _ = ctx.extract_features_batch(scans, X)
    dev_frames = [b.class_clouds(down=True) for b in blocks]
    host_frames = [[ctx_download(ctx, cl) for cl in f] for f in dev_frames]
    assert sum(len(c) for f in host_frames for c in f) > 0
    start = small_frames(70, n_frames=1)[0]
    maps = [ctx.local_map(start[0], start[1]) for _ in range(3)]
    twins = [ctx.local_map(start[0], start[1]) for _ in range(3)]
    poses = [synth.se3(0.4 * k, 0.05 * k, 0.0) for k in range(3)]
    P = [abi.map_params(max_num_pts=1500 + 500 * k, kept_vertex_num=100, rng_seed=k, recalculate_feature_on=k % 2) for k in range(3)]
    reps_d, _ = ctx.map_update_batch(maps, dev_frames, poses, P)
    reps_h, _ = ctx.map_update_batch(twins, host_frames, poses, P)
    for k in range(3):
        same_report(reps_d[k], reps_h[k])
        assert state(maps[k]) == state(twins[k])
    clouds, appended, ro = pyoracle.map_update(start[0], start[1], host_frames[1], poses[1], P[1])
    against_oracle(maps[1], reps_d[1], clouds, appended, ro, P[1], poses[1])
    close(maps, twins, blocks)


def ctx_download(ctx, cloud):
    """a device cloud's records on the host (through a scratch map: mulls_map_set takes device clouds, mulls_map_download returns them)"""
    m = ctx.local_map([cloud] + [E.empty()] * 5, np.eye(4))
    out = m.download(0)
    m.close()
    return out


# -------------------------------------------------------------------------------------------------------------------------- resident targets
def test_batched_maps_serve_as_resident_targets(ctx_auto):
    ctx = ctx_auto
    streams = [of_frames(small_frames(80 + 10 * i, n_frames=3), lambda k: abi.map_params(max_num_pts=10**7, kept_vertex_num=10**6)) for i in range(3)]
    out, maps, twins = lockstep(ctx, streams, oracle=(0,))
    src_pair, _ = synth.make_pair(83, n_beams=32, n_az=700, src_counts={abi.GROUND: 500, abi.PILLAR: 200, abi.FACADE: 600, abi.BEAM: 120, abi.ROOF: 60},
                                  vertex_count=150)
    src = [abi.as_points(src_pair.src[c]) for c in range(6)]

    def pairs_of(group):
        arr = (abi.Pair * len(group))()
        for i, m in enumerate(group):
            bound = abi.PairData([m.download(c) for c in range(6)], src).tgt_bound
            for c in range(6):
                arr[i].tgt[c], arr[i].src[c], arr[i].src_down[c] = m.cloud(c), abi.as_cloud(src[c]), abi.as_cloud(None)
            for k in range(6):
                arr[i].tgt_bound[k] = float(bound[k])
            for k, v in enumerate(np.eye(4).reshape(-1)):
                arr[i].init_guess[k] = float(v)
        return arr

    P = abi.kitti_params(dis_thre_unit=2.4)
    ra = ctx.icp_batch([None] * 3, P, marshalled=(pairs_of(maps), abi.make_result_array(3)))
    rb = ctx.icp_batch([None] * 3, P, marshalled=(pairs_of(twins), abi.make_result_array(3)))
    for a, b in zip(ra, rb):
        assert (a.code, a.iters, list(a.ncorr)) == (b.code, b.iters, list(b.ncorr)) and a.T[:] == b.T[:] and a.info[:] == b.info[:] and a.sigma == b.sigma
    assert sum(ra[0].ncorr) > 0
    close(maps, twins)


# ------------------------------------------------------------------------------------------------------------------------- random sequences
def random_stream(block):
    """tests/test_gpu_map.py::test_random_update_sequences_match_oracle's construction"""
    rng = np.random.default_rng(5200 + block)
    frames = small_frames(400 + block, n_frames=4)

    def mutate(clouds):
        out = []
        for c in clouds:
            roll = rng.random()
            if roll < 0.15:
                out.append(c[:0])
            elif roll < 0.3:
                out.append(c[: int(rng.integers(1, 12))])
            elif roll < 0.4:
                out.append(np.concatenate([c, c[: len(c) // 2]]))  # exact duplicates
            else:
                out.append(c)
        return out

    def params(k):
        used = "".join(rng.choice(["0", "1"], p=[0.25, 0.75]) for _ in range(6))
        box = sorted(rng.uniform(-40, 40, 2)) + sorted(rng.uniform(-20, 20, 2)) + sorted(rng.uniform(-4, 8, 2))
        return abi.map_params(used_feature_type=used, max_num_pts=int(rng.choice([300, 1500, 6000, 10**7])),
                              kept_vertex_num=int(rng.choice([0, 50, 10**6])), local_map_radius=float(rng.uniform(15, 80)),
                              map_based_dynamic_removal_on=int(rng.random() < 0.7), dynamic_removal_center_radius=float(rng.uniform(5, 40)),
                              dynamic_dist_thre_min=float(rng.uniform(0.1, 0.6)), dynamic_dist_thre_max=float(rng.uniform(0.2, 3.0)),
                              near_dist_thre=float(rng.uniform(0.0, 0.1)), rng_seed=int(rng.integers(0, 2**31)), tree_mode=int(rng.integers(0, 3)),
                              tree_used="".join(rng.choice(["0", "1"]) for _ in range(6)), tree_box=[box[0], box[2], box[4], box[1], box[3], box[5]])

    return of_frames([(mutate(fc), fp) for fc, fp in frames], params)


def random_streams():
    return [random_stream(b) for b in range(4)]


def test_random_sequences_in_lock_step(ctx_auto):
    out, maps, twins = lockstep(ctx_auto, random_streams(), oracle=ORACLE["random"], digests="random")
    assert len(out) == 3
    close(maps, twins)


# ------------------------------------------------------------------------------------------------------------------------- recorded digests
DIGEST_CASES = {"mixed": mixed_streams, "removal": removal_streams, "refresh": refresh_streams, "capacity": capacity_streams, "seven": seven_streams,
                "random": random_streams}


def record_digests(ctx):
    """what mulls_map_update (LocalMap.update) leaves behind, per stream and step of DIGEST_CASES.  The file in tests/golden/ was written by this function from
    the commit before mulls_map_update became a batch of one; it is not a fixture to refresh when a test fails.
        PYTHONPATH=. python tests/test_gpu_map_batch.py --record-digests [file]"""
    out = {}
    for name, make in DIGEST_CASES.items():
        for i, s in enumerate(make()):
            m = ctx.local_map(s.clouds, s.pose)
            out["%s/%d" % (name, i)] = [digest(m, m.update(fc, fp, P)) for fc, fp, P in s.steps]
            m.close()
    return out


if __name__ == "__main__" and "--record-digests" in sys.argv:
    from mulls_amd import lib

    context = lib.Context(0)
    target = sys.argv[sys.argv.index("--record-digests") + 1] if len(sys.argv) > sys.argv.index("--record-digests") + 1 else DIGEST_FILE
    with open(target, "w") as f:
        json.dump(record_digests(context), f, indent=0, sort_keys=True)
        f.write("\n")
    context.close()
