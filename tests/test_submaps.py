"""CPU tests of the submap archive's definition (include/mulls_hip.h, "the submap archive"): the numpy restatement tests/submaps_restated.py against literal
loops and hand-worked cases, the ctypes mirrors against the header, and the bridge's syntax against the reference's types.  The device is compared with the
restatement, exactly, in tests/test_gpu_submaps.py."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import submaps_restated as R
from mulls_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = R.DBL_MAX
INF, NAN = float("inf"), float("nan")


def literal_bbx(points):
    """CloudUtility::get_cloud_bbx (utility.hpp:817-847), line by line"""
    min_x = min_y = min_z = DBL_MAX
    max_x = max_y = max_z = -DBL_MAX
    for x, y, z in points:
        x, y, z = float(np.float32(x)), float(np.float32(y)), float(np.float32(z))
        if min_x > x:
            min_x = x
        if min_y > y:
            min_y = y
        if min_z > z:
            min_z = z
        if max_x < x:
            max_x = x
        if max_y < y:
            max_y = y
        if max_z < z:
            max_z = z
    return [min_x, min_y, min_z, max_x, max_y, max_z]


BBX_CLOUDS = {
    "empty": [],
    "one": [(1.5, -2.0, 3.25)],
    "plain": [(1, 2, 3), (-4, 5, -6), (0.5, -0.25, 7)],
    "nan_first": [(NAN, NAN, NAN), (1, 2, 3), (-1, -2, -3)],
    "nan_mixed": [(1, NAN, 3), (NAN, 2, NAN), (0, 0, 0)],
    "all_nan": [(NAN, NAN, NAN)] * 3,
    "pos_inf": [(INF, 1, 2), (3, INF, 4)],
    "neg_inf": [(-INF, 1, 2), (3, -INF, 4)],
    "only_inf": [(INF, -INF, INF), (INF, -INF, -INF)],
    "inf_and_nan": [(INF, NAN, -INF), (-INF, INF, NAN), (2, 2, 2)],
}


@pytest.mark.parametrize("name", sorted(BBX_CLOUDS))
def test_restated_bounds_are_the_literal_loop(name):
    pts = BBX_CLOUDS[name]
    got = R.cloud_bbx(np.array(pts, np.float32).reshape(-1, 3))
    want = literal_bbx(pts)
    assert got.tolist() == want, (name, got, want)


def test_restated_posed_bounds_are_the_literal_loop():
    """bound = get_cloud_bbx of the points moved by pose_lo: ((m00 x + m01 y) + m02 z) + m03 in double, stored as float; translations of 1e4 m"""
    rng = np.random.RandomState(5)
    xyz = (rng.standard_normal((40, 3)) * 30).astype(np.float32)
    xyz[3] = (NAN, 1, 2)
    xyz[7] = (INF, -INF, 0)
    a = 0.7
    pose = np.array([[math.cos(a), -math.sin(a), 0, 1e4], [math.sin(a), math.cos(a), 0, -1e4], [0, 0, 1, 12.5], [0, 0, 0, 1]])
    moved = []
    with np.errstate(all="ignore"):
        for x, y, z in xyz.astype(np.float64):
            moved.append(tuple(np.float32(((pose[r, 0] * x + pose[r, 1] * y) + pose[r, 2] * z) + pose[r, 3]) for r in range(3)))
    rec = np.zeros((len(xyz), 48), np.uint8)
    rec[:, :12] = xyz.view(np.uint8).reshape(-1, 12)
    local, posed = R.submap_bounds(rec, pose)
    assert local.tolist() == literal_bbx([tuple(p) for p in xyz])
    assert posed.tolist() == literal_bbx(moved)
    nan_pose = pose.copy()
    nan_pose[1, 1] = NAN
    nan_pose[0, 3] = NAN
    nan_pose[2, 0] = NAN
    assert R.submap_bounds(rec, nan_pose)[1].tolist() == [DBL_MAX] * 3 + [-DBL_MAX] * 3


def test_merge_order():
    clouds = [np.full((k + 1, 48), k, np.uint8) for k in range(6)]  # class k has k + 1 records of byte k
    merged = R.merge(clouds)
    assert merged[:, 0].tolist() == [0] + [2] * 3 + [1] * 2 + [3] * 4 + [4] * 5 + [5] * 6
    assert R.MERGE_ORDER == abi.SUBMAP_MERGE_ORDER


EMPTY = [DBL_MAX] * 3 + [-DBL_MAX] * 3


def box(x0, y0, x1, y1):
    return [x0, y0, -1.0, x1, y1, 1.0]


def test_calculate_iou_hand_worked():
    assert R.calculate_iou(box(0, 0, 2, 2), box(0, 0, 2, 2)) == 1.0
    assert R.calculate_iou(box(0, 0, 2, 2), box(1, 0, 3, 2)) == 2.0 / 6.0  # intersection 1 x 2, union 4 + 4 - 2
    assert R.calculate_iou(box(0, 0, 2, 2), box(0.5, 0.5, 1.5, 1.5)) == 0.25  # nested: 1 / (4 + 1 - 1)
    assert R.calculate_iou(box(0.5, 0.5, 1.5, 1.5), box(0, 0, 2, 2)) == 0.25
    assert R.calculate_iou(box(0, 0, 1, 1), box(2, 2, 3, 3)) == 0.0  # disjoint: w and h clamp to 0
    assert R.calculate_iou(box(0, 0, 1, 1), box(1, 0, 2, 1)) == 0.0  # touching
    assert R.calculate_iou(box(0, 0, 4, 1), box(3, -5, 5, 5)) == 1.0 / (4.0 + 20.0 - 1.0)
    # an empty box (nothing won: min = DBL_MAX, max = -DBL_MAX): its area is (-inf)(-inf) = +inf, the intersection clamps to 0 -> 0 / inf = 0
    assert R.calculate_iou(EMPTY, box(0, 0, 1, 1)) == 0.0
    assert R.calculate_iou(box(0, 0, 1, 1), EMPTY) == 0.0
    assert R.calculate_iou(EMPTY, EMPTY) == 0.0
    # two boxes of no area on one spot: 0 / 0
    assert math.isnan(R.calculate_iou(box(1, 1, 1, 1), box(1, 1, 1, 1)))
    # z plays no part
    assert R.calculate_iou([0, 0, 100, 2, 2, 200], [1, 0, -9, 3, 2, -8]) == 2.0 / 6.0


def test_adjacent_by_id():
    assert R.adjacent_by_id(10, 7, 3) and R.adjacent_by_id(7, 10, 3) and R.adjacent_by_id(5, 5, 0)
    assert not R.adjacent_by_id(10, 6, 3) and not R.adjacent_by_id(6, 10, 3)


def pose_at(x, y, z=0.0):
    P = np.eye(4)
    P[:3, 3] = (x, y, z)
    return P


def layout():
    """a loop: the query (id 7) returns near submaps 0, 1 and 2; 4 .. 6 are adjacent by id; 3 is out of reach.  Boxes are 20 x 20 around each centre."""
    centres = [(0, 0), (10, 0), (0, 15), (200, 0), (30, 30), (20, 20), (10, 10), (5, 0)]
    poses = [pose_at(x, y, 0.5 * k) for k, (x, y) in enumerate(centres)]
    bounds = [[x - 10, y - 10, -2, x + 10, y + 10, 2] for x, y in centres]
    return poses, bounds, list(range(8))


def test_find_overlap_hand_worked():
    poses, bounds, ids = layout()
    edges = R.find_overlap(poses, bounds, ids, 7)
    # neighbours within 50 m, by distance: 0 and 1 (25), 6 (125), 2 (250), 5 (625), 4 (1525); 4, 5 and 6 are adjacent by id (7 - 3 = 4)
    # IoU with 0: 15 x 20 / (800 - 300) = 0.6; with 1: the same; with 2: 15 x 5 / (800 - 75)
    assert [(e["tgt_id"], e["src_id"]) for e in edges] == [(0, 7), (1, 7)]
    assert [e["overlapping_ratio"] for e in edges] == [300.0 / 500.0, 300.0 / 500.0]
    assert np.array_equal(edges[0]["Trans1_2"], pose_at(5, 0, 3.5)) and np.array_equal(edges[1]["Trans1_2"], pose_at(-5, 0, 3.0))
    low = R.find_overlap(poses, bounds, ids, 7, min_iou_thre=0.1)
    assert [e["tgt_id"] for e in low] == [0, 1, 2] and low[2]["overlapping_ratio"] == 75.0 / 725.0
    assert [e["tgt_id"] for e in R.find_overlap(poses, bounds, ids, 7, min_iou_thre=0.1, max_neighbor=1)] == [0]  # the distance tie goes to the smaller id
    assert [e["tgt_id"] for e in R.find_overlap(poses, bounds, ids, 7, min_iou_thre=0.1, max_neighbor=0)] == [0, 1, 2]
    assert [e["tgt_id"] for e in R.find_overlap(poses, bounds, ids, 7, min_iou_thre=0.0, adjacent_id_thre=0)] == [0, 1, 6, 2]  # 6: 150 / 650; 5 and 4 share no area with the query
    # the radius is strict: submap 0 lies exactly 5 m from the query
    assert [e["tgt_id"] for e in R.find_overlap(poses, bounds, ids, 7, neighbor_search_dist=5.0)] == []
    assert [e["tgt_id"] for e in R.find_overlap(poses, bounds, ids, 7, neighbor_search_dist=5.000001)] == [0, 1]
    # too few submaps: blocks.size() < adjacent_id_thre + 2
    assert R.find_overlap(poses, bounds, ids, 3) == [] and R.find_overlap(poses, bounds, ids, 7, adjacent_id_thre=7) == []
    # 3-D: the query's z differs by 3.5 from submap 0's and by 3.0 from submap 1's, so 1 is now the nearer one; IoU ties keep the neighbour order
    assert [e["tgt_id"] for e in R.find_overlap(poses, bounds, ids, 7, search_2d=0)] == [1, 0]


def test_invert4_on_rigid_and_general_matrices():
    a = 0.3
    T = np.array([[math.cos(a), -math.sin(a), 0, 3], [math.sin(a), math.cos(a), 0, -4], [0, 0, 1, 5], [0, 0, 0, 1]])
    assert np.allclose(R.mul4(R.invert4(T), T), np.eye(4), atol=1e-14)
    G = np.random.RandomState(2).standard_normal((4, 4))
    assert np.allclose(R.invert4(G), np.linalg.inv(G), rtol=1e-10, atol=1e-12)
    assert np.array_equal(R.invert4(np.eye(4)), np.eye(4))


HARNESS = r"""
// stand-alone driver of the library's host arithmetic (mulls_amd/csrc/submaps_host.h): infos, a query id and parameters in, edges out
#include <cstdio>
#include "submaps_host.h"
int main(int argc, char **argv)
{
	if (argc != 3)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	uint32_t n = 0, cur = 0;
	mulls_overlap_params P;
	if (!f || fread(&n, 4, 1, f) != 1 || fread(&cur, 4, 1, f) != 1 || fread(&P, sizeof(P), 1, f) != 1)
		return 3;
	std::vector<mulls_submap_info> infos(n);
	if (n && fread(infos.data(), sizeof(mulls_submap_info), n, f) != n)
		return 4;
	fclose(f);
	const std::vector<mulls_submap_edge> e = mulls::submaps::find_overlap(infos.data(), cur, P);
	FILE *g = fopen(argv[2], "wb");
	if (!g)
		return 5;
	if (!e.empty())
		fwrite(e.data(), sizeof(mulls_submap_edge), e.size(), g);
	fclose(g);
	return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """the host overlap search as a program of its own, built with the address and undefined-behaviour sanitizers"""
    d = tmp_path_factory.mktemp("submaps_harness")
    src, exe = os.path.join(d, "h.cpp"), os.path.join(d, "h")
    open(src, "w").write(HARNESS)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "mulls_amd", "csrc"), src, "-o", exe])

    def run(poses, bounds, ids, cur, **kw):
        infos = (abi.SubmapInfo * len(poses))()
        for k in range(len(poses)):
            infos[k].id_in_strip = int(ids[k])
            infos[k].pose_lo = abi.colmajor16(poses[k])
            for j in range(6):
                infos[k].bound[j] = float(bounds[k][j])
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([len(poses), cur], np.uint32).tobytes() + bytes(abi.overlap_params(**kw)) + bytes(infos))
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
        assert len(raw) % C.sizeof(abi.SubmapEdge) == 0
        return (abi.SubmapEdge * (len(raw) // C.sizeof(abi.SubmapEdge))).from_buffer_copy(raw)

    return run


def random_layout(seed):
    rng = np.random.RandomState(seed)
    n = 24
    centres = rng.uniform(-60, 60, (n, 3))
    centres[n - 1] = 0.0
    centres[2], centres[3] = (40.0, 30.0, 0.0), (50.0, 0.0, 3.0)  # 2-D distance exactly 50
    centres[5] = centres[4]
    poses = []
    for k in range(n):
        a = rng.uniform(-3, 3)
        P = np.eye(4)
        P[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
        P[:3, 3] = centres[k]
        poses.append(P)
    poses[5] = poses[4].copy()
    half = rng.uniform(5, 50, (n, 2))
    bounds = [[c[0] - h[0], c[1] - h[1], -1, c[0] + h[0], c[1] + h[1], 1] for c, h in zip(centres, half)]
    bounds[5] = list(bounds[4])  # an IoU tie
    bounds[6] = EMPTY
    bounds[7] = [1, 1, 0, 1, 1, 0]
    ids = list(range(n))
    ids[9], ids[20] = 20, 9
    return poses, bounds, ids


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_overlap_search_equals_restatement(harness, seed):
    """the library's own host code (no device involved) against the restatement: every id, every ratio and every bit of Trans1_2"""
    poses, bounds, ids = random_layout(seed)
    seen = 0
    for kw in (dict(), dict(search_2d=0), dict(max_neighbor=0, min_iou_thre=0.0), dict(max_neighbor=1), dict(max_neighbor=100, adjacent_id_thre=0, min_iou_thre=0.01),
               dict(neighbor_search_dist=75.0, min_iou_thre=0.0, max_neighbor=20), dict(adjacent_id_thre=22), dict(adjacent_id_thre=23), dict(min_iou_thre=-1.0, max_neighbor=0)):
        for cur in (len(poses) - 1, 12, 3):
            want = R.find_overlap(poses, bounds, ids, cur, **kw)
            got = harness(poses, bounds, ids, cur, **kw)
            assert len(got) == len(want), (kw, cur)
            for g, w in zip(got, want):
                assert (g.tgt_id, g.src_id, g.overlapping_ratio) == (w["tgt_id"], w["src_id"], w["overlapping_ratio"]), (kw, cur)
                assert np.array(g.Trans1_2[:]).tobytes() == np.asarray(w["Trans1_2"], np.float64).T.tobytes(), (kw, cur)
            seen += len(want)
    assert seen > 30


def test_ctypes_layout_matches_header():
    structs = {"mulls_submap_info": abi.SubmapInfo, "mulls_overlap_params": abi.OverlapParams, "mulls_submap_edge": abi.SubmapEdge}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){"]
    for cname, ct in structs.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog.append('printf("CHUNK %u\\nMERGED %d\\nNO_GROUND %d\\n", MULLS_SUBMAP_CHUNK, MULLS_SUBMAP_MERGED, MULLS_SUBMAP_MERGED_NO_GROUND);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    for cname, ct in structs.items():
        assert int(got[cname]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(ct, f).offset, (cname, f)
    assert (int(got["CHUNK"]), int(got["MERGED"]), int(got["NO_GROUND"])) == (abi.SUBMAP_CHUNK, abi.SUBMAP_MERGED, abi.SUBMAP_MERGED_NO_GROUND)


def test_exports_and_defaults():
    header = open(os.path.join(ROOT, "include", "mulls_hip.h")).read()
    declared = set(re.findall(r"\b(mulls_submaps_\w+|mulls_overlap_default_params)\s*\(", header))
    assert declared and declared <= set(lib.EXPORTS)
    p, q = abi.overlap_params(), R.OVERLAP_DEFAULTS
    assert (p.neighbor_search_dist, p.min_iou_thre, p.adjacent_id_thre, p.search_2d, p.max_neighbor) == (
        q["neighbor_search_dist"], q["min_iou_thre"], q["adjacent_id_thre"], q["search_2d"], q["max_neighbor"]) == (50.0, 0.25, 3, 1, 10)


def test_library_defaults_match():
    p = abi.OverlapParams()
    lib.load().mulls_overlap_default_params(C.byref(p))
    assert bytes(p) == bytes(abi.overlap_params())


from test_ncc import REF_UTILITY  # noqa: E402  (where the reference tree is looked for)

BRIDGE_TU = r"""
#include <chrono>
#include <cstdio>
#include "ref_shim/shim.hpp"
#include "mulls_hip.h"
#define max_(a, b) (((a) > (b)) ? (a) : (b))
#define min_(a, b) (((a) < (b)) ? (a) : (b))
using namespace std;
typedef pcl::PointXYZINormal Point_T;
typedef pcl::PointCloud<Point_T>::Ptr pcTPtr;
typedef pcl::PointCloud<Point_T> pcT;
typedef pcl::search::KdTree<Point_T>::Ptr pcTreePtr;
typedef pcl::search::KdTree<Point_T> pcTree;
#include "util_typedefs.inc"
namespace lo
{
#include "util_types.inc"
} // namespace lo
#include "cregistration_hip.hpp"
// the calls of test/mulls_slam.cpp:454 / :462 (a new submap), :508 / :511 (candidate edges) and :616 (after a successful optimisation)
int call(mulls_ctx *ctx, mulls_submaps *store, lo::cloudblock_Ptr &submap, lo::cloudblock_Ptrs &cblock_submaps, lo::constraints &current_registration_edges)
{
	mulls_submap_info a = lo::hip::submaps_push(ctx, store, submap);
	mulls_submap_info b = lo::hip::submaps_push(ctx, store, submap, 0.25f);
	int n = lo::hip::find_overlap_registration_constraint(ctx, store, cblock_submaps, current_registration_edges, 1.5f * 50.0f, 0.0f, 3, true, 20);
	n += lo::hip::find_overlap_registration_constraint(ctx, store, cblock_submaps, current_registration_edges, 50.0f, 0.25f, 3, true);
	n += lo::hip::find_overlap_registration_constraint(ctx, store, cblock_submaps, current_registration_edges);
	bool ok = lo::hip::update_optimized_nodes(ctx, store, cblock_submaps, true, true) && lo::hip::update_optimized_nodes(ctx, store, cblock_submaps);
	return ok ? n + (int)a.submaps_needed + (int)b.submaps_needed : -1;
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_against_the_reference_types():
    """lo::hip::submaps_push, update_optimized_nodes and find_overlap_registration_constraint on the reference's cloudblock_Ptrs and constraints, as
    tests/test_pgo.py checks its bridge"""
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 592, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(BRIDGE_TU)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
