"""CPU tests of mulls_extract_features_batch's host side: the exported symbol, the layout of the two structs of include/mulls_hip.h against mulls_amd/abi.py, the
planner (mulls_amd/csrc/extract_batch.h through tests/extract_batch_harness.cpp: the sub-batch cuts, the arena's offsets, the per-scan bytes against the single
calls' formulas — in Python, and once more by the harness itself as a stand-alone program under the sanitizers) and the bridge lo::hip::extract_semantic_pts_batch
against the reference's types.  The device is tested in tests/test_gpu_extract_batch.py."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from mulls_amd import abi, build, lib
from test_ncc import REF_UTILITY
from test_teaser import BRIDGE_TU, ROOT

HARNESS = os.path.join(ROOT, "tests", "extract_batch_harness.cpp")


def rocm_include():
    """the runtime's host headers (types only: the harness links nothing), next to the compiler the build uses"""
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "include")


def test_symbol_is_exported():
    assert "mulls_extract_features_batch" in lib.EXPORTS
    fn = lib.load().mulls_extract_features_batch
    assert fn(None, None, 0, None, None, 0, None, None) == abi.MULLS_E_INVALID  # no context


def test_struct_layouts():
    """mulls_extract_batch_result and mulls_extract_batch_stats as the header lays them out; the header is still plain C"""
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){"]
    for name, cls in (("mulls_extract_batch_result", abi.ExtractBatchResult), ("mulls_extract_batch_stats", abi.ExtractBatchStats)):
        prog.append('printf("%s.size %%zu\\n", sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    prog.append('printf("limit %llu\\n", (unsigned long long)MULLS_EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES);')
    prog.append('printf("count %d\\n", (int)MULLS_EX_COUNT);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    for name, cls in (("mulls_extract_batch_result", abi.ExtractBatchResult), ("mulls_extract_batch_stats", abi.ExtractBatchStats)):
        assert int(got[name + ".size"]) == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (name, f)]) == getattr(cls, f).offset, (name, f)
    assert C.sizeof(abi.ExtractBatchResult) == 8 + 4 * abi.EX_COUNT == 64 and C.sizeof(abi.ExtractBatchStats) == 28
    assert int(got["limit"]) == abi.EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES and int(got["count"]) == abi.EX_COUNT


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("extract_batch_harness") / "extract_batch_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", rocm_include(), HARNESS, "-o", so])
    L = C.CDLL(so)
    for f in (L.eb_gf_total, L.eb_cl_total, L.eb_table_bytes, L.eb_head_bytes, L.eb_offsets):
        f.restype = C.c_uint64
    L.eb_gf_total.argtypes = [C.c_uint32, C.c_int, C.c_int]
    L.eb_cl_total.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.eb_work_points.restype = L.eb_cuts.restype = L.eb_max_scans.restype = C.c_uint32
    L.eb_work_points.argtypes = [C.c_uint32, C.c_int, C.c_int]
    L.eb_scan_cost.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    L.eb_cuts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    L.eb_offsets.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    return L


SIZES = [6375, 0, 22400, 19182, 1025, 0, 964, 3125, 200, 500, 121000, 1]  # zeros among them; 121 000: one scan larger than the smaller limits
SHAPES = {"D": dict(prefilter=0, method=0, fixed=0, ufn=20000), "K": dict(prefilter=1, method=3, fixed=1, ufn=3000)}


def up256(v):
    return (v + 255) // 256 * 256


def costs(L, sizes, shape, K=50):
    out = []
    for n in sizes:
        c = (C.c_uint64 * 3)()
        L.eb_scan_cost(n, shape["prefilter"], shape["method"], shape["fixed"], shape["ufn"], K, c)
        out.append([int(v) for v in c])
    return out


def cuts_of(L, need, limit):
    arr, out = (C.c_uint64 * max(len(need), 1))(*need), (C.c_uint32 * (len(need) + 2))()
    k = L.eb_cuts(arr, len(need), limit, out)
    return [int(v) for v in out[:k]]


def offsets_of(L, cost, first, last):
    flat = (C.c_uint64 * (3 * len(cost)))(*[v for c in cost for v in c])
    out = (C.c_uint64 * (2 * len(cost)))()
    arena = L.eb_offsets(flat, len(cost), first, last, out)
    return int(arena), [(int(out[2 * b]), int(out[2 * b + 1])) for b in range(len(cost))]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_scan_bytes_are_the_single_calls(planner, shape):
    """a scan's regions are what gf_layout and carve give for that scan alone (rounded up to 256 bytes), plus its table row"""
    S = SHAPES[shape]
    table = planner.eb_table_bytes()
    for n, (gf, cl, total) in zip(SIZES, costs(planner, SIZES, S)):
        if n == 0:
            assert (gf, cl, total) == (0, 0, table)
            continue
        work = planner.eb_work_points(n, S["fixed"], S["ufn"])
        assert work == (min(n, S["ufn"]) if S["fixed"] else n)
        assert gf == up256(planner.eb_gf_total(n, S["prefilter"], S["method"]))
        assert cl == up256(planner.eb_cl_total(work, 50, n))
        assert total == gf + cl + table
    # the KITTI shape of the header's default: 121 000 returns, the non-ground cloud thinned to 20 000 — 64 of them in one sub-batch
    kitti = costs(planner, [121000] * 64, dict(prefilter=1, method=3, fixed=1, ufn=20000))
    need = [c[2] for c in kitti]
    assert planner.eb_head_bytes() + sum(need) <= abi.EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES
    assert cuts_of(planner, need, abi.EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES) == [0, 64]
    assert 129 << 20 < need[0] < 130 << 20  # 129.6 MiB a scan


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cuts_and_offsets(planner, shape):
    cost = costs(planner, SIZES, SHAPES[shape])
    need = [c[2] for c in cost]
    head, table = planner.eb_head_bytes(), planner.eb_table_bytes()
    assert cuts_of(planner, [], 1 << 30) == [0]  # the empty batch: no sub-batch
    assert cuts_of(planner, need, 1) == list(range(len(SIZES) + 1))  # every scan larger than the limit: each runs alone
    after_each = cuts_of(planner, need, head + max(need))
    everything = head + sum(need)
    assert cuts_of(planner, need, everything) == [0, len(SIZES)] and cuts_of(planner, need, everything - 1)[-2] > 0
    limits = [1, need[0], head + need[0] + need[1] + need[2], everything // 3, head + max(need), everything - 1, everything, 1 << 62]
    for limit in limits:
        c = cuts_of(planner, need, limit)
        assert c[0] == 0 and c[-1] == len(SIZES) and all(a < b for a, b in zip(c, c[1:]))  # every scan in exactly one sub-batch, in order
        for a, b in zip(c, c[1:]):
            arena, off = offsets_of(planner, cost, a, b)
            assert arena == head + sum(need[a:b])
            assert arena <= limit or b == a + 1  # fits, or alone
            assert b == len(SIZES) or head + sum(need[a:b + 1]) > limit  # and takes what fits
            spans = [(0, head + table * (b - a))]
            for s in range(a, b):
                assert off[s][0] % 256 == 0 and off[s][1] % 256 == 0
                spans += [(off[s][0], cost[s][0]), (off[s][1], cost[s][1])]
            spans = sorted(sp for sp in spans if sp[1])
            for (p, lp), (q, _) in zip(spans, spans[1:]):
                assert p + lp <= q, (p, lp, q)  # no two regions overlap
            assert spans[-1][0] + spans[-1][1] <= arena
    assert len(after_each) >= 3
    cap = planner.eb_max_scans()
    assert cuts_of(planner, [table] * (cap + 5), 1 << 40) == [0, cap, cap + 5]  # the grid axis bounds a sub-batch too


def test_voxel_flag_of_the_scan_cost(planner):
    """a scan that is voxel-down-sampled ahead of the ground filter: never cheaper than without, and the ground arena gf_layout gives with the flag"""
    planner.eb_scan_cost_vox.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    planner.eb_gf_total_vox.restype, planner.eb_gf_total_vox.argtypes = C.c_uint64, [C.c_uint32, C.c_int, C.c_int, C.c_int]
    table = planner.eb_table_bytes()
    for n in SIZES:
        for prefilter in (0, 1):
            for method in (0, 1, 2, 3):
                a, b = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
                planner.eb_scan_cost_vox(n, prefilter, 1, method, 1, 3000, 50, a)
                planner.eb_scan_cost_vox(n, prefilter, 0, method, 1, 3000, 50, b)
                assert a[0] >= b[0] and a[1] == b[1] and a[2] == a[0] + a[1] + table
                assert a[0] == (up256(planner.eb_gf_total_vox(n, prefilter, 1, method)) if n else 0)
                assert n == 0 or a[0] > b[0]  # the keys and the order take room
                assert b[0] == (up256(planner.eb_gf_total(n, prefilter, method)) if n else 0)


def test_one_scan_cuts(planner):
    """the scan-local steps: `count` sub-batches of one scan each, whatever the limit"""
    planner.eb_cuts_max.restype, planner.eb_cuts_max.argtypes = C.c_uint32, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]
    need = [c[2] for c in costs(planner, SIZES, SHAPES["K"])]
    arr, out = (C.c_uint64 * len(need))(*need), (C.c_uint32 * (len(need) + 2))()
    for limit in (1, need[0], planner.eb_head_bytes() + sum(need), 1 << 62):
        assert planner.eb_cuts_max(arr, len(need), limit, 1, out) == len(need) + 1
        assert list(out[:len(need) + 1]) == list(range(len(need) + 1))
        k = planner.eb_cuts_max(arr, len(need), limit, planner.eb_max_scans(), out)
        assert list(out[:k]) == cuts_of(planner, need, limit)  # the default is the grid axis's bound
    assert planner.eb_cuts_max(arr, 0, 1, 1, out) == 1 and out[0] == 0


def test_block_layout(planner):
    """a feature block's buffer against the two hand-written forms the function replaces: offsets rounded to 256, the selection indices riding at the end"""
    planner.eb_ex_count.restype = C.c_uint32
    planner.eb_block_layout.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    count = planner.eb_ex_count()
    assert count == abi.EX_COUNT
    rec = abi.POINT_BYTES
    cases = [([0] * count, 0), ([16] * count, 0), ([0, 0, 16, 8, 0] + [0] * (count - 5), 8),  # 16 records are 768 bytes: a multiple of 256 already
             ([0, 0, 4097, 2049, 1900, 7, 300, 0, 41, 7, 200, 0, 17, 3][:count], 2049), ([0, 0, 121000, 60500, 20000] + [1] * (count - 5), 60500)]
    for cnt, n_idx in cases:
        out = (C.c_uint64 * (count + 2))()
        planner.eb_block_layout((C.c_uint32 * count)(*cnt), n_idx, out)
        need = 0
        for k in range(count):
            assert out[k] == need and out[k] % 256 == 0
            need += (cnt[k] * rec + 255) & ~255
        need += n_idx * 4 + 256
        assert out[count + 1] == need and out[count] == need - (n_idx * 4 + 128)
        assert out[count] >= out[count - 1] + cnt[count - 1] * rec and out[count] + n_idx * 4 <= need  # the indices lie behind the last cloud, inside the block


def test_planner_under_sanitizers(tmp_path):
    """the harness as a stand-alone program (its own main checks the same properties on the same inputs), built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "extract_batch_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DEB_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", rocm_include(), HARNESS, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"extract_batch_harness: OK" in out.stdout, out.stdout.decode()[-2000:]


BATCH_TU = BRIDGE_TU.split("// the call of test/mulls_reg.cpp:177")[0] + r"""
// the frames of a sequence through extract_semantic_pts' arguments as test/mulls_slam.cpp:365-380 passes them, together
bool call(std::vector<lo::cloudblock_Ptr> &blocks, int &gf_down_rate_ground, int &gf_downsample_rate_nonground)
{
	bool a = lo::hip::extract_semantic_pts_batch<Point_T>(blocks, 0.0f, 3.0f, 0.3f, 1.5f, 2.0f, gf_down_rate_ground, gf_downsample_rate_nonground, 1.0f, 50, 0.65f, 0.65f, 0.1f,
															0.75f, 0.75f);
	bool b = lo::hip::extract_semantic_pts_batch<Point_T>(blocks, 0.2f, 3.0f, 0.3f, 1.5f, 2.0f, gf_down_rate_ground, gf_downsample_rate_nonground, 1.0f, 50, 0.65f, 0.65f, 0.1f,
															0.75f, 0.75f, true, 2, 15.0f, 3, 2.0f, true, true, false, 2, 8, 0, 2, 8, 1, FLT_MAX, 0.94f, 0.17f, 0.98f, 0.34f, true, true,
															500, 200, 800, 200, 200, 20000, FLT_MAX, 0.0f, 2.0f, -7.0f, 0.3f, true);
	bool c = lo::hip::extract_semantic_pts<Point_T>(blocks[0], 0.0f, 3.0f, 0.3f, 1.5f, 2.0f, gf_down_rate_ground, gf_downsample_rate_nonground, 1.0f, 50, 0.65f, 0.65f, 0.1f, 0.75f,
													 0.75f);
	return a && b && c;
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t: what the bridge header expects to be visible) is not here")
def test_batch_bridge_compiles_against_the_reference_types():
    """lo::hip::extract_semantic_pts_batch on a vector of the reference's cloudblock_Ptr, and the single bridge it shares its pieces with"""
    assert "extract_semantic_pts_batch" not in BRIDGE_TU and "cregistration_hip.hpp" in BATCH_TU
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 590, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(BATCH_TU)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
