"""CPU tests of mulls_non_max_suppress_batch's host side: the layout of mulls_nms_problem in include/mulls_hip.h (compiled as C) against mulls_amd/abi.py
and the exported symbol; the planner of mulls_amd/csrc/nms_batch.h (through tests/nms_batch_harness.cpp: the sub-batch cuts and the arena's offsets); the
bridge lo::hip::non_max_suppress_batch against the reference's types.  The device is tested in tests/test_gpu_nms_batch.py."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from mulls_amd import abi, build, lib
from test_nms import NMS_TU, REF_UTILITY, ROOT

LIMIT = abi.NMS_LDS_MAX_POINTS


def test_symbol_header_and_layout():
    """fails without the feature: the struct as the header lays it out, the default limit, the declaration, the symbol in the built library"""
    names = [f[0] for f in abi.NmsProblem._fields_]
    assert names == ["cloud", "out", "kept_idx", "order", "cap", "idx_cap"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){", 'printf("size %zu\\n", sizeof(mulls_nms_problem));']
    for f in names:
        prog.append('printf("%s %%zu\\n", offsetof(mulls_nms_problem, %s));' % (f, f))
    prog.append('printf("limit %llu\\n", (unsigned long long)MULLS_NMS_BATCH_DEFAULT_SCRATCH_BYTES);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # the header is still plain C
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got["size"]) == C.sizeof(abi.NmsProblem) == 48
    for f in names:
        assert int(got[f]) == getattr(abi.NmsProblem, f).offset, f
    assert int(got["limit"]) == abi.NMS_BATCH_DEFAULT_SCRATCH_BYTES == 512 << 20
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mulls_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mulls_non_max_suppress_batch\s*\(\s*mulls_ctx\s*\*", text)
    build.build()
    assert "mulls_non_max_suppress_batch" in lib.EXPORTS and "mulls_nms_batch_arena_bytes" in lib.EXPORTS
    L = lib.load()
    assert L.mulls_non_max_suppress_batch(None, None, 0, None, 0, None) == abi.MULLS_E_INVALID  # no context
    assert L.mulls_nms_batch_arena_bytes(None) == 0
    assert "nms_batch.h" in build.DEPS


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("nms_batch_harness") / "nms_batch_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "nms_batch_harness.cpp"), "-o", so])
    P = C.CDLL(so)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    for name, args in (("nmb_cloud_bytes", [C.c_uint32, C.c_int, C.c_int]), ("nmb_problem_bytes", [C.c_uint32, C.c_uint32, C.c_int]), ("nmb_fixed_bytes", []),
                       ("nmb_limit", [C.c_uint64])):
        getattr(P, name).restype, getattr(P, name).argtypes = C.c_uint64, args
    P.nmb_cuts.argtypes = [u64p, u32p, u32p, u32p, C.c_uint32, C.c_int, C.c_uint64, u32p, u64p]
    P.nmb_layout.argtypes = [u64p, u32p, u32p, u32p, C.c_uint32, C.c_int, u64p, u64p]
    return P


def arrays(problems):
    """problems: (cloud address, n, cap, device-resident) each"""
    k = max(len(problems), 1)
    return ((C.c_uint64 * k)(*[p[0] for p in problems]), (C.c_uint32 * k)(*[p[1] for p in problems]), (C.c_uint32 * k)(*[p[2] for p in problems]),
            (C.c_uint32 * k)(*[p[3] for p in problems]))


def cuts(P, problems, limit, path=0):
    n = len(problems)
    out, held = (C.c_uint32 * (n + 2))(), (C.c_uint64 * (n + 1))()
    k = P.nmb_cuts(*arrays(problems), n, path, limit, out, held)
    return list(out[:k]), list(held[:max(k - 1, 0)])


def layout(P, problems, path=0):
    n = len(problems)
    rec, info = (C.c_uint64 * (8 * max(n, 1)))(), (C.c_uint64 * 14)()
    assert P.nmb_layout(*arrays(problems), n, path, rec, info) == 0
    names = ("stage", "lds", "recs", "hdr", "kept", "n", "H", "out_cap")
    inames = ("n_desc", "n_max", "n_staged", "n_src", "n_gather", "gather_blk", "grid_blk", "head_bytes", "up_bytes", "o_cursor",
              "down_bytes", "o_out", "out_records", "dev_bytes")
    return [dict(zip(names, rec[8 * b:8 * b + 8])) for b in range(n)], dict(zip(inames, info))


def up256(v):
    return (v + 255) & ~255


def need(P, p, alone=True):
    """the bytes the cut rule counts for a problem that brings its cloud along"""
    _, n, cap, dev = p
    lds = 10 <= n <= LIMIT
    return P.nmb_problem_bytes(n, cap, lds) + (P.nmb_cloud_bytes(n, dev, lds) if alone else 0)


def test_planner_bytes(planner):
    P = planner
    # below the gate and the empty cloud take no arena, whoever holds them
    for n in (0, 9):
        for dev in (0, 1):
            assert P.nmb_cloud_bytes(n, dev, 0) == 0 and P.nmb_problem_bytes(n, n, 0) == 0
    # per staged point: the 48-byte record (a device-resident cloud: also its key and its permutation entry); per problem: a header and its record in the
    # head (counted as 256), the kept positions, the kept records it may return
    n = 2840
    assert P.nmb_cloud_bytes(n, 0, 1) == up256(48 * n) and P.nmb_cloud_bytes(n, 1, 1) == up256(48 * n) + 2 * up256(4 * n) + 256
    assert P.nmb_problem_bytes(n, n, 1) == 256 + up256(4 * n) + 48 * n and P.nmb_problem_bytes(n, 100, 1) == 256 + up256(4 * n) + 48 * 100
    # the multi-launch path stages nothing here; a device-resident cloud still has its keys read by the key pass
    assert P.nmb_cloud_bytes(5000, 0, 0) == 0 and P.nmb_cloud_bytes(5000, 1, 0) == 256 + up256(4 * 5000) and P.nmb_problem_bytes(5000, 5000, 0) == 0
    assert P.nmb_limit(0) == abi.NMS_BATCH_DEFAULT_SCRATCH_BYTES and P.nmb_limit(12345) == 12345


def test_planner_cuts(planner):
    P = planner
    fixed = P.nmb_fixed_bytes()
    assert cuts(P, [], 1 << 30) == ([0], [])  # the empty batch: no sub-batch
    probs = [(0x1000 * (b + 1), n, n, 0) for b, n in enumerate((10, 2840, 4096, 63, 2767, 1025))]
    each = [need(P, p) for p in probs]
    assert cuts(P, probs, 1)[0] == list(range(len(probs) + 1))  # a limit of 1 byte: every problem is larger and runs alone
    assert cuts(P, probs, fixed + sum(each)) == ([0, len(probs)], [fixed + sum(each)])
    assert cuts(P, probs, fixed + sum(each) - 1)[0] == [0, len(probs) - 1, len(probs)]
    limit = fixed + each[1] + each[2]
    c, held = cuts(P, probs, limit)
    assert c[0] == 0 and c[-1] == len(probs) and all(a < b for a, b in zip(c, c[1:]))
    for (a, b), h in zip(zip(c, c[1:]), held):
        assert h == fixed + sum(each[a:b]) and (h <= limit or b == a + 1)  # consecutive, fits or alone
        assert b == len(probs) or fixed + sum(each[a:b + 1]) > limit  # and takes what fits
    # a problem larger than the limit runs alone, its neighbours are not pulled in
    c, _ = cuts(P, probs, fixed + each[0] + each[3] + each[5])
    assert [2, 3] in [[a, b] for a, b in zip(c, c[1:])] and [1, 2] in [[a, b] for a, b in zip(c, c[1:])]
    # limit 0: the default
    many = [(0x100000 + 0x40000 * b, 4096, 4096, 0) for b in range(2000)]
    assert cuts(P, many, 0)[0] == cuts(P, many, abi.NMS_BATCH_DEFAULT_SCRATCH_BYTES)[0]
    per = (abi.NMS_BATCH_DEFAULT_SCRATCH_BYTES - fixed) // need(P, many[0])
    assert cuts(P, many, 0)[0][:2] == [0, per] and 1000 < per < 2000
    # a host cloud that several problems of a sub-batch name counts once in it, and again in the next sub-batch
    shared = [(0x5000, 3000, 3000, 0)] * 4
    own, cloud = need(P, shared[0], alone=False), P.nmb_cloud_bytes(3000, 0, 1)
    assert cuts(P, shared, 1 << 30) == ([0, 4], [fixed + cloud + 4 * own])
    assert cuts(P, shared, fixed + cloud + 2 * own) == ([0, 2, 4], [fixed + cloud + 2 * own] * 2)
    # sizes 0 and 9 take no arena: any number of them rides along, even under a limit that nothing fits
    small = [(0x9000, 9, 9, 0), (0, 0, 0, 0)] * 50
    assert cuts(P, small, 1) == ([0, 100], [fixed])
    assert cuts(P, small + probs[:1] + small, fixed + each[0])[0] == [0, 201]
    # MULLS_NMS_BATCH_MAX_PROBLEMS: the suppression launch's grid
    assert cuts(P, [(0x1000, 10, 10, 0)] * (16384 + 5), 1 << 40)[0] == [0, 16384, 16384 + 5]
    # path 2: nothing of a host cloud is staged
    assert cuts(P, probs, 1, path=2) == ([0, len(probs)], [fixed])


def test_planner_layout(planner):
    P = planner
    probs = [(0x1000, 0, 0, 0), (0x2000, 9, 9, 0), (0x3000, 10, 10, 0), (0x4000, 2048, 2048, 0), (0x5000, 2049, 100, 0), (0x6000, 4096, 4096, 1),
             (0x7000, 4097, 4097, 0), (0x8000, 5000, 5000, 1), (0x5000, 2049, 2049, 0), (0x9000, 300, 0, 1), (0xa000, 5, 5, 1)]
    recs, info = layout(P, probs)
    lds = [b for b, p in enumerate(probs) if 10 <= p[1] <= LIMIT]
    assert [b for b, r in enumerate(recs) if r["lds"]] == lds and info["n_desc"] == len(lds)
    assert info["n_max"] == 4096  # the largest cloud sizes the suppression launch's LDS
    assert info["n_staged"] == 6 and recs[4]["stage"] == recs[8]["stage"] and recs[4]["recs"] == recs[8]["recs"]  # the shared cloud once
    assert [recs[b]["stage"] for b in (0, 1, 6, 10)] == [0xffffffff] * 4  # nothing staged: empty, below the gate, a host cloud on the multi-launch path
    assert info["n_src"] == 3 and info["n_gather"] == 2  # the device-resident clouds of 10 points or more; the 5000-point one has only its keys read
    assert info["gather_blk"] == 16 + 2 and info["grid_blk"] == 16 + 2 + 20
    spans = []
    for b in lds:
        r, (_, n, cap, dev) = recs[b], probs[b]
        assert (r["n"], r["out_cap"]) == (n, min(n, cap)) and r["H"] == max(64, 1 << (n - 1).bit_length())
        spans += [(r["hdr"], 16), (r["kept"], 4 * n)]
        if b != 8:
            spans.append((r["recs"], 48 * n))
        assert (r["recs"] < info["up_bytes"]) == (not dev)  # host clouds go up with the head, device-resident ones are gathered behind it
        assert info["o_cursor"] < r["hdr"] and r["kept"] + 4 * n <= info["o_cursor"] + info["down_bytes"] <= info["o_out"]
    spans.sort()
    assert spans[0][0] >= info["head_bytes"] and all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))
    assert all(a % 256 == 0 for a, n in spans if n != 16) and info["o_cursor"] % 256 == 0 and info["o_out"] % 256 == 0
    assert info["out_records"] == sum(min(probs[b][1], probs[b][2]) for b in lds) and info["o_out"] + up256(48 * info["out_records"]) == info["dev_bytes"]
    # what the cut rule counts bounds what the layout takes
    _, held = cuts(P, probs, 1 << 40)
    assert info["dev_bytes"] <= held[0] <= info["dev_bytes"] + 256 * (len(probs) + 3) + P.nmb_fixed_bytes()
    # path 2: no problem takes a workgroup; the device-resident clouds still have their keys read
    recs, info = layout(P, probs, path=2)
    assert info["n_desc"] == 0 and info["n_src"] == 3 and info["n_gather"] == 0 and info["out_records"] == 0


BATCH_TU = NMS_TU.split("// the calls of test/mulls_reg.cpp:147")[0] + r"""
// both key-point clouds of test/mulls_reg.cpp:147-148, or the vertex clouds of the submaps of an event (test/mulls_slam.cpp:462), in one call
bool call(std::vector<pcTPtr> &vertex_clouds, float keypoint_nms_radius)
{
	std::vector<bool> ok = lo::hip::non_max_suppress_batch<Point_T>(vertex_clouds, keypoint_nms_radius);
	std::vector<bool> refused = lo::hip::non_max_suppress_batch<Point_T>(vertex_clouds, keypoint_nms_radius, false, false);
	return ok.size() == vertex_clouds.size() && refused.size() == ok.size();
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_batch_bridge_compiles_against_the_reference_types():
    """lo::hip::non_max_suppress_batch on a vector of the reference's cloud pointers, as tests/test_nms.py checks the single bridge"""
    assert "non_max_suppress_batch" not in NMS_TU and "cregistration_hip.hpp" in BATCH_TU
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
