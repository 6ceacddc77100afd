"""CPU tests of mulls_ncc_correspond_batch's host side: the layouts of mulls_ncc_problem and mulls_ncc_result in include/mulls_hip.h (compiled as C) against
mulls_amd/abi.py and the exported symbol; the planner of mulls_amd/csrc/ncc_batch.h (through tests/ncc_batch_harness.cpp: the sub-batch cuts, the arena's
offsets, the column chunks and the prefix tables); the bridge lo::hip::find_feature_correspondence_ncc_batch against the reference's types; and
k_ncc_batch.hip cross-compiled for gfx950 with the library's flags, every kernel without scratch memory.  The device is tested in
tests/test_gpu_ncc_batch.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mulls_amd import abi, build, lib
from test_ncc import BRIDGE_TU, REF_UTILITY, ROOT


def test_struct_layouts_and_export():
    """fails without the feature: the two structs as the header lays them out, the default limit, the symbol in the built library"""
    structs = {"mulls_ncc_problem": abi.NccProblem, "mulls_ncc_result": abi.NccResult}
    assert [f[0] for f in abi.NccProblem._fields_] == ["tgt", "src", "tgt_idx", "src_idx", "cap", "reserved"]
    assert [f[0] for f in abi.NccResult._fields_] == ["ret", "n_corr"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){"]
    for name, cls in structs.items():
        prog.append('printf("%s.size %%zu\\n", sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    prog.append('printf("limit %llu\\n", (unsigned long long)MULLS_NCC_BATCH_DEFAULT_SCRATCH_BYTES);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # the header is still plain C
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got["mulls_ncc_problem.size"]) == C.sizeof(abi.NccProblem) == 56 and int(got["mulls_ncc_result.size"]) == C.sizeof(abi.NccResult) == 8
    for name, cls in structs.items():
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (name, f)]) == getattr(cls, f).offset, (name, f)
    assert int(got["limit"]) == abi.NCC_BATCH_DEFAULT_SCRATCH_BYTES
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mulls_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mulls_ncc_correspond_batch\s*\(\s*mulls_ctx\s*\*", text)
    build.build()
    assert "mulls_ncc_correspond_batch" in lib.EXPORTS
    fn = lib.load().mulls_ncc_correspond_batch
    assert fn(None, None, 0, None, 0, None) == abi.MULLS_E_INVALID  # no context


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ncc_batch_harness") / "ncc_batch_harness.so")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which(build.hipcc()) or build.hipcc())))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "ncc_batch_harness.cpp"), "-o", so])
    P = C.CDLL(so)
    P.nb_problem_bytes.restype = C.c_uint64
    P.nb_problem_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]
    P.nb_cuts.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]
    P.nb_layout.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.c_int,
                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return P


def cuts(P, need, limit, wgs=None):
    n = len(need)
    a, w, out = (C.c_uint64 * max(n, 1))(*need), (C.c_uint64 * max(n, 1))(*(wgs or [1] * n)), (C.c_uint32 * (n + 2))()
    k = P.nb_cuts(a, w, n, limit, out)
    return list(out[:k])


def test_cuts(planner):
    assert cuts(planner, [], 1 << 30) == [0]  # the empty batch: no sub-batch
    shapes = [(10, 10), (2840, 2767), (4097, 513), (63, 65), (16384, 12288)]
    for fixed, K in ((0, 0), (1, 300), (1, 65536)):
        need = [planner.nb_problem_bytes(nt, ns, fixed, min(K, nt * ns)) for nt, ns in shapes]
        # what a problem holds: 20 bytes per staged key point, 48 + 8 per key point of descriptors and keys, the output, the selection state
        nt, ns = shapes[1]
        floor = 76 * (nt + ns) + ((K + 1) * 8 + 6 * 2048 * 4 if fixed else (2 + 2 * nt) * 4)
        assert floor <= need[1] <= floor + 12 * 256 + 512
        assert cuts(planner, need, 1) == list(range(len(shapes) + 1))  # a limit of 1 byte: every problem is larger and runs alone
        assert cuts(planner, need, sum(need)) == [0, len(shapes)]
        assert cuts(planner, need, sum(need) - 1) == [0, len(shapes) - 1, len(shapes)]
        c = cuts(planner, need, need[1] + need[2])
        assert c[0] == 0 and c[-1] == len(shapes) and all(a < b for a, b in zip(c, c[1:]))
        for a, b in zip(c, c[1:]):
            assert sum(need[a:b]) <= need[1] + need[2] or b == a + 1  # fits, or alone
            assert b == len(shapes) or sum(need[a:b + 1]) > need[1] + need[2]  # and takes what fits
    assert cuts(planner, [256] * (16384 + 5), 1 << 40) == [0, 16384, 16384 + 5]  # MULLS_NCC_BATCH_MAX_PROBLEMS
    assert cuts(planner, [256] * 4, 1 << 40, [1 << 29] * 4) == [0, 2, 4]  # a launch's grid stays at or below 2^30 workgroups


def layout(P, shapes, fixed, K=300, keys=None):
    """-> (records as dicts, info)"""
    n = len(shapes)
    nt, ns = (C.c_uint32 * n)(*[s[0] for s in shapes]), (C.c_uint32 * n)(*[s[1] for s in shapes])
    k = (C.c_uint32 * n)(*[min(K, s[0] * s[1]) if fixed else 0 for s in shapes])
    keys = keys or [(0x1000 * (2 * b + 1), 0x1000 * (2 * b + 2)) for b in range(n)]
    kt, ks = (C.c_uint64 * n)(*[a for a, _ in keys]), (C.c_uint64 * n)(*[b for _, b in keys])
    rec, info = (C.c_uint64 * (20 * n))(), (C.c_uint64 * 16)()
    assert P.nb_layout(nt, ns, k, kt, ks, n, fixed, rec, info) == 0
    names = ("in_t", "in_s", "desc_t", "desc_s", "rowkey", "colkey", "mm", "out", "sel", "hist", "n_t", "n_s", "K", "ext_t", "ext_s", "chunk", "chunk_swap", "wg",
             "wg_swap", "blk")
    inames = ("o_desc", "o_wg", "o_wg_swap", "o_blk", "o_in", "up_bytes", "o_sel", "sel_bytes", "o_out", "out_bytes", "dev_bytes", "grid", "grid_swap", "grid_blk",
              "n_staged", "record_bytes")
    return [dict(zip(names, rec[20 * b:20 * b + 20])) for b in range(n)], dict(zip(inames, info))


def test_layout_offsets_chunks_and_prefix_tables(planner):
    shapes = [(10, 10), (11, 64), (257, 33), (1000, 3000), (4097, 513), (2840, 2767)]
    for fixed in (0, 1):
        recs, info = layout(planner, shapes, fixed)
        assert info["record_bytes"] % 8 == 0 and info["o_desc"] == 0 and info["n_staged"] == 2 * len(shapes)
        # no two arrays overlap, everything lies inside the arena on a 256-byte boundary, the head and the staged clouds come first, the outputs last
        spans = []
        for r, (nt, ns) in zip(recs, shapes):
            out = (1 + r["K"]) * 8 if fixed else (2 + 2 * nt) * 4
            spans += [(r["in_t"], nt * 20), (r["in_s"], ns * 20), (r["desc_t"], nt * 48), (r["desc_s"], ns * 48), (r["rowkey"], nt * 8), (r["colkey"], ns * 8),
                      (r["mm"], 8), (r["out"], out)]
            if fixed:
                spans += [(r["sel"], 32), (r["hist"], 6 * 2048 * 4)]
                assert info["o_sel"] <= r["sel"] < r["hist"] and r["hist"] + 6 * 2048 * 4 <= info["o_sel"] + info["sel_bytes"]
            assert info["o_in"] <= r["in_t"] < info["up_bytes"] and info["o_in"] <= r["in_s"] < info["up_bytes"]
            assert info["o_out"] <= r["out"] and r["out"] + out <= info["o_out"] + info["out_bytes"] == info["dev_bytes"]
            assert (r["n_t"], r["n_s"], r["ext_t"], r["ext_s"]) == (nt, ns, 0, 0)
        spans.sort()
        assert spans[0][0] >= info["o_blk"] + 4 * (len(shapes) + 1) and all(a % 256 == 0 for a, _ in spans)
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= info["dev_bytes"]
        # the prefix tables: a problem's workgroups are its row blocks times its column chunks, in both passes; the chunks cover the columns
        wg = wg_swap = blk = 0
        for r, (nt, ns) in zip(recs, shapes):
            assert (r["wg"], r["wg_swap"], r["blk"]) == (wg, wg_swap, blk)
            assert r["chunk"] >= 32 and r["chunk_swap"] >= 32
            wg += -(-nt // 256) * -(-ns // r["chunk"])
            wg_swap += -(-ns // 256) * -(-nt // r["chunk_swap"])
            blk += -(-(nt + ns) // 256)
        assert (info["grid"], info["grid_swap"], info["grid_blk"]) == (wg, wg_swap, blk)
        assert 1024 <= info["grid"] <= 2048 + sum(-(-nt // 256) for nt, _ in shapes)  # about the 2048 workgroups the single call aims at
    # a batch of one has the single call's split: 2048 // row blocks splits of the columns
    for nt, ns in ((2840, 2767), (16384, 12288), (10, 100000), (100000, 10)):
        recs, info = layout(planner, [(nt, ns)], 0)
        rb = -(-nt // 256)
        assert recs[0]["chunk"] == max(32, -(-ns // max(1, 2048 // rb)))
    # 64 equal problems share the workgroups equally
    recs, info = layout(planner, [(2840, 2767)] * 64, 1, 4000)
    assert len({r["chunk"] for r in recs}) == 1 and 1024 <= info["grid"] <= 2048 + 64 * 12
    # a cloud that several problems name is staged once: one source under eight targets, and a device-resident side (key 0) is not staged at all
    keys = [(0x1000 * (b + 1), 0x900000) for b in range(8)]
    recs, info = layout(planner, [(300 + b, 700) for b in range(8)], 0, keys=keys)
    assert info["n_staged"] == 9 and len({r["in_s"] for r in recs}) == 1 and len({r["in_t"] for r in recs}) == 8
    recs, info = layout(planner, [(300, 700), (300, 700)], 0, keys=[(0, 0x2000), (0x1000, 0)])
    assert info["n_staged"] == 2 and (recs[0]["ext_t"], recs[0]["ext_s"], recs[1]["ext_t"], recs[1]["ext_s"]) == (1, 0, 0, 1)


BATCH_TU = BRIDGE_TU.split("// the call of test/mulls_reg.cpp:173-174")[0] + r"""
// the candidates of test/mulls_slam.cpp:517-557, matched together, and the defaults of cregistration.hpp:411
bool call(std::vector<pcTPtr> &target_kpts, std::vector<pcTPtr> &source_kpts, bool fixed_num_corr_on, int feature_correspondence_num, bool reciprocal_corr_on)
{
	std::vector<pcTPtr> target_cors, source_cors;
	for (size_t k = 0; k < target_kpts.size(); k++)
		target_cors.push_back(pcTPtr(new pcT())), source_cors.push_back(pcTPtr(new pcT()));
	std::vector<bool> ok, ok_default;
	lo::hip::find_feature_correspondence_ncc_batch<Point_T>(target_kpts, source_kpts, target_cors, source_cors, ok, fixed_num_corr_on, feature_correspondence_num,
															reciprocal_corr_on);
	lo::hip::find_feature_correspondence_ncc_batch<Point_T>(target_kpts, source_kpts, target_cors, source_cors, ok_default);
	return ok.size() == ok_default.size() && target_cors[0]->points.size() == source_cors[0]->points.size();
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_batch_bridge_compiles_against_the_reference_types():
    """lo::hip::find_feature_correspondence_ncc_batch on vectors of the reference's cloud pointers, as tests/test_ncc.py checks the single bridge"""
    assert "find_feature_correspondence_ncc_batch" not in BRIDGE_TU and "cregistration_hip.hpp" in BATCH_TU
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


def test_batch_kernels_cross_compile_without_scratch():
    """k_ncc_batch.hip for gfx950 with the library's flags: every kernel of the sub-batch launches is there and none spills to scratch memory"""
    assert "k_ncc_batch.hip" in build.SOURCES and "ncc_batch.h" in build.DEPS and "ncc_device.h" in build.DEPS
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "k_ncc_batch.s")
        subprocess.check_call([build.hipcc()] + build.FLAGS + ["--cuda-device-only", "-S", os.path.join(build.CSRC, "k_ncc_batch.hip"), "-o", asm],
                              stderr=subprocess.DEVNULL)
        text = open(asm).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", text, flags=re.M)]
    sizes = [int(v) for v in re.findall(r";\s*ScratchSize:\s*(\d+)", text)]
    for stem in ("k_nb_minmax", "k_nb_desc", "k_nb_rowmin", "k_nb_recip", "k_nb_hist", "k_nb_pick", "k_nb_collect"):
        assert any(stem in k for k in kernels), stem
    assert len(kernels) == 13 == len(scratch) and len(sizes) >= 13  # minmax, desc, rowmin x 2, recip, hist x 6, pick, collect
    assert not any(scratch) and not any(sizes), (scratch, sizes)
