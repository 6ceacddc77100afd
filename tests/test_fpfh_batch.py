"""CPU tests of mulls_compute_fpfh_batch and mulls_coarse_reg_fpfhsac_batch: the fixture tests/golden/fpfh_batch_cases.npz against the numpy restatement
(tests/fpfh_restated.py, once per problem); the ctypes mirror, the exports and the default limit against include/mulls_hip.h, which must still compile
as plain C; the planner mulls_amd/csrc/fpfh_batch.h, compiled for the host as a stand-alone program (tests/fpfh_batch_harness.cpp): the counted bytes
against the header's formulas, the cuts, and the stretches of the flat hypothesis list; the bridge's batch calls as a compile check.
tests/test_gpu_fpfh_batch.py runs the calls on a device."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import fpfh_batch_plan as plan  # noqa: E402
from fpfh_names import GOLDEN  # noqa: E402
from mulls_amd import abi, lib  # noqa: E402
from test_ncc import REF_UTILITY  # noqa: E402  (where the reference tree is looked for)
from test_ndt import BRIDGE_TU  # noqa: E402


@pytest.fixture(scope="module")
def batch_golden():
    z = np.load(plan.BATCH_GOLDEN)
    return {k: z[k] for k in z.files}


# ---- 1. the fixture

def test_fixture_equals_the_restatement(batch_golden):
    pytest.importorskip("mpmath")
    import make_fpfh_batch_golden as maker

    assert maker.BATCH_GOLDEN == plan.BATCH_GOLDEN and maker.SCENES == plan.SCENES
    fresh = maker.compute()
    assert sorted(fresh) == sorted(batch_golden)
    for k in batch_golden:
        a, b = fresh[k], batch_golden[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_fixture_scenes_reach_their_edges(batch_golden):
    g, single = batch_golden, np.load(GOLDEN)
    assert tuple(json.loads(str(g["scenes"]))) == plan.SCENES
    ints = lambda s: g[s + "/ints"]
    # mixed: 65 hypotheses, one lane past a wave; five sizes, k_eff = 7 beside 15; no problem's answer is hypothesis 0
    assert ints("mixed")[:, 0].tolist() == [44, 41, 26, 33, 60] and (ints("mixed")[:, 1] == 65).all()
    assert ints("mixed")[:, 2:].tolist() == [[3, 80], [8, 24], [30, 7], [60, 80], [10, 20]]
    # chunks: 3 090 flat hypotheses; problem 0 is the single fixture's sac_chunks itself; the other winners lie in the second and the third stretch of 1 024
    assert ints("chunks")[:, 0].tolist() == [757, 163, 562] and (ints("chunks")[:, 1] == 1030).all()
    assert ints("chunks")[0].tolist() == single["sac_chunks/ints"].tolist()
    assert g["chunks/floats"][0].tobytes() == single["sac_chunks/floats"].tobytes() and g["chunks/T"][0].tobytes() == single["sac_chunks/T"].tobytes()
    flat = [b * 1030 + int(w) for b, w in enumerate(ints("chunks")[:, 0])]
    assert [f // 1024 for f in flat] == [0, 1, 2]
    # shared: one target against four sources, the first and the last the same; then the roles exchanged
    probs = json.loads(str(g["shared/problems"]))
    assert len({tuple(p[0]) for p in probs[:4]}) == 1 and probs[0] == probs[3] and probs[4] == [probs[0][1], probs[0][0]]
    assert json.loads(str(g["shared/prm"])) == json.loads(str(g["mixed/prm"]))
    for k in ("ints", "floats", "T"):
        assert g["shared/" + k][0].tobytes() == g["shared/" + k][3].tobytes()
    assert g["shared/T"][0].tobytes() == g["mixed/T"][3].tobytes()  # (sac_it64's own pair under the same parameters)
    assert ints("shared")[4, 2:].tolist() == [80, 60]
    # default: upstream's infinite range, hypothesis 0 wins in all, pinned
    assert np.isinf(abi.fpfhsac_params(**json.loads(str(g["default/prm"]))).max_correspondence_distance)
    assert ints("default")[:, 0].tolist() == [0, 0, 0] and (g["default/floats"][:, 0] == 0.0).all()
    # nan: errors that are NaN come after every number (the single fixture's winner 3), beside a problem of equal descriptors
    assert ints("nan")[:, 0].tolist() == [3, 0] and ints("nan")[0].tolist() == single["sac_nan_errors/ints"].tolist()
    assert json.loads(str(g["huber/prm"]))["error_function"] == abi.SACIA_HUBER and ints("huber")[0].tolist() == single["sac_huber/ints"].tolist()


# ---- 2. the ABI

def test_ctypes_layout_matches_header():
    ct, cname = abi.FpfhSacProblem, "mulls_fpfhsac_problem"
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "mulls_hip.h"', "int main(void){", 'printf("size %%zu\\n", sizeof(%s));' % cname]
    for f, _ in ct._fields_:
        prog.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f))
    prog.append('printf("limit %llu\\n", (unsigned long long)MULLS_FPFHSAC_BATCH_DEFAULT_SCRATCH_BYTES);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # (the header is still C99)
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got["size"]) == C.sizeof(ct) == 2 * C.sizeof(abi.Cloud)
    for f, _ in ct._fields_:
        assert int(got[f]) == getattr(ct, f).offset, f
    assert int(got["limit"]) == abi.FPFHSAC_BATCH_DEFAULT_SCRATCH_BYTES == 1024 << 20


def test_exports_and_null_context():
    names = ["mulls_compute_fpfh_batch", "mulls_coarse_reg_fpfhsac_batch"]
    header = open(os.path.join(ROOT, "include", "mulls_hip.h")).read()
    L = lib.load()
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.EXPORTS and hasattr(L, name), name
    assert "a value chosen without a measurement" in header[header.index("many FPFH clouds"):header.index("#define MULLS_FPFHSAC_BATCH_DEFAULT_SCRATCH_BYTES")]
    assert "A batch entry point is not built" not in header
    # argument checks that need no device
    assert L.mulls_compute_fpfh_batch(None, None, 0, None, None, None, 0) == abi.MULLS_E_INVALID
    assert L.mulls_compute_fpfh_batch(None, None, 3, None, None, None, 0) == abi.MULLS_E_INVALID
    assert L.mulls_coarse_reg_fpfhsac_batch(None, None, 0, None, 0, None) == abi.MULLS_E_INVALID
    assert L.mulls_coarse_reg_fpfhsac_batch(None, None, 2, None, 0, None) == abi.MULLS_E_INVALID


# ---- 3. the planner

@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fb") / "fpfh_batch_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "fpfh_batch_harness.cpp"), "-o", exe])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, check=True).stdout.decode()
        return [[int(v) for v in line.split()] for line in out.split("\n") if line]

    return run


def test_counted_bytes_are_the_headers(planner):
    for iters, ns, nt in ((65, 3, 80), (1030, 60, 80), (10, 16000, 20000), (1, 511, 513), (65536, 3, 1)):
        assert planner("bytes", iters, ns, nt) == [[plan.problem_bytes(ns, nt, iters), plan.cloud_bytes(ns), plan.cloud_bytes(nt), plan.HEAD_BYTES, plan.MAX_SLOTS,
                                                   plan.MAX_POOL_BYTES]]
    chunk = re.search(r"#define MULLS_FPFH_HYP_CHUNK (\d+)u", open(os.path.join(ROOT, "mulls_amd", "csrc", "fpfh_launch.h")).read())
    assert int(chunk.group(1)) == plan.MAX_SLOTS == abi.FPFH_HYP_CHUNK


def test_cuts(planner):
    sizes, iters = [(3, 80), (8, 24), (30, 7), (60, 80), (10, 20)], 65
    flat = [v for st in sizes for v in st]
    assert planner("cuts", 1, iters, *flat) == [[b] for b in range(6)]  # a problem larger than the limit runs alone
    assert planner("cuts", 1 << 40, iters, *flat) == [[0], [5]]
    limit = max(plan.counted(sizes[0:2], iters), plan.counted(sizes[2:4], iters))
    assert plan.cuts(sizes, iters, limit) == [0, 2, 4, 5] and planner("cuts", limit, iters, *flat) == [[0], [2], [4], [5]]
    many = [(3, 1)] * 2500
    assert planner("cuts", 1 << 40, 1, *[v for st in many for v in st]) == [[0], [1024], [2048], [2500]]  # at most 1 024 problems
    for lim in (plan.counted(sizes[:1], iters), plan.counted(sizes[:3], iters) - 1, plan.counted(sizes[:3], iters), plan.counted(sizes, iters) - 1):
        assert [c[0] for c in planner("cuts", lim, iters, *flat)] == plan.cuts(sizes, iters, lim), lim


def check_stretches(rows, n_src, iters, pool):
    """never more than 1 024 slots or the pool; every hypothesis once, in order; offsets 4-byte aligned, inside the pool and disjoint"""
    per = [4 * n for n in n_src for _ in range(iters)]  # the distance bytes of every flat hypothesis
    prefix = np.concatenate([[0], np.cumsum(per)])
    at = 0
    for h0, n, d0, nbytes, n_max in rows:
        assert h0 == at and 1 <= n <= plan.MAX_SLOTS and nbytes <= pool, (h0, n, nbytes)
        assert d0 == prefix[h0] and nbytes == prefix[h0 + n] - prefix[h0]
        offs = prefix[h0:h0 + n] - d0
        assert (offs % 4 == 0).all() and (np.diff(offs) == per[h0:h0 + n - 1]).all() and offs[-1] + per[h0 + n - 1] <= pool
        assert n_max == max(n_src[h // iters] for h in range(h0, h0 + n))
        at += n
    assert at == len(per)


def test_stretches(planner):
    cases = [([8, 60, 8], 1030, 1 << 30), ([8, 60, 8], 1030, 100 * 240), ([8, 60, 8], 1030, 240), ([3, 8, 30, 60, 10], 65, 1 << 30), ([3, 8, 30, 60, 10], 65, 240),
             ([1200], 120, 4800 * 7 + 3), ([5, 2000, 5], 1500, 8000 * 3), ([7], 1, 28), ([7, 9], 2048, 1 << 30)]
    for n_src, iters, pool in cases:
        rows = planner("stretches", pool, iters, *n_src)
        check_stretches(rows, n_src, iters, pool)
        if pool == 1 << 30:
            assert [r[1] for r in rows[:-1]] == [1024] * (len(rows) - 1)
    rows = planner("stretches", 100 * 240, 1030, 8, 60, 8)
    inside = [r for r in rows if 1030 <= r[0] and r[0] + r[1] <= 2060]
    assert len(inside) >= 9 and all(r[1] == 100 for r in inside[1:-1])  # a hundred hypotheses of the 60-point source a stretch
    assert planner("stretches", 240, 1030, 8, 60, 8)[0][:2] == [0, 7]  # a pool of one hypothesis of the largest source: 7 of the 8-point source fit
    assert len([r for r in planner("stretches", 240, 1030, 8, 60, 8) if r[4] == 60 and r[1] == 1]) >= 1029


def test_pool(planner):
    n_src, iters = [8, 60, 8], 1030
    sizes = [(8, 24), (60, 80), (8, 80)]
    counted = plan.counted(sizes, iters)
    for limit in (1, counted, counted - 3 * 256 + 24000, 1 << 40):
        assert planner("pool", limit, iters, counted, *n_src) == [[plan.pool_bytes(n_src, iters, counted, limit)]], limit
    assert plan.pool_bytes(n_src, iters, counted, 1) == 240 and plan.pool_bytes(n_src, iters, counted, counted - 768 + 24000) == 24000
    assert plan.pool_bytes(n_src, iters, counted, 1 << 40) == 4 * 76 * 1030  # no more than all hypotheses need
    assert plan.pool_bytes([1 << 20], 65536, counted, 1 << 40) == plan.MAX_POOL_BYTES


# ---- 4. the bridge

BATCH_CALLS = r"""
struct Signature33
{
	float histogram[33];
};
typedef boost::shared_ptr<pcl::PointCloud<Signature33>> fpfhPtr;
// the calls a loop-closure event's candidate loop would make in place of CRegistration::compute_fpfh_feature and coarse_reg_fpfhsac per candidate
std::vector<double> call_fpfh_batch(const std::vector<pcTPtr> &sources, const std::vector<pcTPtr> &targets, std::vector<pcTPtr> &traned_sources,
									std::vector<Eigen::Matrix4d> &transformationS2T, std::vector<fpfhPtr> &clouds_fpfh, float search_radius)
{
	lo::hip::compute_fpfh_feature_batch<Point_T>(sources, clouds_fpfh, search_radius);
	lo::hip::fpfhsac_params().max_correspondence_distance = 0.5f;
	return lo::hip::coarse_reg_fpfhsac_batch<Point_T>(sources, targets, traned_sources, transformationS2T, search_radius);
}
"""


def test_stand_alone_bridge_harness_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "fpfh_batch_bridge_harness.cpp")])


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_against_the_reference_types():
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 592, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(BRIDGE_TU + BATCH_CALLS)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
