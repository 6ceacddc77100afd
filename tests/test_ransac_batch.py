"""CPU tests of mulls_coarse_reg_ransac_batch's host side: the layout of mulls_ransac_problem in include/mulls_hip.h against mulls_amd/abi.py and the exported
symbol, the planner (mulls_amd/csrc/ransac_batch.h through tests/ransac_batch_harness.cpp: the sub-batch cuts, the arena's offsets, the descriptor table), the
resumable refinement control of ransac_host.h against refine_control and against PCL's loop written out here, and the bridge
lo::hip::coarse_reg_ransac_batch against the reference's types.  The device is tested in tests/test_gpu_ransac_batch.py."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mulls_amd import abi, lib
from test_ncc import REF_UTILITY
from test_ransac import BRIDGE_TU, ROOT, vp

KEYS = ("src", "tgt", "idx", "tri", "models", "counts", "mask", "d2", "round", "n", "n_hyp", "best", "mask_stride")
INFO = ("dev_bytes", "pin_bytes", "o_desc", "o_win", "o_gather", "o_jobs", "o_pts", "pts_bytes", "o_tri", "tri_bytes", "o_counts", "counts_bytes", "o_mask",
        "mask_bytes", "o_round", "round_bytes")
SIZES = [3, 8, 64, 65, 517, 65536]


def test_problem_layout_and_export():
    """mulls_ransac_problem as the header lays it out, the default limit, the symbol in the built library"""
    names = [f[0] for f in abi.RansacProblem._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){", 'printf("size %zu\\n", sizeof(mulls_ransac_problem));']
    for f in names:
        prog.append('printf("%s %%zu\\n", offsetof(mulls_ransac_problem, %s));' % (f, f))
    prog.append('printf("limit %llu\\n", (unsigned long long)MULLS_RANSAC_BATCH_DEFAULT_SCRATCH_BYTES);')
    prog.append('printf("count %d\\n", (int)MULLS_OPT_COUNT);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # the header is still plain C
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got["size"]) == C.sizeof(abi.RansacProblem) == 64
    for f in names:
        assert int(got[f]) == getattr(abi.RansacProblem, f).offset, f
    assert [getattr(abi.RansacProblem, f).offset for f in names] == [getattr(abi.TeaserProblem, f[0]).offset for f in abi.TeaserProblem._fields_]  # its shape
    assert int(got["limit"]) == abi.RANSAC_BATCH_DEFAULT_SCRATCH_BYTES == 512 << 20
    assert int(got["count"]) == 29  # no option was added
    assert "mulls_coarse_reg_ransac_batch" in lib.EXPORTS
    fn = lib.load().mulls_coarse_reg_ransac_batch
    assert fn(None, None, 0, None, 0, None) == abi.MULLS_E_INVALID  # no context


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ransac_batch_harness") / "ransac_batch_harness.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "ransac_batch_harness.cpp"),
                           "-o", so])
    L = C.CDLL(so)
    L.rb_problem_bytes.restype = C.c_uint64
    L.rb_problem_bytes.argtypes = [C.c_uint32, C.c_int32]
    for f in (L.rb_desc_bytes, L.rb_gather_bytes, L.rb_job_bytes, L.rb_max_problems, L.rb_cuts):
        f.restype = C.c_uint32
    L.rb_cuts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    L.rb_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
    L.rb_refine.argtypes = [C.c_int, C.c_double, C.c_uint32] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int]
    return L


def cuts(L, sizes, limit):
    b = np.ascontiguousarray(sizes, np.uint64)
    out = np.zeros(len(b) + 2, np.uint32)
    k = L.rb_cuts(vp(b), len(b), limit, vp(out))
    return [int(v) for v in out[:k]]


def layout(L, n, max_iter):
    n = np.ascontiguousarray(n, np.uint32)
    desc, info = np.zeros((max(len(n), 1), len(KEYS)), np.uint64), np.zeros(len(INFO), np.uint64)
    L.rb_layout(vp(n), len(n), max_iter, vp(desc), vp(info))
    rows = [dict(zip(KEYS, (int(v) for v in r))) for r in desc[: len(n)]]
    return rows, dict(zip(INFO, (int(v) for v in info)))


def up256(v):
    return -(-v // 256) * 256


def arrays(r, hyp):
    """(offset, bytes) of every array of a problem in the arena"""
    n = r["n"]
    return {"src": (r["src"], 16 * n), "tgt": (r["tgt"], 16 * n), "idx": (r["idx"], 8 * n), "tri": (r["tri"], 12 * hyp), "models": (r["models"], 48 * hyp),
            "counts": (r["counts"], 4 * hyp), "mask0": (r["mask"], n), "mask1": (r["mask"] + r["mask_stride"], n), "mask2": (r["mask"] + 2 * r["mask_stride"], n),
            "d2": (r["d2"], 4 * n), "round": (r["round"], 64)}


def assert_disjoint(spans, end):
    spans = sorted(s for s in spans if s[1])
    for (a, la), (b, _) in zip(spans, spans[1:]):
        assert a + la <= b, (a, la, b)
    assert not spans or spans[-1][0] + spans[-1][1] <= end


@pytest.mark.parametrize("max_iter", [1, 20000])
def test_offsets_are_aligned_and_disjoint(planner, max_iter):
    hyp = max_iter + 1  # iteration max_iter_num is still evaluated
    rows, info = layout(planner, SIZES, max_iter)
    spans = []
    for r, n in zip(rows, SIZES):
        assert r["n"] == n and r["n_hyp"] == 0 and r["best"] == 2**64 - 1 and r["mask_stride"] == up256(n)
        for name, (off, size) in arrays(r, hyp).items():
            assert off % 256 == 0 and off >= info["o_pts"], name
            spans.append((off, size))
    assert_disjoint(spans, info["dev_bytes"])
    # the tables lie in front of the arrays, one entry per problem, and do not overlap
    B = len(SIZES)
    tables = [(info["o_desc"], planner.rb_desc_bytes() * B), (info["o_win"], 64 * B), (info["o_gather"], 2 * planner.rb_gather_bytes() * B),
              (info["o_jobs"], planner.rb_job_bytes() * B)]
    assert all(t[0] % 8 == 0 for t in tables) and planner.rb_desc_bytes() % 8 == 0 and planner.rb_gather_bytes() % 8 == 0 and planner.rb_job_bytes() % 8 == 0
    assert_disjoint(tables, info["o_pts"])
    assert tables[-1][0] + tables[-1][1] <= 512 * B  # the share the cuts count
    # the arena is what the cuts count, or less; a problem's bytes hold its arrays
    need = [planner.rb_problem_bytes(n, max_iter) for n in SIZES]
    assert info["dev_bytes"] <= sum(need)
    for r, n, b in zip(rows, SIZES, need):
        assert b == sum(up256(size) for _, size in arrays(r, hyp).values()) + 512
        assert layout(planner, [n], max_iter)[1]["dev_bytes"] <= b
    # the regions that travel in one copy are packed in problem order: points, triples, counts, masks, round records
    for key, first in (("pts", "src"), ("tri", "tri"), ("counts", "counts"), ("mask", "mask"), ("round", "round")):
        assert rows[0][first] == info["o_" + key]
        assert [r[first] for r in rows] == sorted(r[first] for r in rows)
        last = arrays(rows[-1], hyp)["tgt" if key == "pts" else ("mask2" if key == "mask" else first)]
        assert info["o_" + key] + info[key + "_bytes"] == last[0] + up256(last[1])
    assert info["tri_bytes"] == B * up256(12 * hyp) and info["counts_bytes"] == B * up256(4 * hyp) and info["round_bytes"] == 256 * B
    assert layout(planner, SIZES, -5)[1]["tri_bytes"] == B * 256  # a negative max_iter_num: one hypothesis, as the single call


def check_partition(c, count):
    assert c[0] == 0 and c[-1] == count and all(a < b for a, b in zip(c, c[1:]))  # every problem in exactly one sub-batch, order kept


@pytest.mark.parametrize("max_iter", [1, 20000])
def test_cuts(planner, max_iter):
    assert cuts(planner, [], 1 << 30) == [0]  # the empty batch: no sub-batch
    need = [planner.rb_problem_bytes(n, max_iter) for n in SIZES]
    assert cuts(planner, need, 1) == list(range(len(SIZES) + 1))  # a limit of 1 byte: one problem per sub-batch (each is larger than the limit and runs alone)
    assert cuts(planner, need, sum(need)) == [0, len(SIZES)]
    assert cuts(planner, need, sum(need) - 1) == [0, len(SIZES) - 1, len(SIZES)]
    for limit in (need[0] + need[1], sum(need[:3]), sum(need[:3]) + 1, need[5], need[5] - 1, sum(need[:5]) - 1):
        c = cuts(planner, need, limit)
        check_partition(c, len(SIZES))
        for a, b in zip(c, c[1:]):
            assert sum(need[a:b]) <= limit or b == a + 1  # fits, or alone
            assert b == len(SIZES) or sum(need[a:b + 1]) > limit  # and takes what fits
    cap = planner.rb_max_problems()  # the grid axis bounds a sub-batch too
    assert cuts(planner, [256] * (cap + 5), 1 << 40) == [0, cap, cap + 5]


# ---------------------------------------------------------------------------------------------------------------- the resumable refinement control
def pcl_refine(noise_bound, n_in, script):
    """RandomSampleConsensus::refineModel(3.0, 1000)'s control flow (sac.h) written out around a script of rounds: the outcome, the (prev, next) buffers and
    the squared thresholds of the rounds"""
    nb = float(np.float32(noise_bound))
    thr_sqr, error_threshold = nb * nb, nb
    prev, prev_size, sizes, rounds, log, thr = 0, n_in, [], 0, [], []
    out = dict(rounds=0, failed=0, oscillating=0, final_mask=0, n_inliers=0)
    while True:
        nxt = 2 if prev == 1 else 1
        n_new, changed, median = script[min(rounds, len(script) - 1)]
        log.append((prev, nxt))
        thr.append(error_threshold * error_threshold)
        rounds += 1
        out["rounds"] = rounds
        sizes.append(prev_size)
        if not n_new:
            out["failed"] = 1
            return out, log, thr
        error_threshold = math.sqrt(min(thr_sqr, 9.0 * (2.1981 * float(np.float32(median)))))
        new_size, prev_size, prev = prev_size, n_new, nxt
        if new_size != prev_size:
            if len(sizes) >= 4 and sizes[-1] == sizes[-3] and sizes[-2] == sizes[-4]:
                out["oscillating"] = 1
                return out, log, thr
            inlier_changed = True
        else:
            inlier_changed = bool(changed)
        if not (inlier_changed and rounds < 1000):
            break
    out.update(failed=int(inlier_changed), final_mask=prev, n_inliers=prev_size)
    return out, log, thr


def run_refine(L, resumable, noise_bound, n_in, script):
    n_new = np.array([r[0] for r in script], np.uint32)
    changed = np.array([r[1] for r in script], np.int32)
    median = np.array([r[2] for r in script], np.float32)
    out, log, thr = np.zeros(5, np.int32), np.full(2 * 1000, -1, np.int32), np.zeros(1000)
    L.rb_refine(resumable, float(np.float32(noise_bound)), n_in, vp(n_new), vp(changed), vp(median), len(script), vp(out), vp(log), vp(thr), 1000)
    keys = ("rounds", "failed", "oscillating", "final_mask", "n_inliers")
    return dict(zip(keys, (int(v) for v in out))), [tuple(int(v) for v in r) for r in log.reshape(-1, 2)[: out[0]]], thr[: out[0]]


SCRIPTS = {
    "converging": ([(120, 1, 0.004), (130, 1, 0.003), (130, 0, 0.003)], dict(rounds=3, failed=0, oscillating=0, final_mask=1, n_inliers=130)),
    "empty selection": ([(50, 1, 0.01), (0, 1, 0.0)], dict(rounds=2, failed=1, oscillating=0, final_mask=0, n_inliers=0)),
    "empty at once": ([(0, 1, 0.0)], dict(rounds=1, failed=1, oscillating=0, final_mask=0, n_inliers=0)),
    "1000 rounds still changing": ([(101 + r, 1, 0.01) for r in range(1001)], dict(rounds=1000, failed=1, oscillating=0, final_mask=2, n_inliers=1100)),
    # the only cover of the oscillating exit: none of the committed input sets takes it
    "2-cycle of set sizes": ([(90, 1, 0.01), (100, 1, 0.01), (90, 1, 0.01), (100, 1, 0.01), (95, 1, 0.01)], dict(rounds=4, failed=0, oscillating=1, final_mask=0, n_inliers=0)),
    "equal sizes, changed set": ([(100, 1, 0.004), (100, 0, 0.004)], dict(rounds=2, failed=0, oscillating=0, final_mask=2, n_inliers=100)),
    "three sizes repeat: no cycle": ([(90, 1, 0.01), (100, 1, 0.01), (80, 1, 0.01), (80, 0, 0.01)], dict(rounds=4, failed=0, oscillating=0, final_mask=2, n_inliers=80)),
    "a large median leaves the bound": ([(100, 1, 1.0), (100, 0, 1.0)], dict(rounds=2, failed=0, oscillating=0, final_mask=2, n_inliers=100)),
}


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_resumable_control_equals_refine_control(planner, name):
    """refine_begin / refine_feed fed one round at a time, refine_control's loop and PCL's loop as written out above: the rounds, the prev / next sequence, the
    thresholds' bits and the outcome"""
    script, want = SCRIPTS[name]
    for nb in (0.5, 0.3):
        loop, resumable, stated = run_refine(planner, 0, nb, 100, script), run_refine(planner, 1, nb, 100, script), pcl_refine(nb, 100, script)
        assert loop[0] == resumable[0] == stated[0] == want, name
        assert loop[1] == resumable[1] == stated[1]
        assert loop[2].tobytes() == resumable[2].tobytes() == np.array(stated[2]).tobytes()
        log = loop[1]
        assert log[0] == (0, 1) and all(nxt in (1, 2) and prev != nxt for prev, nxt in log) and all(p != 0 for p, _ in log[1:])  # buffer 0 is never written
        assert all(a[1] == b[0] for a, b in zip(log, log[1:]))  # a round fits what the round before selected


BATCH_TU = BRIDGE_TU.split("// the call of test/mulls_reg.cpp:179")[0] + r"""
// the candidates of test/mulls_slam.cpp:517-557 under --teaser_based_global_registration_on=false, solved together
std::vector<int> call(std::vector<pcTPtr> &targets, std::vector<pcTPtr> &sources, std::vector<Eigen::Matrix4d> &trans, float keypoint_nms_radius)
{
	std::vector<int> a = lo::hip::coarse_reg_ransac_batch<Point_T>(targets, sources, trans, 4.0 * keypoint_nms_radius);
	std::vector<int> b = lo::hip::coarse_reg_ransac_batch<Point_T>(targets, sources, trans);
	std::vector<int> c = lo::hip::coarse_reg_ransac_batch<Point_T>(targets, sources, trans, 0.2, 8, 20000);
	a.insert(a.end(), b.begin(), b.end());
	a.insert(a.end(), c.begin(), c.end());
	return a;
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_batch_bridge_compiles_against_the_reference_types():
    """lo::hip::coarse_reg_ransac_batch on vectors of the reference's cloud pointers and Eigen::Matrix4d, as tests/test_ransac.py checks the single bridge"""
    assert "coarse_reg_ransac_batch" not in BRIDGE_TU and "cregistration_hip.hpp" in BATCH_TU
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
