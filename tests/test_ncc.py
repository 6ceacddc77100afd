"""CPU tests of the key-point descriptor matching (find_feature_correspondence_ncc, include/common/cregistration.hpp:409-601): the numpy restatement
the GPU tests compare against equals what the reference's own lines returned (fixture tests/golden/ncc_demo.npz, made by tests/golden/make_ncc_golden.py
where the reference tree exists); the entry point is declared in the C header, mirrored by the ctypes layer and exported by the library; the C++
bridge compiles and instantiates with the reference's call.  A second fixture (tests/golden/ncc_edges.npz, same generator) holds what those lines return on
small synthetic sets at the edges of the descriptor arithmetic: (int) and % of out-of-range codes, NaN target intensities at the first, a middle, the last and
two indices, all-negative target intensities (also behind a NaN), source intensities outside the target's range, infinite source heights, NaN source
curvatures, one infinite distance selected by corr_num.  The bridge runs in oracle/_ref/adapter_check (modes ncc, ncc_ref): its reference side is checked here
against the demo fixture, both sides against each other on the GPU (tests/test_gpu_adapter.py)."""
import ctypes as C
import json
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import ncc_restated
from mulls_amd import abi, build, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mulls_hip.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ncc_demo.npz")
EDGES = os.path.join(ROOT, "tests", "golden", "ncc_edges.npz")
ADAPTER_CHECK = os.path.join(ROOT, "oracle", "_ref", "adapter_check")
REF_UTILITY = os.path.join(os.environ.get("MULLS_REFERENCE", "/root/reference"), "include", "common", "utility.hpp")


def fixture_cases():
    Z = np.load(FIXTURE)
    for name in Z["cases"]:
        a, b, fixed, cn, recip, nt, const = (int(v) for v in Z[name + "_args"])
        t, s = Z["kpts_%d" % a].copy(), Z["kpts_%d" % b]
        if nt >= 0:
            t = t[:nt].copy()
        if const:
            t.view(np.float32).reshape(len(t), 12)[:, 8] = 7.0
        yield str(name), t, s, fixed, cn, recip, bool(Z[name + "_ok"]), Z[name + "_pairs"], Z


def edge_cases():
    Z = np.load(EDGES, allow_pickle=False)
    for name in Z["cases"]:
        k, fixed, cn, recip = (int(v) for v in Z[name + "_args"])
        sname = str(Z["sets"][k])
        yield str(name), Z[sname + "_t"], Z[sname + "_s"], fixed, cn, recip, bool(Z[name + "_ok"]), Z[name + "_pairs"]


def test_fixture_holds_arrays_only():
    Z = np.load(FIXTURE, allow_pickle=False)
    assert len(Z["cases"]) == 10 and Z["kpts_0"].shape == (2840, 48) and Z["kpts_15"].shape == (2767, 48)
    assert all(Z[k].dtype.kind in "iufU" for k in Z.files)
    tied = [str(n) for n in Z["cases"] if n + "_tied" in Z.files and int(Z[n + "_tied"])]
    assert len(tied) <= 2, tied  # the condition under which the fixed-number cases may be compared at all


def test_restatement_equals_the_reference_lines():
    seen = 0
    for name, t, s, fixed, cn, recip, ok, pairs, _ in fixture_cases():
        got_ok, got = ncc_restated.restate(t, s, fixed, cn, recip)
        assert got_ok == ok, name
        assert got.shape == pairs.shape and np.array_equal(got, pairs), name  # every case exactly, the one with an equal pair in its sorted prefix included
        seen += 1
    assert seen == 10
    Z = np.load(FIXTURE)
    assert len(Z["recip_0_15_pairs"]) == 517 and len(Z["fixed2000_0_15_pairs"]) == 1543 and not bool(Z["few_0_15_ok"])
    assert np.array_equal(Z["const_recip_0_15_pairs"], np.stack([np.arange(2840), np.zeros(2840)], 1))  # every distance a NaN: (i, 0)


def test_edges_fixture_holds_arrays_only_and_what_it_claims():
    Z = np.load(EDGES, allow_pickle=False)
    assert all(Z[k].dtype.kind in "iufU" for k in Z.files)
    assert os.path.getsize(EDGES) <= os.path.getsize(FIXTURE)
    F = lambda raw: ncc_restated.fields(raw)
    for sname in Z["sets"]:
        assert Z[sname + "_t"].shape[1] == 48 and 10 <= len(Z[sname + "_t"]) <= 700 and 10 <= len(Z[sname + "_s"]) <= 700, sname
    for sname, at in (("nan_first", [0]), ("nan_middle", [150]), ("nan_last", [299]), ("nan_two", [37, 211])):
        assert list(np.nonzero(np.isnan(F(Z[sname + "_t"])["inten"]))[0]) == at and len(Z[sname + "_t"]) == 300, sname
    assert (F(Z["negative_t"])["inten"] < 0).all() and ncc_restated.intensity_range(F(Z["negative_t"])["inten"])[1] == 0
    lo, hi = ncc_restated.intensity_range(F(Z["nan_negative_t"])["inten"])
    assert np.isnan(F(Z["nan_negative_t"])["inten"][0]) and (F(Z["nan_negative_t"])["inten"][1:] < 0).all() and lo < hi < 0  # no clamp behind a NaN
    lo, hi = ncc_restated.intensity_range(F(Z["outside_t"])["inten"])
    assert (F(Z["outside_s"])["inten"] > hi).sum() > 20 and (F(Z["outside_s"])["inten"] < lo).sum() > 20
    assert np.isposinf(F(Z["inf_height_s"])["h"]).sum() == 10 and np.isfinite(F(Z["inf_height_t"])["h"]).all()
    assert np.isnan(F(Z["nan_source_s"])["n3"]).sum() > 20
    # one +inf distance and no two equal ones: corr_num = 144 takes the whole table, the infinite entry last, and the walk still has room for its pair
    lo, hi = ncc_restated.intensity_range(F(Z["inf_single_t"])["inten"])
    dt = ncc_restated.table(ncc_restated.descriptors(Z["inf_single_t"], lo, hi), ncc_restated.descriptors(Z["inf_single_s"], lo, hi))
    assert dt.shape == (12, 12) and np.isposinf(dt).sum() == 1 and np.isposinf(dt[5, 7]) and len(np.unique(dt)) == 144
    assert not int(Z["inf_single_fixed144_tied"]) and list(Z["inf_single_fixed144_pairs"][-1]) == [5, 7]
    assert np.array_equal(Z["inf_single_fixed143_pairs"], Z["inf_single_fixed144_pairs"][:-1])
    c = ncc_restated.f2i(F(Z["bigcodes_t"])["n0"])
    assert (c == ncc_restated.INT_MIN).sum() >= 4 and (np.abs(c) > 2 ** 24).sum() > 100 and (c < 0).sum() > 100
    names = [str(n) for n in Z["cases"]]
    for sname in Z["sets"]:
        assert sname + "_recip" in names and sname + "_nn" in names, sname
    fixed = [n for n in names if n + "_tied" in Z.files]
    assert {n.rsplit("_", 1)[0] for n in fixed} == {"bigcodes", "negative", "outside", "inf_height", "inf_single"}  # no fixed-number case where a NaN distance exists


def test_restatement_equals_the_reference_lines_at_the_edges():
    """every case of ncc_edges.npz exactly: the restatement's (int) / %, its NaN and inf handling and its min_ / max_ fold against the reference's own lines"""
    seen = 0
    for name, t, s, fixed, cn, recip, ok, pairs in edge_cases():
        got_ok, got = ncc_restated.restate(t, s, fixed, cn, recip)
        assert got_ok == ok, name
        assert got.shape == pairs.shape and np.array_equal(got, pairs), name
        seen += 1
    assert seen == 33
    Z = np.load(EDGES)
    assert np.array_equal(Z["nan_last_recip_pairs"], np.stack([np.arange(300), np.zeros(300)], 1))  # NaN range: every distance a NaN, (i, 0)
    assert np.array_equal(Z["nan_last_nn_pairs"], Z["nan_last_recip_pairs"])
    assert list(Z["nan_first_nn_pairs"][0]) == [0, 0] and len(np.unique(Z["nan_first_nn_pairs"][1:, 1])) > 50  # the NaN row alone keeps column 0


def write_adapter_dump(path, tgt0, src0):
    """adapter_check's input format (tests/test_gpu_adapter.py: dump()) with one cloud in slot 0 of each side"""
    with open(path, "wb") as f:
        for c in (tgt0, src0):
            f.write(struct.pack("<I", len(c)))
            f.write(np.ascontiguousarray(c).tobytes())
            f.write(struct.pack("<I", 0) * 5)
        f.write(np.eye(4).tobytes())
        f.write(np.zeros(6).tobytes())


def pairs_by_bytes(t, s, tc, sc):
    wt, ws = {r.tobytes(): i for i, r in enumerate(t)}, {r.tobytes(): i for i, r in enumerate(s)}
    return np.array([(wt[a.tobytes()], ws[b.tobytes()]) for a, b in zip(tc, sc)], np.int64).reshape(-1, 2)


def adapter_check_has(mode):
    """oracle/_ref/adapter_check exists and was built from this tree's oracle/adapter_check.cpp, which knows `mode`: an oracle/_ref/ left by an older recipe
    (build() rebuilds it only where the reference tree is) holds a binary that takes any unknown mode for "reg" and starts the device.  The binary names
    its modes in the message it has for an unknown one."""
    return os.path.exists(ADAPTER_CHECK) and (" %s" % mode).encode() in open(ADAPTER_CHECK, "rb").read()


@pytest.mark.skipif(not adapter_check_has("ncc_ref"), reason="oracle/_ref/adapter_check with the ncc modes not built (needs the reference tree)")
def test_adapter_check_reference_side_equals_the_fixture():
    """adapter_check <file> ncc_ref: the reference member inside the binary that also runs the bridge, without a device.  Its output clouds, written next
    to the dump, hold the fixture's pairs (records looked up by their bytes); the printed sizes, bools and the pre-fill / too-few cases are as the lines have them."""
    Z = np.load(FIXTURE)
    for a, b in ((0, 15), (15, 0)):
        t, s = Z["kpts_%d" % a], Z["kpts_%d" % b]
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "kpts.bin")
            write_adapter_dump(path, t, s)
            out = subprocess.check_output([ADAPTER_CHECK, path, "ncc_ref"], timeout=300).decode().strip().split("\n")
            rows = [json.loads(l) for l in out]
            assert all(r["who"] == "reference" for r in rows)
            rows = {r["mode"]: r for r in rows}
            for mode, case in (("recip", "recip"), ("nn", "nn"), ("fixed2000", "fixed2000")):
                r, want = rows[mode], Z["%s_%d_%d_pairs" % (case, a, b)]
                clouds = np.fromfile(path + ".reference." + mode, np.uint8).reshape(2, -1, 48)
                assert r["ok"] is True and r["n_target"] == r["n_source"] == len(want) == clouds.shape[1], (mode, a, b)
                assert np.array_equal(pairs_by_bytes(t, s, clouds[0], clouds[1]), want), (mode, a, b)
            # fixed_num_corr with 300 and reciprocal_on false (the fixture's fixed300 cases pass true, which that mode ignores)
            want = Z["fixed300_%d_%d_pairs" % (a, b)]
            clouds = np.fromfile(path + ".reference.fixed300", np.uint8).reshape(2, -1, 48)
            assert np.array_equal(pairs_by_bytes(t, s, clouds[0], clouds[1]), want)
            # appended behind three points that were there, which stay as they were
            r, want = rows["recip_prefilled"], Z["recip_%d_%d_pairs" % (a, b)]
            clouds = np.fromfile(path + ".reference.recip_prefilled", np.uint8).reshape(2, -1, 48)
            assert r["ok"] is True and r["n_target"] == r["n_source"] == len(want) + 3
            assert np.array_equal(clouds[0, :3], s[:3]) and np.array_equal(clouds[1, :3], t[:3])
            assert np.array_equal(pairs_by_bytes(t, s, clouds[0, 3:], clouds[1, 3:]), want)
            assert rows["recip_prefilled"]["hash_target"] != rows["recip"]["hash_target"]
            r = rows["few"]
            assert r["ok"] is False and r["n_target"] == r["n_source"] == 3  # 9 target points: false, the clouds left as they were
            clouds = np.fromfile(path + ".reference.few", np.uint8).reshape(2, -1, 48)
            assert np.array_equal(clouds[0], s[:3]) and np.array_equal(clouds[1], t[:3])
    assert len(Z["recip_0_15_pairs"]) == 517 and len(Z["fixed2000_0_15_pairs"]) == 1543


def test_restatement_degenerate_cases():
    t, s = ncc_restated.random_kpts(1, 40), ncc_restated.random_kpts(2, 50)
    assert ncc_restated.restate(t[:9], s)[0] is False and ncc_restated.restate(t, s[:9])[0] is False
    const = t.copy()
    const.view(np.float32).reshape(len(const), 12)[:, 8] = 7.0
    assert len(ncc_restated.restate(const, s, True, 300, False)[1]) == 0  # NaN distances are never selected
    assert len(ncc_restated.restate(t, s, True, 0, False)[1]) == 0
    ok, p = ncc_restated.restate(t, s, True, 65536, False)  # more than the table holds: all of it walked, seven uses per point at most
    assert ok and len(p) == 7 * 40 and np.bincount(p[:, 0]).max() == 7 and np.bincount(p[:, 1]).max() <= 7
    # row chunking does not change a result
    q = ncc_restated.random_kpts(3, 300, "quantised"), ncc_restated.random_kpts(4, 200, "quantised")
    whole = [ncc_restated.restate(q[0], q[1], f, 500, r)[1] for f, r in ((0, 1), (0, 0), (1, 0))]
    keep = ncc_restated.CHUNK_ENTRIES
    try:
        ncc_restated.CHUNK_ENTRIES = 200 * 7
        parts = [ncc_restated.restate(q[0], q[1], f, 500, r)[1] for f, r in ((0, 1), (0, 0), (1, 0))]
    finally:
        ncc_restated.CHUNK_ENTRIES = keep
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    # (int) and % as the x86 build evaluates them
    assert list(ncc_restated.f2i(np.array([3.0e9, -3.0e9, np.nan, -7.9, 16777218.0], np.float32))) == [-2 ** 31, -2 ** 31, -2 ** 31, -7, 16777218]
    d = ncc_restated.descriptors(ncc_restated.make_records([0], [-12345678.0], [3.0e9], [0], [1]), 0, 1)
    assert list(d[0, :8]) == [-12, -34, -56, -78, -2147, -48, -36, -48]


def test_header_abi_and_defaults():
    """fails without the feature: the header declares the entry point and its parameter struct, the ctypes mirror has the same layout, the library exports both
    functions and the defaults are the reference's (cregistration.hpp:411)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+mulls_ncc_correspond\s*\(\s*mulls_ctx\s*\*", text) and re.search(r"\bvoid\s+mulls_ncc_default_params\s*\(", text)
    names = [f[0] for f in abi.NccParams._fields_]
    assert names == ["fixed_num_corr", "corr_num", "reciprocal_on", "reserved"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mulls_hip.h"', "int main(void){", 'printf("size %zu\\n", sizeof(mulls_ncc_params));']
    prog += ['printf("%s %%zu\\n", offsetof(mulls_ncc_params, %s));' % (f, f) for f in names] + ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got["size"]) == C.sizeof(abi.NccParams) == 16
    for f in names:
        assert int(got[f]) == getattr(abi.NccParams, f).offset, f
    build.build()
    L = lib.load()
    assert "mulls_ncc_correspond" in lib.EXPORTS and "mulls_ncc_default_params" in lib.EXPORTS
    p = abi.NccParams(7, 7, 7, 7)
    L.mulls_ncc_default_params(C.byref(p))
    assert (p.fixed_num_corr, p.corr_num, p.reciprocal_on, p.reserved) == (0, 2000, 1, 0)
    q = abi.ncc_params()
    assert (q.fixed_num_corr, q.corr_num, q.reciprocal_on) == (0, 2000, 1)
    # argument checks that need no device
    n = C.c_uint32(5)
    assert L.mulls_ncc_correspond(None, None, None, None, None, None, 0, C.byref(n)) == abi.MULLS_E_INVALID


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
// the call of test/mulls_reg.cpp:173-174, and the defaults of cregistration.hpp:411
bool call(lo::constraint_t &reg_con, bool fixed_num_corr_on, int feature_correspondence_num, bool reciprocal_corr_on)
{
	pcTPtr target_cor(new pcT()), source_cor(new pcT());
	bool a = lo::hip::find_feature_correspondence_ncc<Point_T>(reg_con.block1->pc_vertex, reg_con.block2->pc_vertex, target_cor, source_cor, fixed_num_corr_on,
															   feature_correspondence_num, reciprocal_corr_on);
	bool b = lo::hip::find_feature_correspondence_ncc<Point_T>(reg_con.block1->pc_vertex, reg_con.block2->pc_vertex, target_cor, source_cor);
	return a && b && target_cor->points.size() == source_cor->points.size();
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_with_the_reference_call():
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        # the ranges oracle/build_ref.sh cuts for the same purpose, into a directory that goes away with the test
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 590, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(BRIDGE_TU)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
