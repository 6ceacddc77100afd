"""Regenerates tests/golden/ncc_demo.npz: what the reference's own find_feature_correspondence_ncc lines return on the key points of its demo scans.

    python tests/golden/make_ncc_golden.py      (needs the reference tree and oracle/_ref/, i.e. __graft_entry__.build() run where the tree exists)

The two demo scans come out of tests/golden/demo_pair.npz (scan_0, scan_15); the reference's extract_semantic_pts (oracle/pyref.py) with
make_demo_pair_golden.extract_params()'s values (ncc_restated.demo_extract_params) leaves their key points (pc_vertex, MULLS_EX_VERTEX: 2840 and 2767 records).  Lines 409-601 of the
reference's include/common/cregistration.hpp are cut into a temporary directory at run time, compiled -O3 -ffp-contract=off inside a class shell against
oracle/ref_shim/shim.hpp, and called for both directions x four modes, plus the two degenerate cases.  Nothing cut or compiled from the reference is kept:
the fixture holds the key-point records and index arrays only.

Fixture contents: kpts_0, kpts_15 ((n, 48) uint8 records); cases (names); per case <name>_args = (target scan, source scan, fixed_num_corr, corr_num,
reciprocal_on, n_target or -1, constant_target_intensity), <name>_ok, <name>_pairs ((n, 2) int32: target, source index in push_back order), and for the
fixed-number cases <name>_tied = 1 when the sorted prefix of corr_num + 1 distances holds two equal neighbours (the order upstream's unstable sort leaves
among them is not defined: such a case may be compared as a set up to the tied entries only).
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mulls_amd import abi  # noqa: E402
from oracle import pyref  # noqa: E402
import ncc_restated  # noqa: E402

REF_HEADER = "/root/reference/include/common/cregistration.hpp"
FIRST, LAST = 409, 601

WRAPPER = r"""
#include <chrono>
#include <cfloat>
#include <cmath>
#include <algorithm>
#include <vector>
#include "ref_shim/shim.hpp"
#ifndef max_
#define max_(a, b) (((a) > (b)) ? (a) : (b))
#endif
#ifndef min_
#define min_(a, b) (((a) < (b)) ? (a) : (b))
#endif
namespace Eigen
{
struct VectorXf
{
	std::vector<float> v;
	explicit VectorXf(int n) : v(n) {}
	float &operator()(int i) { return v[i]; }
	const float &operator()(int i) const { return v[i]; }
};
} // namespace Eigen
template <typename PointT>
class Shell
{
  public:
#include "ncc_lines.inc"
};
typedef pcl::PointXYZINormal P;
extern "C" int ncc_lines(const P *t, int nt, const P *s, int ns, int fixed, int corr_num, int recip, P *to, P *so)
{
	pcl::PointCloud<P>::Ptr T(new pcl::PointCloud<P>()), S(new pcl::PointCloud<P>()), TO(new pcl::PointCloud<P>()), SO(new pcl::PointCloud<P>());
	T->points.assign(t, t + nt);
	S->points.assign(s, s + ns);
	Shell<P> c;
	if (!c.find_feature_correspondence_ncc(T, S, TO, SO, fixed != 0, corr_num, recip != 0))
		return -1;
	for (size_t i = 0; i < TO->points.size(); i++)
		to[i] = TO->points[i], so[i] = SO->points[i];
	return (int)TO->points.size();
}
"""


def build_lines(tmp):
    lines = open(REF_HEADER, errors="replace").read().split("\n")
    assert "bool find_feature_correspondence_ncc" in lines[FIRST - 1], "the reference's header is not the pinned one"
    open(os.path.join(tmp, "ncc_lines.inc"), "w").write("\n".join(lines[FIRST - 1:LAST]) + "\n")
    open(os.path.join(tmp, "wrap.cpp"), "w").write(WRAPPER)
    so = os.path.join(tmp, "libncc_lines.so")
    subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++14", "-shared", "-fPIC", "-w", "-I", os.path.join(ROOT, "oracle"), "-I", tmp,
                           os.path.join(tmp, "wrap.cpp"), "-o", so])
    return C.CDLL(so)


def index_of(cloud, recs):
    """indices of the returned records in their cloud (every record of a cloud is unique: asserted by main)"""
    where = {r.tobytes(): i for i, r in enumerate(cloud)}
    return np.array([where[r.tobytes()] for r in recs], np.int32)


def run_lines(L, traw, sraw, fixed, corr_num, recip):
    cap = max(len(traw), corr_num) + 8
    to, so = np.zeros((cap, 48), np.uint8), np.zeros((cap, 48), np.uint8)
    n = L.ncc_lines(traw.ctypes.data_as(C.c_void_p), len(traw), sraw.ctypes.data_as(C.c_void_p), len(sraw), int(fixed), int(corr_num), int(recip),
                    to.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p))
    if n < 0:
        return False, np.zeros((0, 2), np.int32)
    return True, np.stack([index_of(traw, to[:n]), index_of(sraw, so[:n])], 1).astype(np.int32)


def tied_prefix(traw, sraw, corr_num):
    imin, imax = ncc_restated.intensity_range(ncc_restated.fields(traw)["inten"])
    dt = ncc_restated.table(ncc_restated.descriptors(traw, imin, imax), ncc_restated.descriptors(sraw, imin, imax)).reshape(-1)
    s = np.sort(dt[~np.isnan(dt)])[: corr_num + 1]
    return int((np.diff(s) == 0).any())


def main():
    Z = np.load(os.path.join(HERE, "demo_pair.npz"))
    X = ncc_restated.demo_extract_params()
    V = {}
    for k in (0, 15):
        a = Z["scan_%d" % k]
        ex, _ = pyref.extract_semantic_pts(abi.make_points(a[:, :3], None, a[:, 3], None), X)
        V[k] = np.ascontiguousarray(abi.records(ex[abi.EX_VERTEX]))
        assert len({r.tobytes() for r in V[k]}) == len(V[k]), "key-point records are not unique in scan %d" % k
        print("scan %d: %d key points" % (k, len(V[k])))
    out = {"kpts_0": V[0], "kpts_15": V[15]}
    names, flagged = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        L = build_lines(tmp)
        L.ncc_lines.restype = C.c_int
        cases = []
        for a, b in ((0, 15), (15, 0)):
            for tag, fixed, cn, recip in (("recip", 0, 2000, 1), ("nn", 0, 2000, 0), ("fixed2000", 1, 2000, 0), ("fixed300", 1, 300, 1)):
                cases.append(("%s_%d_%d" % (tag, a, b), a, b, fixed, cn, recip, -1, 0))
        cases.append(("few_0_15", 0, 15, 0, 2000, 1, 9, 0))
        cases.append(("const_recip_0_15", 0, 15, 0, 2000, 1, -1, 1))
        for name, a, b, fixed, cn, recip, nt, const in cases:
            t, s = V[a].copy(), V[b]
            if nt >= 0:
                t = t[:nt].copy()
            if const:
                t.view(np.float32).reshape(len(t), 12)[:, 8] = 7.0
            ok, pairs = run_lines(L, t, s, fixed, cn, recip)
            out[name + "_args"] = np.array([a, b, fixed, cn, recip, nt, const], np.int32)
            out[name + "_ok"] = np.array(int(ok), np.int32)
            out[name + "_pairs"] = pairs
            if fixed:
                out[name + "_tied"] = np.array(tied_prefix(t, s, cn), np.int32)
                flagged += int(out[name + "_tied"])
            names.append(name)
            print("%-20s ok %d, %d pairs%s" % (name, ok, len(pairs), ", tied prefix" if fixed and out[name + "_tied"] else ""))
    assert flagged <= 2, "more than 2 of the 4 fixed-number cases have equal neighbours in their sorted prefix: choose other corr_num values"
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "ncc_demo.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
