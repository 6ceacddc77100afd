"""Regenerates tests/golden/ncc_demo.npz and tests/golden/ncc_edges.npz: what the reference's own find_feature_correspondence_ncc lines return on the key
points of its demo scans, and on small synthetic key-point sets at the edges of the descriptor arithmetic.

    python tests/golden/make_ncc_golden.py            (needs the reference tree and oracle/_ref/, i.e. __graft_entry__.build() run where the tree exists)
    python tests/golden/make_ncc_golden.py --edges    (ncc_edges.npz only: needs the reference tree alone)

The two demo scans come out of tests/golden/demo_pair.npz (scan_0, scan_15); the reference's extract_semantic_pts (oracle/pyref.py) with
make_demo_pair_golden.extract_params()'s values (ncc_restated.demo_extract_params) leaves their key points (pc_vertex, MULLS_EX_VERTEX: 2840 and 2767 records).  Lines 409-601 of the
reference's include/common/cregistration.hpp are cut into a temporary directory at run time, compiled -O3 -ffp-contract=off inside a class shell against
oracle/ref_shim/shim.hpp, and called for both directions x four modes, plus the two degenerate cases.  Nothing cut or compiled from the reference is kept:
the fixture holds the key-point records and index arrays only.

Fixture contents: kpts_0, kpts_15 ((n, 48) uint8 records); cases (names); per case <name>_args = (target scan, source scan, fixed_num_corr, corr_num,
reciprocal_on, n_target or -1, constant_target_intensity), <name>_ok, <name>_pairs ((n, 2) int32: target, source index in push_back order), and for the
fixed-number cases <name>_tied = 1 when the sorted prefix of corr_num + 1 distances holds two equal neighbours (the order upstream's unstable sort leaves
among them is not defined: such a case may be compared as a set up to the tied entries only).

ncc_edges.npz (edge_sets() below): sets (names); per set <set>_t, <set>_s ((n, 48) uint8 records, at most 700, unique through an index in the x field, the
bytes the descriptor does not read zero); cases (names); per case <name>_args = (index of its set, fixed_num_corr, corr_num, reciprocal_on), <name>_ok,
<name>_pairs, and <name>_tied for the fixed-number cases.  Fixed-number cases exist only for the sets without a NaN distance (a NaN under upstream's std::sort
is undefined behaviour); one whose sorted prefix holds equal neighbours is kept only if the stable order of tests/ncc_restated.py reproduces it exactly.
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


def compact(raw):
    """the five live floats kept, everything else zero, the record's index in its x field: unique records that compress well"""
    f = np.ascontiguousarray(raw).view(np.float32).reshape(len(raw), 12)
    out = np.zeros_like(f)
    out[:, [3, 4, 5, 7, 8]] = f[:, [3, 4, 5, 7, 8]]
    out[:, 0] = np.arange(len(f), dtype=np.float32)
    return out.view(np.uint8).reshape(len(raw), 48)


def edge_sets():
    """-> [(name, target, source, fixed-number corr_nums or ())]: the sets of ncc_edges.npz"""
    kp = lambda seed, n, family="plain": compact(ncc_restated.random_kpts(seed, n, family))
    f32 = lambda raw: raw.view(np.float32).reshape(len(raw), 12)  # a view: writes go to the records
    sets = [("bigcodes", kp(701, 600, "bigcodes"), kp(702, 500, "bigcodes"), (300, 2000)), ("quantised", kp(703, 600, "quantised"), kp(704, 500, "quantised"), ())]
    for tag, at in (("nan_first", (0,)), ("nan_middle", (150,)), ("nan_last", (299,)), ("nan_two", (37, 211))):
        t = kp(710 + len(sets), 300)
        f32(t)[list(at), 8] = np.nan
        sets.append((tag, t, kp(720 + len(sets), 200), ()))
    t = kp(731, 300)
    f32(t)[:, 8] = -1.0 - f32(t)[:, 8]  # every target intensity negative: intensity_max stays 0
    sets.append(("negative", t, kp(732, 200), (300, 2000)))
    t = t.copy()
    f32(t)[0, 8] = np.nan  # ... and behind a NaN no clamp to 0 either: intensity_max is the largest of them, below 0
    sets.append(("nan_negative", t, kp(732, 200), ()))
    s = kp(734, 200)
    f32(s)[::3, 8] += 300.0  # source intensities above and below the target's range
    f32(s)[1::3, 8] -= 300.0
    sets.append(("outside", kp(733, 300), s, (300, 2000)))
    s = kp(736, 40)
    f32(s)[::4, 3] = np.inf  # source heights of +inf (the target has none: no inf - inf)
    sets.append(("inf_height", kp(735, 50), s, (300, 1700)))  # 50 x 30 finite distances: 1700 reaches into the infinite ones
    # one infinite distance, no two equal: heights so far apart that every entry is its own float, and d(5, 7) = |3e38 + 3e38| overflows.  The sorted table
    # is then the same under any sort, +inf its last entry, and corr_num = 144 takes it
    t, s = kp(741, 12), kp(742, 12)
    f32(t)[:, 3] = np.arange(1, 13, dtype=np.float32) * np.float32(1e32)
    f32(s)[:, 3] = np.arange(1, 13, dtype=np.float32) * np.float32(1e35)
    f32(t)[5, 3], f32(s)[7, 3] = 1e37, -1e37
    sets.append(("inf_single", t, s, (143, 144)))
    s = kp(738, 200)
    f32(s)[5::7, 7] = np.nan  # source curvature NaN: whole columns of NaN distances
    sets.append(("nan_source", kp(737, 300), s, ()))
    return sets


def tied(traw, sraw, corr_num):
    """tied_prefix() for tables with infinite entries (inf - inf is no zero)"""
    imin, imax = ncc_restated.intensity_range(ncc_restated.fields(traw)["inten"])
    dt = ncc_restated.table(ncc_restated.descriptors(traw, imin, imax), ncc_restated.descriptors(sraw, imin, imax)).reshape(-1)
    assert not np.isnan(dt).any(), "a fixed-number case on a table with NaN distances"
    s = np.sort(dt)[: corr_num + 1]
    return int((s[1:] == s[:-1]).any())


def edges(L):
    out, set_names, names = {}, [], []
    for k, (sname, t, s, nums) in enumerate(edge_sets()):
        assert len(t) <= 700 and len(s) <= 700 and len({r.tobytes() for r in t}) == len(t) and len({r.tobytes() for r in s}) == len(s)
        out[sname + "_t"], out[sname + "_s"] = t, s
        set_names.append(sname)
        for tag, fixed, cn, recip in [("recip", 0, 2000, 1), ("nn", 0, 2000, 0)] + [("fixed%d" % cn, 1, cn, 0) for cn in nums]:
            name = "%s_%s" % (sname, tag)
            ok, pairs = run_lines(L, t, s, fixed, cn, recip)
            note = ""
            if fixed:
                flag = tied(t, s, cn)
                if flag and not np.array_equal(ncc_restated.restate(t, s, fixed, cn, recip)[1], pairs):
                    print("%-24s tied prefix, and upstream's sort left another order than the stable one: not kept" % name)
                    continue
                out[name + "_tied"] = np.array(flag, np.int32)
                note = ", tied prefix" if flag else ""
            out[name + "_args"] = np.array([k, fixed, cn, recip], np.int32)
            out[name + "_ok"] = np.array(int(ok), np.int32)
            out[name + "_pairs"] = pairs
            names.append(name)
            print("%-24s ok %d, %d pairs%s" % (name, ok, len(pairs), note))
    out["sets"], out["cases"] = np.array(set_names), np.array(names)
    path = os.path.join(HERE, "ncc_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "ncc_demo.npz"))


def main():
    if "--edges" in sys.argv:
        with tempfile.TemporaryDirectory() as tmp:
            L = build_lines(tmp)
            L.ncc_lines.restype = C.c_int
            edges(L)
        return
    from mulls_amd import abi
    from oracle import pyref

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
        edges(L)
    assert flagged <= 2, "more than 2 of the 4 fixed-number cases have equal neighbours in their sorted prefix: choose other corr_num values"
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "ncc_demo.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
