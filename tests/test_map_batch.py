"""mulls_map_update_batch as the Python side sees it: the three new structures and the symbol of mulls_amd/abi.py and lib.py against include/mulls_hip.h
(a compiled program prints the header's sizes and offsets), the argument order, the field order."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from mulls_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mulls_hip.h")

STRUCTS = {"mulls_map_update_item": "MapUpdateItem", "mulls_map_batch_result": "MapBatchResult", "mulls_map_batch_stats": "MapBatchStats"}


def test_ctypes_layout_matches_header():
    fields = {cname: getattr(abi, pyname) for cname, pyname in STRUCTS.items()}
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "mulls_hip.h"', "int main(void){"]
    for cname, ct in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = {line.split()[0]: line.split()[1:] for line in out if line}
    for cname, ct in fields.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got["%s.%s" % (cname, f)][0]) == getattr(ct, f).offset, (cname, f)


def header_struct_fields(cname):
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (cname, cname), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            names.append(re.search(r"(\w+)\s*(\[\d+\])?\s*$", part.strip()).group(1))
    return names


def test_field_order_matches_header():
    for cname, pyname in STRUCTS.items():
        assert [f for f, _ in getattr(abi, pyname)._fields_] == header_struct_fields(cname), cname
    assert [f for f, _ in abi.MapBatchStats._fields_] == ["n_groups", "n_lockstep", "n_single_path", "n_kernel_launches", "n_syncs"]
    assert [f for f, _ in abi.MapBatchResult._fields_] == ["status", "path", "report"] and dict(abi.MapBatchResult._fields_)["report"] is abi.MapReport
    assert [f for f, _ in abi.MapUpdateItem._fields_] == ["map", "frame_down", "frame_pose_lo", "params"]


def test_argument_order_matches_header():
    text = open(HEADER).read()
    proto = re.search(r"int mulls_map_update_batch\((.*?)\);", text, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    args = [re.sub(r"\s+", " ", a.strip()) for a in proto.split(",")]
    assert args == ["mulls_ctx *ctx", "const mulls_map_update_item *items", "uint32_t n_items", "const mulls_map_params *shared_params", "uint32_t max_lockstep",
                    "mulls_map_batch_result *results", "mulls_map_batch_stats *stats"]
    assert "mulls_map_update_batch" in lib.EXPORTS
    fn = lib.load().mulls_map_update_batch
    P = C.POINTER
    assert list(fn.argtypes) == [C.c_void_p, P(abi.MapUpdateItem), C.c_uint32, P(abi.MapParams), C.c_uint32, P(abi.MapBatchResult), P(abi.MapBatchStats)]
    assert fn.restype is C.c_int


def test_python_entry_point():
    import inspect

    sig = inspect.signature(lib.Context.map_update_batch)
    assert list(sig.parameters)[:5] == ["self", "maps", "frames", "poses", "params"]


# ---- the bridge

from test_ncc import REF_UTILITY  # noqa: E402  (where the reference tree is looked for)

BRIDGE_TU = r"""
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
// MapManager::update_local_map's call of test/mulls_slam.cpp for several streams, next to the single form
bool call(std::vector<std::pair<lo::cloudblock_Ptr, lo::cloudblock_Ptr>> &streams)
{
	bool a = lo::hip::update_local_map(streams[0].first, streams[0].second, 80, 20000, 800, 60, true, "111110", 30.0, 0.3, 3.0, 0.03, true);
	bool b = lo::hip::update_local_map_batch(streams, 80, 20000, 800, 60, true, "111110", 30.0, 0.3, 3.0, 0.03, true);
	bool c = lo::hip::update_local_map_batch(streams);
	return a && b && c;
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_against_the_reference_types():
    """lo::hip::update_local_map_batch on the reference's cloudblock_t, as tests/test_ndt.py checks its bridge: the stand-in headers under oracle/ref_shim
    offer the pcl types, the reference's utility.hpp the block types.  A compile check: running the bridge needs the reference tree and a device together."""
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
