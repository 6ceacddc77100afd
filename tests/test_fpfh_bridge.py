"""The FPFH / SAC-IA bridge (include/cregistration_fpfh_hip.hpp, which include/cregistration_hip.hpp includes) as a compile check on the CPU: inside the
translation unit the other registration bridges are checked in, with the reference's types visible, and alone, with nothing but the stand-in PCL and
Eigen types of oracle/ref_shim.  tests/test_gpu_fpfh.py runs the stand-alone program on a device."""
import os
import subprocess
import tempfile

import pytest

from test_ncc import REF_UTILITY  # noqa: E402  (where the reference tree is looked for)
from test_ndt import BRIDGE_TU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPFH_CALLS = r"""
struct Signature33
{
	float histogram[33];
};
typedef boost::shared_ptr<pcl::PointCloud<Signature33>> fpfhPtr;
// the calls CRegistration::compute_fpfh_feature's and coarse_reg_fpfhsac's bodies would make
double call_fpfh(const pcTPtr &source, const pcTPtr &target, pcTPtr &traned_source, Eigen::Matrix4d &transformationS2T, fpfhPtr &cloud_fpfh, float search_radius)
{
	lo::hip::compute_fpfh_feature<Point_T>(source, cloud_fpfh, search_radius);
	lo::hip::fpfhsac_params().max_correspondence_distance = 0.5f;
	return lo::hip::coarse_reg_fpfhsac<Point_T>(source, target, traned_source, transformationS2T, search_radius);
}
"""


def test_stand_alone_bridge_harness_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "fpfh_bridge_harness.cpp")])


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (cloudblock_t, constraint_t: what the bridge header expects to be visible) is not here")
def test_bridge_compiles_against_the_reference_types():
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 592, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(BRIDGE_TU + FPFH_CALLS)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
