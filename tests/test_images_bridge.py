"""The bridge of the pictures of a cloud (include/cregistration_hip.hpp: lo::hip::get_cloud_cpt, generate_2d_map, pointcloud_to_rangeimage) as a compile check
on the CPU, inside the translation unit the other bridges are checked in: the stand-in PCL and Eigen types of oracle/ref_shim, the reference's utility.hpp
for centerpoint_t and the block types.  Once as the project is built (no OpenCV: the std::vector forms only), once with OPENCV_ON and a stand-in cv::Mat,
for the overloads with upstream's verbatim signatures.  tests/test_gpu_images.py runs the entry points behind them on a device."""
import os
import subprocess
import tempfile

import pytest

from test_ncc import REF_UTILITY  # noqa: E402  (where the reference tree is looked for)
from test_ndt import BRIDGE_TU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_CALLS = r"""
// the calls of test/mulls_slam.cpp:722-733 and :1016-1025, on vectors
int call_images(pcTPtr &pc_raw, pcTPtr &pc_map_merged, mulls_mapper *mapper)
{
	lo::centerpoint_t cpt;
	lo::hip::get_cloud_cpt<Point_T>(pc_raw, cpt);
	std::vector<uint8_t> range_image, bev, map_2d, map_2d_resident;
	int width = 0, height = 0;
	bool ok = lo::hip::pointcloud_to_rangeimage<Point_T>(pc_raw, range_image, width, height);
	lo::hip::generate_2d_map<Point_T>(pc_raw, bev, 4, 400, 400, 2, 50, -5.0, 15.0);
	lo::hip::generate_2d_map<Point_T>(pc_map_merged, map_2d, 1, 1920, 1080, 20, 1000, -FLT_MAX, FLT_MAX, true);
	mulls_cloud resident;
	mulls_mapper_cloud(lo::hip::thread_context(), mapper, &resident);
	lo::hip::image_2d_of_cloud(resident, map_2d_resident, 1, 1920, 1080, 20, 1000, -FLT_MAX, FLT_MAX, true);
	return (int)ok + mulls_io_write_pgm("merged_map_2d.pgm", map_2d.data(), 1920, 1080) + (int)(cpt.x + cpt.y + cpt.z) + width + height;
}
"""
CV_STAND_IN = r"""
#define OPENCV_ON 1
#define CV_8UC1 0
namespace cv
{
struct Mat
{
	Mat() {}
	Mat(int rows, int cols, int type, void *data) {}
	Mat clone() const { return *this; }
};
} // namespace cv
"""
CV_CALLS = r"""
// ... and with upstream's verbatim signatures
int call_images_cv(pcTPtr &pc_raw, pcTPtr &pc_map_merged)
{
	cv::Mat ri_temp, map_2d;
	bool ok = lo::hip::pointcloud_to_rangeimage<Point_T>(pc_raw, ri_temp);
	cv::Mat bev = lo::hip::generate_2d_map<Point_T>(pc_raw, 4, 400, 400, 2, 50, -5.0, 15.0);
	map_2d = lo::hip::generate_2d_map<Point_T>(pc_map_merged, 1, 1920, 1080, 20, 1000, -FLT_MAX, FLT_MAX, true);
	return (int)ok;
}
"""


@pytest.mark.skipif(not os.path.exists(REF_UTILITY), reason="the reference's utility.hpp (centerpoint_t, cloudblock_t: what the bridge header expects to be visible) is not here")
@pytest.mark.parametrize("opencv", [False, True], ids=["vectors", "cv_mat"])
def test_bridge_compiles_with_the_reference_calls(opencv):
    lines = open(REF_UTILITY, errors="replace").read().split("\n")

    def cut(first, last, expect):
        assert expect in lines[first - 1], (first, expect)
        return "\n".join(lines[first - 1:last]) + "\n"

    include = '#include "cregistration_hip.hpp"'
    assert BRIDGE_TU.count(include) == 1
    tu = "#include <cfloat>\n" + BRIDGE_TU.replace(include, (CV_STAND_IN if opencv else "") + include) + IMAGE_CALLS + (CV_CALLS if opencv else "")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "util_typedefs.inc"), "w").write(cut(84, 85, "typedef Eigen::Matrix<double, 6, 1> Vector6d"))
        open(os.path.join(d, "util_types.inc"), "w").write(cut(92, 157, "struct centerpoint_t") + cut(233, 558, "struct cloudblock_t") + cut(561, 592, "struct constraint_t"))
        open(os.path.join(d, "tu.cpp"), "w").write(tu)
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I", d, "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "tu.cpp")])
