"""Build libmulls_hip.so (hand-written HIP kernels + host driver) for gfx950 with hipcc, in-tree.

    python -m mulls_amd.build            # incremental
    python -m mulls_amd.build --force

hipcc cross-compiles without a GPU.  The flags matter for parity: -ffp-contract=off keeps every float/double
expression free of FMA contraction (the reference is built -O3 without -march, CMakeLists.txt:43).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmulls_hip.so")
SOURCES = ["k_setup.hip", "k_grid.hip", "k_search.hip", "k_reduce.hip", "k_ground.hip", "k_ground_normals.hip", "k_classify.hip", "map_kernels.hip", "k_map_batch.hip", "k_ncc_batch.hip", "k_pair_gather.hip", "k_ransac.hip", "k_teaser.hip", "k_teaser_clique.hip", "k_sor.hip", "k_nms.hip", "k_scan.hip", "k_image.hip", "k_pgo.hip", "k_submaps.hip", "k_ndt.hip", "k_gicp.hip", "k_pcl_icp.hip", "k_reg_table.hip", "k_fpfh.hip", "k_fpfh_batch.hip", "k_extract_batch.hip", "driver.cpp", "batch.cpp", "loop.cpp", "variants.cpp", "stage.cpp", "shard.cpp", "map.cpp", "map_batch.cpp", "ground.cpp", "classify.cpp", "extract_batch.cpp", "io.cpp", "ncc.cpp", "pair_stage.cpp", "ransac.cpp", "teaser.cpp", "sor.cpp", "nms.cpp", "scan.cpp", "image.cpp", "pgo.cpp", "submaps.cpp", "ndt.cpp", "gicp.cpp", "pcl_icp.cpp", "reg_host.cpp", "fpfh.cpp"]
DEPS = ["device_types.h", "device_util.h", "lds_tier.h", "big_tier.h", "crop_grid.h", "solve_wave.h", "detmath.h", "accum.h", "icp_step.h", "launch.h", "map_launch.h", "map_internal.h", "classify_launch.h", "ground_launch.h", "ncc_launch.h", "ncc_device.h", "ncc_batch.h", "pair_gather.h", "pair_stage.h", "ransac_launch.h", "ransac_math.h", "ransac_host.h", "ransac_batch.h", "teaser_launch.h", "teaser_math.h", "teaser_host.h", "teaser_search.h", "teaser_batch.h", "sor_launch.h", "sor_math.h", "nms_launch.h", "nms_host.h", "nms_batch.h", "scan_launch.h", "scan_math.h", "scan_host.h", "image_launch.h", "image_math.h", "pgo_launch.h", "pgo_math.h", "ndt_launch.h", "ndt_math.h", "gicp_launch.h", "gicp_math.h", "pcl_icp_launch.h", "pcl_icp_math.h", "fpfh_launch.h", "fpfh_device.h", "fpfh_batch.h", "fpfh_math.h", "reg_table.h", "reg_device.h", "reg_launch.h", "reg_host.h", "jacobi_rot.h", "submaps_launch.h", "submaps_host.h", "rounds.h", "extract_batch.h", "subbatch.h", "extract_internal.h", "extract_launch.h", "pca_device.h", "ctx.h", "batch.h", "hostmath.h", os.path.join("..", "..", "include", "mulls_hip.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function"]


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    for f in SOURCES + DEPS + [os.path.join("..", "build.py")]:
        if os.path.getmtime(os.path.join(CSRC, f)) > t:
            return True
    return False


def build(force=False, verbose=False):
    if not force and not needs_build():
        return LIB
    objs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src + ".o")
        cmd = [hipcc()] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        objs.append(obj)
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-fopenmp", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
