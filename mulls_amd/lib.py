"""Python host-side binding of libmulls_hip.so (the C ABI in include/mulls_hip.h).

This is plumbing for the tests, bench.py and smoke(): it loads the in-tree shared library with ctypes and forwards
calls.  There is deliberately NO fallback: if the HIP library is missing or no gfx950 device is usable, every call
raises.  The product for C++ callers is the library itself plus include/cregistration_hip.hpp.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmulls_hip.so")
LIB_PATH = os.environ.get("MULLS_HIP_LIB", LIB_PATH)  # A/B timing of two builds of the same library on one box (tools/)
_LIB = None


class MullsError(RuntimeError):
    pass


def load():
    """Load libmulls_hip.so (raises if it has not been built: run `python -m mulls_amd.build`)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise MullsError("libmulls_hip.so is not built (python -m mulls_amd.build); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.mulls_default_params.argtypes = [C.POINTER(abi.Params)]
    lib.mulls_default_params.restype = None
    lib.mulls_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.mulls_destroy.argtypes = [vp]
    lib.mulls_destroy.restype = None
    lib.mulls_last_error.argtypes = [vp]
    lib.mulls_last_error.restype = C.c_char_p
    lib.mulls_set_profiling.argtypes = [vp, C.c_int]
    lib.mulls_get_profile.argtypes = [vp, C.POINTER(abi.Profile)]
    lib.mulls_set_nn_mode.argtypes = [vp, C.c_int]
    lib.mulls_set_option.argtypes = [vp, C.c_int, C.c_double]
    lib.mulls_get_option.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    lib.mulls_stream.argtypes = [vp]
    lib.mulls_stream.restype = vp
    lib.mulls_icp.argtypes = [vp, C.POINTER(abi.Pair), C.POINTER(abi.Params), C.POINTER(abi.Result)]
    lib.mulls_icp_batch.argtypes = [vp, C.POINTER(abi.Pair), C.c_int, C.POINTER(abi.Params), C.POINTER(abi.Result)]
    lib.mulls_pack_results.argtypes = [C.POINTER(abi.Result), C.c_int, C.c_void_p]
    lib.mulls_pack_results.restype = None
    lib.mulls_icp_batch_sharded.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(abi.Pair), C.c_int, C.POINTER(abi.Params), C.POINTER(abi.Result)]
    lib.mulls_pipe_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    lib.mulls_pipe_destroy.argtypes = [vp]
    lib.mulls_pipe_destroy.restype = None
    lib.mulls_pipe_depth.argtypes = [vp]
    lib.mulls_pipe_ctx.argtypes = [vp, C.c_int]
    lib.mulls_pipe_ctx.restype = vp
    lib.mulls_pipe_set_option.argtypes = [vp, C.c_int, C.c_double]
    lib.mulls_icp_batch_begin.argtypes = [vp, C.POINTER(abi.Pair), C.c_int, C.POINTER(abi.Params), C.POINTER(abi.Result)]
    lib.mulls_icp_batch_end.argtypes = [vp, C.c_int]
    lib.mulls_batch_create.argtypes = [vp, C.POINTER(abi.Pair), C.c_int, C.POINTER(vp)]
    lib.mulls_batch_run.argtypes = [vp, vp, C.POINTER(abi.Params), C.POINTER(abi.Result)]
    lib.mulls_batch_destroy.argtypes = [vp, vp]
    lib.mulls_batch_destroy.restype = None
    lib.mulls_icp_3dof_ground.argtypes = [vp, C.POINTER(abi.Pair), C.POINTER(abi.Params), C.POINTER(abi.Result)]
    lib.mulls_icp_3dof_ground_batch.argtypes = [vp, C.POINTER(abi.Pair), C.c_int, C.POINTER(abi.Params), C.POINTER(abi.Result)]
    lib.mulls_icp_4dof_global.argtypes = [vp, C.POINTER(abi.Pair), C.c_float, C.POINTER(C.c_double), C.c_int, C.c_float, C.c_float, C.c_float,
                                          C.c_float, C.c_float, C.c_float, C.POINTER(abi.Result), C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.mulls_stage_transform.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    lib.mulls_stage_correspond.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.Cloud), C.c_float, C.c_int, C.c_float, vp, vp, vp]
    lib.mulls_stage_accumulate.argtypes = [vp, C.c_int, C.POINTER(abi.Cloud), C.POINTER(abi.Cloud), vp, vp, vp, C.c_uint32, C.c_int,
                                           C.c_float, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]
    lib.mulls_map_default_params.argtypes = [C.POINTER(abi.MapParams)]
    lib.mulls_map_default_params.restype = None
    lib.mulls_map_create.argtypes = [vp, C.POINTER(vp)]
    lib.mulls_map_destroy.argtypes = [vp, vp]
    lib.mulls_map_destroy.restype = None
    lib.mulls_map_set.argtypes = [vp, vp, C.POINTER(abi.Cloud), C.POINTER(C.c_double)]
    lib.mulls_map_update.argtypes = [vp, vp, C.POINTER(abi.Cloud), C.POINTER(C.c_double), C.POINTER(abi.MapParams), C.POINTER(abi.MapReport)]
    lib.mulls_map_update_batch.argtypes = [vp, C.POINTER(abi.MapUpdateItem), C.c_uint32, C.POINTER(abi.MapParams), C.c_uint32, C.POINTER(abi.MapBatchResult),
                                           C.POINTER(abi.MapBatchStats)]
    lib.mulls_map_cloud.argtypes = [vp, vp, C.c_int, C.POINTER(abi.Cloud)]
    lib.mulls_map_pose.argtypes = [vp, vp, C.POINTER(C.c_double)]
    lib.mulls_map_download.argtypes = [vp, vp, C.c_int, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_map_frame_download.argtypes = [vp, vp, C.c_int, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_ground_default_params.argtypes = [C.POINTER(abi.GroundParams)]
    lib.mulls_ground_default_params.restype = None
    lib.mulls_ground_filter.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(abi.GroundParams), vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32,
                                        C.POINTER(C.c_uint32)]
    lib.mulls_classify_default_params.argtypes = [C.POINTER(abi.ClassifyParams)]
    lib.mulls_classify_default_params.restype = None
    lib.mulls_classify_nground.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(abi.ClassifyParams), C.POINTER(vp), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint32), vp, C.POINTER(C.c_uint32)]
    lib.mulls_extract_default_params.argtypes = [C.POINTER(abi.ExtractParams)]
    lib.mulls_extract_default_params.restype = None
    lib.mulls_extract_features.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(abi.ExtractParams), C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.mulls_block_create.argtypes = [vp, C.POINTER(vp)]
    lib.mulls_block_destroy.argtypes = [vp, vp]
    lib.mulls_block_destroy.restype = None
    lib.mulls_extract_features_resident.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(abi.ExtractParams), vp, C.POINTER(C.c_uint32)]
    lib.mulls_extract_features_batch.argtypes = [vp, C.POINTER(abi.Cloud), C.c_uint32, C.POINTER(abi.ExtractParams), C.POINTER(vp), C.c_uint64,
                                                 C.POINTER(abi.ExtractBatchResult), C.POINTER(abi.ExtractBatchStats)]
    lib.mulls_block_cloud.argtypes = [vp, vp, C.c_int, C.POINTER(abi.Cloud)]
    lib.mulls_block_download.argtypes = [vp, vp, C.c_int, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_motion_compensate.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_float]
    lib.mulls_block_motion_compensate.argtypes = [vp, vp, C.POINTER(C.c_double), C.c_int]
    lib.mulls_voxel_downsample.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_float, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_ncc_default_params.argtypes = [C.POINTER(abi.NccParams)]
    lib.mulls_ncc_default_params.restype = None
    lib.mulls_ncc_correspond.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.Cloud), C.POINTER(abi.NccParams), vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_ncc_correspond_batch.argtypes = [vp, C.POINTER(abi.NccProblem), C.c_uint32, C.POINTER(abi.NccParams), C.c_uint64, C.POINTER(abi.NccResult)]
    lib.mulls_ransac_default_params.argtypes = [C.POINTER(abi.RansacParams)]
    lib.mulls_ransac_default_params.restype = None
    lib.mulls_coarse_reg_ransac.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.Cloud), C.POINTER(abi.RansacParams), C.POINTER(abi.RansacResult), vp, C.c_uint32]
    lib.mulls_coarse_reg_ransac_indexed.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.Cloud), vp, vp, C.c_uint32, C.POINTER(abi.RansacParams),
                                                    C.POINTER(abi.RansacResult), vp, C.c_uint32]
    lib.mulls_coarse_reg_ransac_batch.argtypes = [vp, C.POINTER(abi.RansacProblem), C.c_uint32, C.POINTER(abi.RansacParams), C.c_uint64, C.POINTER(abi.RansacResult)]
    lib.mulls_teaser_default_params.argtypes = [C.POINTER(abi.TeaserParams)]
    lib.mulls_teaser_default_params.restype = None
    lib.mulls_coarse_reg_teaser.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.Cloud), C.POINTER(abi.TeaserParams), C.POINTER(abi.TeaserResult), vp, C.c_uint32]
    lib.mulls_coarse_reg_teaser_indexed.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.Cloud), vp, vp, C.c_uint32, C.POINTER(abi.TeaserParams),
                                                    C.POINTER(abi.TeaserResult), vp, C.c_uint32]
    lib.mulls_coarse_reg_teaser_batch.argtypes = [vp, C.POINTER(abi.TeaserProblem), C.c_uint32, C.POINTER(abi.TeaserParams), C.c_uint64, C.POINTER(abi.TeaserResult)]
    lib.mulls_pgo_default_params.argtypes = [C.POINTER(abi.PgoParams)]
    lib.mulls_pgo_default_params.restype = None
    lib.mulls_pgo_optimize.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.POINTER(abi.PgoParams), vp, vp, C.POINTER(abi.PgoResult)]
    lib.mulls_pgo_optimize_batch.argtypes = [vp, C.POINTER(abi.PgoProblem), C.c_uint32, C.POINTER(abi.PgoParams), C.c_uint64, C.POINTER(abi.PgoResult)]
    lib.mulls_ndt_default_params.argtypes = [C.POINTER(abi.NdtParams)]
    lib.mulls_ndt_default_params.restype = None
    lib.mulls_ndt.argtypes = [vp, C.POINTER(abi.NdtProblem), C.POINTER(abi.NdtParams), C.POINTER(abi.NdtResult)]
    lib.mulls_ndt_batch.argtypes = [vp, C.POINTER(abi.NdtProblem), C.c_uint32, C.POINTER(abi.NdtParams), C.POINTER(abi.NdtResult)]
    lib.mulls_gicp_default_params.argtypes = [C.POINTER(abi.GicpParams)]
    lib.mulls_gicp_default_params.restype = None
    lib.mulls_gicp.argtypes = [vp, C.POINTER(abi.GicpProblem), C.POINTER(abi.GicpParams), C.POINTER(abi.GicpResult)]
    lib.mulls_gicp_batch.argtypes = [vp, C.POINTER(abi.GicpProblem), C.c_uint32, C.POINTER(abi.GicpParams), C.POINTER(abi.GicpResult)]
    lib.mulls_pcl_icp_default_params.argtypes = [C.POINTER(abi.PclIcpParams)]
    lib.mulls_pcl_icp_default_params.restype = None
    lib.mulls_pcl_icp.argtypes = [vp, C.POINTER(abi.PclIcpProblem), C.POINTER(abi.PclIcpParams), C.POINTER(abi.PclIcpResult)]
    lib.mulls_pcl_icp_batch.argtypes = [vp, C.POINTER(abi.PclIcpProblem), C.c_uint32, C.POINTER(abi.PclIcpParams), C.POINTER(abi.PclIcpResult)]
    lib.mulls_fpfh_default_params.argtypes = [C.POINTER(abi.FpfhParams)]
    lib.mulls_fpfh_default_params.restype = None
    lib.mulls_fpfh.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.FpfhParams), vp, vp]
    lib.mulls_fpfhsac_default_params.argtypes = [C.POINTER(abi.FpfhSacParams)]
    lib.mulls_fpfhsac_default_params.restype = None
    lib.mulls_coarse_reg_fpfhsac.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.Cloud), C.POINTER(abi.FpfhSacParams), C.POINTER(abi.FpfhSacResult)]
    lib.mulls_compute_fpfh_batch.argtypes = [vp, C.POINTER(abi.Cloud), C.c_uint32, C.POINTER(abi.FpfhParams), C.POINTER(vp), C.POINTER(vp), C.c_uint64]
    lib.mulls_coarse_reg_fpfhsac_batch.argtypes = [vp, C.POINTER(abi.FpfhSacProblem), C.c_uint32, C.POINTER(abi.FpfhSacParams), C.c_uint64,
                                                   C.POINTER(abi.FpfhSacResult)]
    lib.mulls_sor_default_params.argtypes = [C.POINTER(abi.SorParams)]
    lib.mulls_sor_default_params.restype = None
    lib.mulls_sor_filter.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.SorParams), vp, C.c_uint32, C.POINTER(C.c_uint32), vp, C.c_uint32, vp,
                                     C.POINTER(abi.SorReport)]
    lib.mulls_nms_default_params.argtypes = [C.POINTER(abi.NmsParams)]
    lib.mulls_nms_default_params.restype = None
    lib.mulls_non_max_suppress.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.NmsParams), vp, C.c_uint32, C.POINTER(C.c_uint32), vp, C.c_uint32, vp,
                                           C.POINTER(abi.NmsReport)]
    lib.mulls_non_max_suppress_batch.argtypes = [vp, C.POINTER(abi.NmsProblem), C.c_uint32, C.POINTER(abi.NmsParams), C.c_uint64, C.POINTER(abi.NmsReport)]
    lib.mulls_nms_batch_arena_bytes.argtypes = [vp]
    lib.mulls_nms_batch_arena_bytes.restype = C.c_uint64
    lib.mulls_scan_prep_default_params.argtypes = [C.POINTER(abi.ScanPrepParams)]
    lib.mulls_scan_prep_default_params.restype = None
    lib.mulls_scan_prepare.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(abi.ScanPrepParams), C.POINTER(C.c_uint32), C.POINTER(abi.ScanPrepReport)]
    lib.mulls_mapper_create.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    lib.mulls_mapper_destroy.argtypes = [vp, vp]
    lib.mulls_mapper_destroy.restype = None
    lib.mulls_mapper_add.argtypes = [vp, vp, C.POINTER(abi.MapperFrame), C.c_uint32, C.POINTER(abi.ScanPrepParams), C.POINTER(C.c_uint32), C.POINTER(abi.MapperReport)]
    lib.mulls_mapper_cloud.argtypes = [vp, vp, C.POINTER(abi.Cloud)]
    lib.mulls_mapper_download.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_mapper_clear.argtypes = [vp, vp]
    lib.mulls_image2d_default_params.argtypes = [C.POINTER(abi.Image2dParams)]
    lib.mulls_image2d_default_params.restype = None
    lib.mulls_range_image_default_params.argtypes = [C.POINTER(abi.RangeImageParams)]
    lib.mulls_range_image_default_params.restype = None
    lib.mulls_cloud_centre.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(C.c_double)]
    lib.mulls_map_image_2d.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.Image2dParams), vp, vp, C.POINTER(abi.Image2dReport)]
    lib.mulls_range_image.argtypes = [vp, C.POINTER(abi.Cloud), C.POINTER(abi.RangeImageParams), vp]
    lib.mulls_scan_images_batch.argtypes = [vp, C.POINTER(abi.Cloud), C.c_uint32, C.POINTER(abi.RangeImageParams), C.POINTER(abi.Image2dParams), C.POINTER(vp),
                                            C.POINTER(vp), C.POINTER(abi.Image2dReport)]
    lib.mulls_io_write_pgm.argtypes = [C.c_char_p, vp, C.c_int32, C.c_int32]
    lib.mulls_overlap_default_params.argtypes = [C.POINTER(abi.OverlapParams)]
    lib.mulls_overlap_default_params.restype = None
    lib.mulls_submaps_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    lib.mulls_submaps_destroy.argtypes = [vp, vp]
    lib.mulls_submaps_destroy.restype = None
    lib.mulls_submaps_push.argtypes = [vp, vp, C.POINTER(abi.Cloud), C.POINTER(C.c_double), C.c_int32, C.c_float, C.POINTER(abi.SubmapInfo)]
    lib.mulls_submaps_push_map.argtypes = [vp, vp, vp, C.c_int32, C.c_float, C.POINTER(abi.SubmapInfo)]
    lib.mulls_submaps_count.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.mulls_submaps_info.argtypes = [vp, vp, C.c_uint32, C.POINTER(abi.SubmapInfo)]
    lib.mulls_submaps_cloud.argtypes = [vp, vp, C.c_uint32, C.c_int, C.POINTER(abi.Cloud)]
    lib.mulls_submaps_download.argtypes = [vp, vp, C.c_uint32, C.c_int, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_submaps_clear.argtypes = [vp, vp]
    lib.mulls_submaps_set_poses.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_int]
    lib.mulls_submaps_find_overlap.argtypes = [vp, vp, C.c_uint32, C.POINTER(abi.OverlapParams), C.POINTER(abi.SubmapEdge), C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_submaps_pairs.argtypes = [vp, vp, C.POINTER(abi.SubmapEdge), C.c_uint32, C.POINTER(abi.Pair)]
    lib.mulls_io_read_kitti_bin.argtypes = [C.c_char_p, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_io_read_pcd.argtypes = [C.c_char_p, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mulls_io_write_pcd.argtypes = [C.c_char_p, vp, C.c_uint32, C.c_uint32, C.c_int]
    lib.mulls_io_write_pose.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.c_int]
    _LIB = lib
    return lib


EXPORTS = [
    "mulls_default_params", "mulls_create", "mulls_destroy", "mulls_last_error", "mulls_set_profiling", "mulls_get_profile",
    "mulls_stream", "mulls_set_nn_mode", "mulls_icp", "mulls_icp_batch", "mulls_batch_create", "mulls_batch_run", "mulls_batch_destroy",
    "mulls_stage_transform", "mulls_stage_correspond", "mulls_stage_accumulate", "mulls_icp_3dof_ground", "mulls_icp_3dof_ground_batch",
    "mulls_icp_4dof_global", "mulls_map_default_params", "mulls_map_create", "mulls_map_destroy", "mulls_map_set", "mulls_map_update", "mulls_map_update_batch",
    "mulls_map_cloud", "mulls_map_pose", "mulls_map_download", "mulls_map_frame_download", "mulls_io_read_kitti_bin", "mulls_io_read_pcd",
    "mulls_io_write_pcd", "mulls_io_write_pose", "mulls_ground_default_params", "mulls_ground_filter",
    "mulls_classify_default_params", "mulls_classify_nground", "mulls_extract_default_params", "mulls_extract_features", "mulls_voxel_downsample",
    "mulls_set_option", "mulls_get_option", "mulls_block_create", "mulls_block_destroy", "mulls_extract_features_resident", "mulls_extract_features_batch", "mulls_block_cloud", "mulls_block_download",
    "mulls_motion_compensate", "mulls_block_motion_compensate",
    "mulls_pack_results", "mulls_icp_batch_sharded", "mulls_pipe_create", "mulls_pipe_destroy", "mulls_pipe_depth", "mulls_pipe_ctx", "mulls_pipe_set_option", "mulls_icp_batch_begin", "mulls_icp_batch_end",
    "mulls_ncc_default_params", "mulls_ncc_correspond", "mulls_ncc_correspond_batch",
    "mulls_ransac_default_params", "mulls_coarse_reg_ransac", "mulls_coarse_reg_ransac_indexed", "mulls_coarse_reg_ransac_batch",
    "mulls_teaser_default_params", "mulls_coarse_reg_teaser", "mulls_coarse_reg_teaser_indexed", "mulls_coarse_reg_teaser_batch",
    "mulls_sor_default_params", "mulls_sor_filter",
    "mulls_pgo_default_params", "mulls_pgo_optimize", "mulls_pgo_optimize_batch",
    "mulls_ndt_default_params", "mulls_ndt", "mulls_ndt_batch", "mulls_gicp_default_params", "mulls_gicp", "mulls_gicp_batch",
    "mulls_pcl_icp_default_params", "mulls_pcl_icp", "mulls_pcl_icp_batch",
    "mulls_fpfh_default_params", "mulls_fpfh", "mulls_fpfhsac_default_params", "mulls_coarse_reg_fpfhsac",
    "mulls_compute_fpfh_batch", "mulls_coarse_reg_fpfhsac_batch",
    "mulls_nms_default_params", "mulls_non_max_suppress", "mulls_non_max_suppress_batch", "mulls_nms_batch_arena_bytes",
    "mulls_scan_prep_default_params", "mulls_scan_prepare",
    "mulls_mapper_create", "mulls_mapper_destroy", "mulls_mapper_add", "mulls_mapper_cloud", "mulls_mapper_download", "mulls_mapper_clear",
    "mulls_image2d_default_params", "mulls_range_image_default_params", "mulls_cloud_centre", "mulls_map_image_2d", "mulls_range_image",
    "mulls_scan_images_batch", "mulls_io_write_pgm",
    "mulls_overlap_default_params", "mulls_submaps_create", "mulls_submaps_destroy", "mulls_submaps_push", "mulls_submaps_push_map", "mulls_submaps_count",
    "mulls_submaps_info", "mulls_submaps_cloud", "mulls_submaps_download", "mulls_submaps_clear", "mulls_submaps_set_poses", "mulls_submaps_find_overlap",
    "mulls_submaps_pairs",
]


def _read(fn, name, path):
    n = C.c_uint32(0)
    rc = fn(path.encode(), None, 0, C.byref(n))
    if rc != 0:
        raise MullsError("%s(%s) failed with %d" % (name, path, rc))
    out = np.zeros(n.value, abi.POINT_DTYPE)
    if n.value:
        rc = fn(path.encode(), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
        if rc != 0:
            raise MullsError("%s(%s) failed with %d" % (name, path, rc))
    return out


def read_kitti_bin(path):
    """DataIo::read_bin_file: KITTI .bin -> POINT_DTYPE array (intensity * 255, trailing zero point like the reference)."""
    return _read(load().mulls_io_read_kitti_bin, "mulls_io_read_kitti_bin", path)


def read_pcd(path):
    """DataIo::read_pcd_file: PCD v0.7 (ascii / binary) of PointXYZINormal -> POINT_DTYPE array."""
    return _read(load().mulls_io_read_pcd, "mulls_io_read_pcd", path)


def write_pcd(path, pts, binary=True):
    pts = abi.as_points(pts)
    rc = load().mulls_io_write_pcd(path.encode(), pts.ctypes.data_as(C.c_void_p), len(pts), abi.POINT_BYTES, int(binary))
    if rc != 0:
        raise MullsError("mulls_io_write_pcd(%s) failed with %d" % (path, rc))


def write_pose(path, T, append=False):
    rc = load().mulls_io_write_pose(path.encode(), abi.colmajor16(T), int(append))
    if rc != 0:
        raise MullsError("mulls_io_write_pose(%s) failed with %d" % (path, rc))


def write_pgm(path, image):
    """mulls_io_write_pgm: a (height, width) uint8 image as a binary PGM"""
    image = np.ascontiguousarray(image, np.uint8)
    rc = load().mulls_io_write_pgm(path.encode(), image.ctypes.data_as(C.c_void_p), image.shape[1], image.shape[0])
    if rc != 0:
        raise MullsError("mulls_io_write_pgm(%s) failed with %d" % (path, rc), rc)


def icp_batch_sharded(contexts, pairs, params, marshalled=None):
    """mulls_icp_batch_sharded: the pairs block-partitioned over `contexts` (Context objects: one per GPU, or several on one), one host thread each."""
    lib = load()
    arr, res = marshalled if marshalled is not None else (abi.make_pair_array(pairs), abi.make_result_array(len(pairs)))
    hs = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    rc = lib.mulls_icp_batch_sharded(hs, len(contexts), arr, len(pairs), C.byref(params), res)
    if rc != 0:
        raise MullsError("mulls_icp_batch_sharded failed with %d: %s" % (rc, "; ".join((lib.mulls_last_error(c.h) or b"").decode() for c in contexts)))
    return res


class Pipe:
    """mulls_pipe: mulls_icp_batch calls from host buffers in flight on alternating contexts of one device (begin / end by ticket)."""

    def __init__(self, device=0, depth=2):
        self.lib = load()
        self.h = C.c_void_p()
        rc = self.lib.mulls_pipe_create(device, depth, C.byref(self.h))
        if rc != 0:
            raise MullsError("mulls_pipe_create(device=%d, depth=%d) failed with %d" % (device, depth, rc))
        self._keep = {}

    def set_option(self, option, value):
        rc = self.lib.mulls_pipe_set_option(self.h, option, float(value))
        if rc != 0:
            raise MullsError("mulls_pipe_set_option failed with %d" % rc)

    def begin(self, pairs, params, marshalled=None):
        """-> ticket; the marshalled arrays (and through them the clouds) are kept alive until end(ticket)"""
        arr, res = marshalled if marshalled is not None else (abi.make_pair_array(pairs), abi.make_result_array(len(pairs)))
        t = self.lib.mulls_icp_batch_begin(self.h, arr, len(pairs), C.byref(params), res)
        if t < 0:
            raise MullsError("mulls_icp_batch_begin failed with %d" % t)
        self._keep[t] = (arr, res, pairs, params)
        return t

    def end(self, ticket):
        rc = self.lib.mulls_icp_batch_end(self.h, ticket)
        arr, res, _, _ = self._keep.pop(ticket)
        if rc != 0:
            lane = ticket % self.lib.mulls_pipe_depth(self.h)
            raise MullsError("mulls_icp_batch_end(%d) failed with %d: %s" % (ticket, rc, (self.lib.mulls_last_error(self.lib.mulls_pipe_ctx(self.h, lane)) or b"").decode()))
        return res

    def lane_profile(self, lane):
        """mulls_profile of one lane's context (its latest call)"""
        pf = abi.Profile()
        self.lib.mulls_get_profile(self.lib.mulls_pipe_ctx(self.h, lane), C.byref(pf))
        return pf

    def close(self):
        if self.h:
            self.lib.mulls_pipe_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """mulls_ctx: one HIP stream on one device."""

    def __init__(self, device=0):
        self.lib = load()
        self.h = C.c_void_p()
        rc = self.lib.mulls_create(device, C.byref(self.h))
        if rc != 0:
            raise MullsError("mulls_create(device=%d) failed with %d (no usable gfx950 device?)" % (device, rc))

    def close(self):
        if self.h:
            self.lib.mulls_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise MullsError("%s failed with %d: %s" % (what, rc, self.lib.mulls_last_error(self.h).decode()))

    def set_profiling(self, on):
        self._check(self.lib.mulls_set_profiling(self.h, int(on)), "mulls_set_profiling")

    def set_nn_mode(self, mode):
        """0 auto, 1 LDS-tiled brute force, 2 uniform grid in global memory, 3 uniform grid staged in LDS (lock-step), 4 the same as 3."""
        self._check(self.lib.mulls_set_nn_mode(self.h, int(mode)), "mulls_set_nn_mode")

    def set_option(self, option, value):
        """enum mulls_option (abi.OPT_*): execution options of the context; none of them changes a result."""
        self._check(self.lib.mulls_set_option(self.h, int(option), float(value)), "mulls_set_option")

    def get_option(self, option):
        v = C.c_double(0)
        self._check(self.lib.mulls_get_option(self.h, int(option), C.byref(v)), "mulls_get_option")
        return v.value

    def profile(self):
        p = abi.Profile()
        self._check(self.lib.mulls_get_profile(self.h, C.byref(p)), "mulls_get_profile")
        return p

    def stream(self):
        return self.lib.mulls_stream(self.h)

    # --- mm_lls_icp replacements -------------------------------------------------------------------------------
    def icp(self, pair, params, trace_cap=0):
        res = abi.make_result_array(1, trace_cap)
        p = pair.as_pair()
        self._check(self.lib.mulls_icp(self.h, C.byref(p), C.byref(params), res), "mulls_icp")
        return res

    def icp_batch(self, pairs, params, trace_cap=0, marshalled=None):
        """mulls_icp_batch.  marshalled: (the mulls_pair array of `pairs`, a result array) made earlier — callers timing the library leave the
        Python-side marshalling out that way; last_call_s = seconds spent inside the C call."""
        arr, res = marshalled if marshalled is not None else (abi.make_pair_array(pairs), abi.make_result_array(len(pairs), trace_cap))
        import time

        t0 = time.perf_counter()
        rc = self.lib.mulls_icp_batch(self.h, arr, len(pairs), C.byref(params), res)
        self.last_call_s = time.perf_counter() - t0
        self._check(rc, "mulls_icp_batch")
        return res

    def batch(self, pairs):
        return Batch(self, pairs)

    def block(self):
        """an empty device-resident feature block (Block.extract fills it)"""
        return Block(self)

    def local_map(self, clouds=None, pose=None):
        """Device-resident local map (mulls_map_*), optionally initialised from six host class clouds and a pose_lo."""
        return LocalMap(self, clouds, pose)

    # --- variants ------------------------------------------------------------------------------------
    def icp_3dof_ground(self, pairs, params, trace_cap=0):
        """lls_icp_3dof_ground on one PairData or a list of them."""
        plist = pairs if isinstance(pairs, (list, tuple)) else [pairs]
        arr = abi.make_pair_array(plist)
        res = abi.make_result_array(len(plist), trace_cap)
        self._check(self.lib.mulls_icp_3dof_ground_batch(self.h, arr, len(plist), C.byref(params), res), "mulls_icp_3dof_ground_batch")
        return res

    def icp_4dof_global(self, pair, heading_step_d, station, max_iter_num=20, dis_thre_unit=1.5, converge_translation=0.005,
                        converge_rotation_d=0.05, dis_thre_min=0.5, dis_thre_update_rate=1.05, max_bearable_rotation_d=15.0):
        """mm_lls_icp_4dof_global.  Returns (results, success, best_heading_deg)."""
        res = abi.make_result_array(1, 0)
        p = pair.as_pair()
        ok, best = C.c_int(0), C.c_float(0)
        st = (C.c_double * 3)(*station)
        self._check(self.lib.mulls_icp_4dof_global(self.h, C.byref(p), heading_step_d, st, int(max_iter_num), dis_thre_unit, converge_translation,
                                                   converge_rotation_d, dis_thre_min, dis_thre_update_rate, max_bearable_rotation_d, res,
                                                   C.byref(ok), C.byref(best)), "mulls_icp_4dof_global")
        return res, bool(ok.value), float(best.value)

    # --- feature extraction, first stage -------------------------------------------------------------------
    def ground_filter(self, pts, params):
        """CFilter::fast_ground_filter on the device.  Returns (ground, ground_down, unground) as (n, 48) uint8 record arrays."""
        pts = abi.as_points(pts)
        n = len(pts)
        raw = [np.zeros(max(n, 1) * abi.POINT_BYTES, np.uint8) for _ in range(3)]
        nout = (C.c_uint32 * 3)()
        self._check(self.lib.mulls_ground_filter(self.h, pts.ctypes.data_as(C.c_void_p), n, abi.POINT_BYTES, C.byref(params), raw[0].ctypes.data_as(C.c_void_p), n,
                                                 raw[1].ctypes.data_as(C.c_void_p), n, raw[2].ctypes.data_as(C.c_void_p), n, nout), "mulls_ground_filter")
        return [raw[k][: nout[k] * abi.POINT_BYTES].reshape(nout[k], abi.POINT_BYTES).copy() for k in range(3)]

    # --- feature extraction, second stage -----------------------------------------------------------------------------------
    def classify_nground(self, pts, params, with_cloud_in=False):
        """CFilter::classify_nground_pts on the device.  Returns the nine clouds of enum mulls_classify_cloud as (n, 48) uint8 record arrays
        (and, with_cloud_in, the input cloud as the function leaves it)."""
        raw_in = abi.records(pts)
        n = len(raw_in)
        outs = [np.zeros((max(n, 1), abi.POINT_BYTES), np.uint8) for _ in range(abi.CL_COUNT)]
        out_p = (C.c_void_p * abi.CL_COUNT)(*[o.ctypes.data for o in outs])
        cap = (C.c_uint32 * abi.CL_COUNT)(*([n] * abi.CL_COUNT))
        nout = (C.c_uint32 * abi.CL_COUNT)()
        after = np.zeros((max(n, 1), abi.POINT_BYTES), np.uint8)
        n_after = C.c_uint32(0)
        self._check(self.lib.mulls_classify_nground(self.h, raw_in.ctypes.data_as(C.c_void_p), n, abi.POINT_BYTES, C.byref(params), out_p, cap, nout,
                                                    after.ctypes.data_as(C.c_void_p) if with_cloud_in else None, C.byref(n_after)), "mulls_classify_nground")
        res = [outs[k][: nout[k]].copy() for k in range(abi.CL_COUNT)]
        return (res, after[: n_after.value].copy()) if with_cloud_in else res

    def extract_features(self, scan, params):
        """CFilter::extract_semantic_pts' chain on the device in one call.  Returns the clouds of enum mulls_extract_cloud as (n, 48) uint8 arrays."""
        raw_in = abi.records(scan)
        n = len(raw_in)
        if getattr(self, "_ex_cap", 0) < n:  # receive buffers kept between calls (fresh pages cost more than the transfers)
            self._ex_out = [np.zeros((max(n, 1), abi.POINT_BYTES), np.uint8) for _ in range(abi.EX_COUNT)]
            self._ex_cap = n
        outs = self._ex_out
        out_p = (C.c_void_p * abi.EX_COUNT)(*[o.ctypes.data for o in outs])
        cap = (C.c_uint32 * abi.EX_COUNT)(*([n] * abi.EX_COUNT))
        filtered = bool(params.apply_scanner_filter or params.apply_dist_filter)
        voxels = not (params.vf_downsample_resolution < 0.001)
        if not filtered:
            cap[abi.EX_RAW] = 0  # pc_raw is the scan itself: not sent back
        if not voxels:
            cap[abi.EX_DOWN] = 0  # pc_down is pc_raw
        nout = (C.c_uint32 * abi.EX_COUNT)()
        self._check(self.lib.mulls_extract_features(self.h, raw_in.ctypes.data_as(C.c_void_p), n, abi.POINT_BYTES, C.byref(params), out_p, cap, nout),
                    "mulls_extract_features")
        res = [outs[k][: nout[k]].copy() for k in range(abi.EX_COUNT)]
        if not filtered:
            res[abi.EX_RAW] = raw_in
        if not voxels:
            res[abi.EX_DOWN] = res[abi.EX_RAW]
        return res

    def map_update_batch(self, maps, frames, poses, params, max_lockstep=0, check=True, shared_params=None):
        """mulls_map_update_batch: one update_local_map per LocalMap, in lock step on the device.  frames[i]: the six clouds LocalMap.update takes (point arrays or
        abi.Cloud device clouds), poses[i]: the frame's pose_lo, params: one abi.MapParams for all or a list with one per map
        (a None entry takes shared_params).  Returns (reports, stats): one abi.MapReport per map and the abi.MapBatchStats; check=False returns
        (results, stats, rc) with the abi.MapBatchResult records instead and does not raise on a refused item."""
        n = len(maps)
        per_item = isinstance(params, (list, tuple))
        shared = shared_params if per_item else params
        items, keep = (abi.MapUpdateItem * max(n, 1))(), []
        for i in range(n):
            items[i].map = maps[i].h if isinstance(maps[i], LocalMap) else maps[i]
            if frames[i] is not None:
                arr, held = LocalMap._clouds(frames[i])
                keep.append((arr, held))
                items[i].frame_down = arr
            items[i].frame_pose_lo = abi.colmajor16(poses[i])
            if per_item and params[i] is not None:
                items[i].params = C.pointer(params[i])
        results, stats = (abi.MapBatchResult * max(n, 1))(), abi.MapBatchStats()
        rc = self.lib.mulls_map_update_batch(self.h, items, n, C.byref(shared) if shared is not None else None, int(max_lockstep), results, C.byref(stats))
        if not check:
            return [results[i] for i in range(n)], stats, rc
        self._check(rc, "mulls_map_update_batch")
        return [results[i].report for i in range(n)], stats

    def extract_features_batch(self, scans, params, blocks=None, scratch_limit_bytes=0, check=True):
        """mulls_extract_features_batch: extract_semantic_pts' chain on many scans per call, in lock step on the device, the feature clouds left in one Block per scan.
        scans: record arrays (abi.records takes them) or abi.Cloud structures (device-resident clouds, strided host records).  Returns (blocks, results, stats):
        the Blocks (created here when none are given), one abi.ExtractBatchResult per scan, the abi.ExtractBatchStats.  check=False: a refused scan does not raise;
        the call's code is left in self.last_batch_rc."""
        n = len(scans)
        keep, clouds = [], (abi.Cloud * max(n, 1))()
        for i, sc in enumerate(scans):
            if isinstance(sc, abi.Cloud):
                clouds[i] = sc
                continue
            raw = abi.records(sc)
            keep.append(raw)
            clouds[i].pts, clouds[i].n, clouds[i].stride = raw.ctypes.data if len(raw) else None, len(raw), abi.POINT_BYTES
        if blocks is None:
            blocks = [Block(self) for _ in range(n)]
        handles = (C.c_void_p * max(n, 1))(*[b.h for b in blocks])
        results = (abi.ExtractBatchResult * max(n, 1))()
        stats = abi.ExtractBatchStats()
        self.last_batch_rc = self.lib.mulls_extract_features_batch(self.h, clouds, n, C.byref(params), handles, int(scratch_limit_bytes), results, C.byref(stats))
        for b, r in zip(blocks, results):
            b.n = list(r.n_out)
        if check:
            self._check(self.last_batch_rc, "mulls_extract_features_batch")
        return blocks, [results[i] for i in range(n)], stats

    def voxel_downsample(self, pts, voxel_size):
        """CFilter::voxel_downsample (cfilter.hpp:83-160).  Returns pc_down as (n, 48) uint8 records."""
        raw_in = abi.records(pts)
        n = len(raw_in)
        out = np.zeros((max(n, 1), abi.POINT_BYTES), np.uint8)
        n_out = C.c_uint32(0)
        self._check(self.lib.mulls_voxel_downsample(self.h, raw_in.ctypes.data_as(C.c_void_p), n, abi.POINT_BYTES, C.c_float(voxel_size),
                                                    out.ctypes.data_as(C.c_void_p), n, C.byref(n_out)), "mulls_voxel_downsample")
        return out[: n_out.value].copy()

    # --- key-point descriptor matching -------------------------------------------------------------------------------
    def ncc_correspond(self, tgt_kpts, src_kpts, params=None, cap=None):
        """find_feature_correspondence_ncc (mulls_ncc_correspond).  tgt_kpts / src_kpts: host clouds (POINT_DTYPE records or raw (n, 48) bytes) or
        device-resident abi.Cloud objects (Block.cloud(abi.EX_VERTEX)).  Returns (ok, tgt_idx, src_idx, n_corr): the reference's bool, the index pairs
        actually written (min(n_corr, cap) of them; cap defaults to what the mode can return at most) and the full count."""
        keep = []

        def cloud(k):
            if isinstance(k, abi.Cloud):
                return k
            raw = abi.records(k)
            keep.append(raw)
            c = abi.Cloud()
            c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
            return c

        ct, cs = cloud(tgt_kpts), cloud(src_kpts)
        p = params if params is not None else abi.ncc_params()
        if cap is None:
            cap = max(0, min(p.corr_num, 65536)) if p.fixed_num_corr else ct.n
        ti, si = np.full(cap + 1, -1, np.int32), np.full(cap + 1, -1, np.int32)  # one slot past cap: callers may check that it is left alone
        n = C.c_uint32(0)
        rc = self.lib.mulls_ncc_correspond(self.h, C.byref(ct), C.byref(cs), C.byref(p), ti.ctypes.data_as(C.c_void_p), si.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        if rc < 0:
            raise MullsError("mulls_ncc_correspond failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        w = min(n.value, cap)
        assert ti[cap] == -1 and si[cap] == -1
        return bool(rc), ti[:w].copy(), si[:w].copy(), n.value

    def ncc_correspond_batch(self, problems, params=None, scratch_limit=0):
        """mulls_ncc_correspond_batch: many problems per call, each with the result of the matching ncc_correspond call.  problems: a list of
        (tgt_kpts, src_kpts) or dicts with the keys tgt, src and optionally cap (the clouds are host clouds or device-resident abi.Cloud objects; a host
        cloud may also be an abi.Cloud with a stride of its own; the same array object in several problems is the same cloud to the library).  One params
        for the whole batch.  scratch_limit: scratch_limit_bytes (0: the library's default).  Returns [(ok, tgt_idx, src_idx, n_corr), ...] as
        ncc_correspond does per problem."""
        keep = {}

        def cloud(k):
            if isinstance(k, abi.Cloud):
                return k
            if id(k) not in keep:  # one conversion per array object: the same pointer wherever it appears
                keep[id(k)] = (k, abi.records(k))
            raw = keep[id(k)][1]
            c = abi.Cloud()
            c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
            return c

        n = len(problems)
        p = params if params is not None else abi.ncc_params()
        arr, res, lists = (abi.NccProblem * max(n, 1))(), (abi.NccResult * max(n, 1))(), []
        for b, prob in enumerate(problems):
            if not isinstance(prob, dict):
                prob = dict(zip(("tgt", "src"), prob))
            P = arr[b]
            P.tgt, P.src = cloud(prob["tgt"]), cloud(prob["src"])
            cap = prob.get("cap")
            if cap is None:
                cap = max(0, min(p.corr_num, 65536)) if p.fixed_num_corr else P.tgt.n
            ti, si = np.full(cap + 1, -1, np.int32), np.full(cap + 1, -1, np.int32)  # one slot past cap: checked to be left alone
            lists.append((ti, si))
            P.tgt_idx, P.src_idx, P.cap = ti.ctypes.data, si.ctypes.data, cap
        rc = self.lib.mulls_ncc_correspond_batch(self.h, arr, n, C.byref(p), int(scratch_limit), res)
        if rc != 0:
            raise MullsError("mulls_ncc_correspond_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        out = []
        for b in range(n):
            (ti, si), cap = lists[b], arr[b].cap
            assert ti[cap] == -1 and si[cap] == -1
            w = min(res[b].n_corr, cap)
            out.append((bool(res[b].ret), ti[:w].copy(), si[:w].copy(), int(res[b].n_corr)))
        return out

    # --- RANSAC coarse registration --------------------------------------------------------------------------------
    def coarse_reg_ransac(self, tgt_pts, src_pts, params=None, cap=None, tgt_idx=None, src_idx=None):
        """coarse_reg_ransac (mulls_coarse_reg_ransac; with tgt_idx / src_idx, mulls_coarse_reg_ransac_indexed on the pairs those lists name).  The clouds
        are host clouds or device-resident abi.Cloud objects, as for ncc_correspond.  Returns (result, inliers): the abi.RansacResult and the ascending
        inlier indices actually written (min(n_inliers, cap) of them; cap defaults to the number of pairs)."""
        keep = []

        def cloud(k):
            if isinstance(k, abi.Cloud):
                return k
            raw = abi.records(k)
            keep.append(raw)
            c = abi.Cloud()
            c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
            return c

        ct, cs = cloud(tgt_pts), cloud(src_pts)
        p = params if params is not None else abi.ransac_params()
        res = abi.RansacResult()
        indexed = tgt_idx is not None
        if indexed:
            ti, si = np.ascontiguousarray(tgt_idx, np.int32), np.ascontiguousarray(src_idx, np.int32)
            assert len(ti) == len(si)
        n_pairs = len(ti) if indexed else ct.n
        if cap is None:
            cap = n_pairs
        inl = np.full(cap + 1, -1, np.int32)  # one slot past cap: checked to be left alone
        ip = inl.ctypes.data_as(C.c_void_p) if cap else None
        if indexed:
            rc = self.lib.mulls_coarse_reg_ransac_indexed(self.h, C.byref(ct), C.byref(cs), ti.ctypes.data_as(C.c_void_p), si.ctypes.data_as(C.c_void_p), len(ti),
                                                          C.byref(p), C.byref(res), ip, cap)
        else:
            rc = self.lib.mulls_coarse_reg_ransac(self.h, C.byref(ct), C.byref(cs), C.byref(p), C.byref(res), ip, cap)
        if rc != 0:
            raise MullsError("mulls_coarse_reg_ransac failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        assert inl[cap] == -1
        return res, inl[: min(res.n_inliers, cap)].copy()

    def coarse_reg_ransac_batch(self, problems, params=None, scratch_limit=0):
        """mulls_coarse_reg_ransac_batch: many problems per call, each with the result of the matching coarse_reg_ransac call.  problems: a list of
        (tgt_pts, src_pts) or (tgt_pts, src_pts, tgt_idx, src_idx) or dicts with the keys tgt, src and optionally tgt_idx, src_idx, cap (the clouds are host
        clouds or device-resident abi.Cloud objects; a host cloud may also be an abi.Cloud with a stride of its own).  One params for the whole batch.
        scratch_limit: scratch_limit_bytes (0: the library's default).  Returns [(result, inliers), ...] as coarse_reg_ransac does per problem."""
        keep = []

        def cloud(k):
            if isinstance(k, abi.Cloud):
                return k
            raw = abi.records(k)
            keep.append(raw)
            c = abi.Cloud()
            c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
            return c

        n = len(problems)
        p = params if params is not None else abi.ransac_params()
        arr, res, lists = (abi.RansacProblem * max(n, 1))(), (abi.RansacResult * max(n, 1))(), []
        for b, prob in enumerate(problems):
            if not isinstance(prob, dict):
                prob = dict(zip(("tgt", "src", "tgt_idx", "src_idx"), prob))
            P = arr[b]
            P.tgt, P.src = cloud(prob["tgt"]), cloud(prob["src"])
            n_pairs = P.tgt.n
            if prob.get("tgt_idx") is not None:
                ti, si = np.ascontiguousarray(prob["tgt_idx"], np.int32), np.ascontiguousarray(prob["src_idx"], np.int32)
                assert len(ti) == len(si)
                keep.extend((ti, si))
                P.tgt_idx, P.src_idx, P.n_corr = ti.ctypes.data, si.ctypes.data, len(ti)
                if not len(ti):  # (an empty array has no address to speak of: the lists stay set)
                    P.tgt_idx = P.src_idx = C.addressof(arr)
                n_pairs = len(ti)
            cap = prob.get("cap")
            cap = n_pairs if cap is None else cap
            inl = np.full(cap + 1, -1, np.int32)  # one slot past cap: checked to be left alone
            lists.append(inl)
            P.inlier_cap, P.inliers = cap, (inl.ctypes.data if cap else None)
        rc = self.lib.mulls_coarse_reg_ransac_batch(self.h, arr, n, C.byref(p), int(scratch_limit), res)
        if rc != 0:
            raise MullsError("mulls_coarse_reg_ransac_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        out = []
        for b in range(n):
            cap = arr[b].inlier_cap
            assert lists[b][cap] == -1
            r = abi.RansacResult.from_buffer_copy(res[b])
            out.append((r, lists[b][: min(r.n_inliers, cap)].copy()))
        return out

    # --- TEASER coarse registration ----------------------------------------------------------------------------------
    def coarse_reg_teaser(self, tgt_pts, src_pts, params=None, cap=None, tgt_idx=None, src_idx=None):
        """coarse_reg_teaser (mulls_coarse_reg_teaser; with tgt_idx / src_idx, mulls_coarse_reg_teaser_indexed on the pairs those lists name).  The clouds
        are host clouds or device-resident abi.Cloud objects, as for coarse_reg_ransac.  Returns (result, clique): the abi.TeaserResult and the ascending
        clique indices actually written (min(clique_size, cap) of them; cap defaults to the number of pairs)."""
        keep = []

        def cloud(k):
            if isinstance(k, abi.Cloud):
                return k
            raw = abi.records(k)
            keep.append(raw)
            c = abi.Cloud()
            c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
            return c

        ct, cs = cloud(tgt_pts), cloud(src_pts)
        p = params if params is not None else abi.teaser_params()
        res = abi.TeaserResult()
        indexed = tgt_idx is not None
        if indexed:
            ti, si = np.ascontiguousarray(tgt_idx, np.int32), np.ascontiguousarray(src_idx, np.int32)
            assert len(ti) == len(si)
        n_pairs = len(ti) if indexed else ct.n
        if cap is None:
            cap = n_pairs
        clique = np.full(cap + 1, -1, np.int32)  # one slot past cap: checked to be left alone
        ip = clique.ctypes.data_as(C.c_void_p) if cap else None
        if indexed:
            rc = self.lib.mulls_coarse_reg_teaser_indexed(self.h, C.byref(ct), C.byref(cs), ti.ctypes.data_as(C.c_void_p), si.ctypes.data_as(C.c_void_p), len(ti),
                                                          C.byref(p), C.byref(res), ip, cap)
        else:
            rc = self.lib.mulls_coarse_reg_teaser(self.h, C.byref(ct), C.byref(cs), C.byref(p), C.byref(res), ip, cap)
        if rc != 0:
            raise MullsError("mulls_coarse_reg_teaser failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        assert clique[cap] == -1
        return res, clique[: min(max(res.clique_size, 0), cap)].copy()

    def coarse_reg_teaser_batch(self, problems, params=None, scratch_limit=0):
        """mulls_coarse_reg_teaser_batch: many problems per call, each with the result of the matching coarse_reg_teaser call.  problems: a list of
        (tgt_pts, src_pts) or (tgt_pts, src_pts, tgt_idx, src_idx) or dicts with the keys tgt, src and optionally tgt_idx, src_idx, cap (the clouds are host
        clouds or device-resident abi.Cloud objects; a host cloud may also be an abi.Cloud with a stride of its own).  One params for the whole batch.
        scratch_limit: scratch_limit_bytes (0: the library's default).  Returns [(result, clique), ...] as coarse_reg_teaser does per problem."""
        keep = []

        def cloud(k):
            if isinstance(k, abi.Cloud):
                return k
            raw = abi.records(k)
            keep.append(raw)
            c = abi.Cloud()
            c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
            return c

        n = len(problems)
        p = params if params is not None else abi.teaser_params()
        arr, res, cliques = (abi.TeaserProblem * max(n, 1))(), (abi.TeaserResult * max(n, 1))(), []
        for b, prob in enumerate(problems):
            if not isinstance(prob, dict):
                prob = dict(zip(("tgt", "src", "tgt_idx", "src_idx"), prob))
            P = arr[b]
            P.tgt, P.src = cloud(prob["tgt"]), cloud(prob["src"])
            n_pairs = P.tgt.n
            if prob.get("tgt_idx") is not None:
                ti, si = np.ascontiguousarray(prob["tgt_idx"], np.int32), np.ascontiguousarray(prob["src_idx"], np.int32)
                assert len(ti) == len(si)
                keep.extend((ti, si))
                P.tgt_idx, P.src_idx, P.n_corr = ti.ctypes.data, si.ctypes.data, len(ti)
                if not len(ti):  # (an empty array has no address to speak of: the lists stay set)
                    P.tgt_idx = P.src_idx = C.addressof(arr)
                n_pairs = len(ti)
            cap = prob.get("cap")
            cap = n_pairs if cap is None else cap
            clique = np.full(cap + 1, -1, np.int32)  # one slot past cap: checked to be left alone
            cliques.append(clique)
            P.clique_cap, P.clique = cap, (clique.ctypes.data if cap else None)
        rc = self.lib.mulls_coarse_reg_teaser_batch(self.h, arr, n, C.byref(p), int(scratch_limit), res)
        if rc != 0:
            raise MullsError("mulls_coarse_reg_teaser_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        out = []
        for b in range(n):
            cap = arr[b].clique_cap
            assert cliques[b][cap] == -1
            r = abi.TeaserResult.from_buffer_copy(res[b])
            out.append((r, cliques[b][: min(max(r.clique_size, 0), cap)].copy()))
        return out

    # --- NDT registration ---------------------------------------------------------------------------------------------
    @staticmethod
    def _ndt_problem(prob, keep):
        """prob: (tgt, src, tgt_bound, src_bound, init_guess) or a dict with those keys; a cloud is an (n, 3) float32 array, a POINT_DTYPE array or an
        abi.Cloud (host or device memory); init_guess a row-major (4, 4) or None"""
        if not isinstance(prob, dict):
            prob = dict(zip(("tgt", "src", "tgt_bound", "src_bound", "init_guess"), prob))

        def cloud(k):
            if isinstance(k, abi.Cloud):
                return k
            k = np.asarray(k)
            raw = k if k.dtype == abi.POINT_DTYPE else np.ascontiguousarray(k, np.float32).reshape(-1, 3)
            raw = np.ascontiguousarray(raw)
            keep.append(raw)
            c = abi.Cloud()
            c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), (abi.POINT_BYTES if raw.dtype == abi.POINT_DTYPE else 12)
            return c

        P = abi.NdtProblem()
        P.tgt, P.src = cloud(prob["tgt"]), cloud(prob["src"])
        P.tgt_bound[:] = [float(v) for v in prob["tgt_bound"]]
        P.src_bound[:] = [float(v) for v in prob["src_bound"]]
        G = np.eye(4) if prob.get("init_guess") is None else np.asarray(prob["init_guess"], np.float64).reshape(4, 4)
        P.init_guess[:] = G.T.reshape(-1).tolist()
        return P

    def ndt(self, tgt, src, tgt_bound, src_bound, init_guess=None, params=None):
        """CRegistration::omp_ndt (mulls_ndt).  Returns the mulls_ndt_result; np.array(res.T).reshape(4, 4).T is the pose."""
        keep = []
        P = self._ndt_problem((tgt, src, tgt_bound, src_bound, init_guess), keep)
        p = params if params is not None else abi.ndt_params()
        res = abi.NdtResult()
        rc = self.lib.mulls_ndt(self.h, C.byref(P), C.byref(p), C.byref(res))
        if rc != 0:
            raise MullsError("mulls_ndt failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return res

    def ndt_batch(self, problems, params=None):
        """mulls_ndt_batch: many problems per call in lock step, each with the bits of its ndt call.  problems: as _ndt_problem takes them.  One params
        for the whole batch (its scratch_limit_bytes sizes the sub-batches).  Returns [mulls_ndt_result, ...]."""
        keep, B = [], len(problems)
        arr, res = (abi.NdtProblem * max(B, 1))(), (abi.NdtResult * max(B, 1))()
        for b, prob in enumerate(problems):
            arr[b] = self._ndt_problem(prob, keep)
        p = params if params is not None else abi.ndt_params()
        rc = self.lib.mulls_ndt_batch(self.h, arr, B, C.byref(p), res)
        if rc != 0:
            raise MullsError("mulls_ndt_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return [abi.NdtResult.from_buffer_copy(res[b]) for b in range(B)]

    # --- voxelised GICP registration ----------------------------------------------------------------------------------
    def gicp(self, tgt, src, tgt_bound, src_bound, init_guess=None, params=None):
        """CRegistration::omp_gicp with using_voxel_gicp = true (mulls_gicp).  The arguments are ndt's.  Returns the mulls_gicp_result."""
        keep = []
        P = self._ndt_problem((tgt, src, tgt_bound, src_bound, init_guess), keep)
        p = params if params is not None else abi.gicp_params()
        res = abi.GicpResult()
        rc = self.lib.mulls_gicp(self.h, C.byref(P), C.byref(p), C.byref(res))
        if rc != 0:
            raise MullsError("mulls_gicp failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return res

    def gicp_batch(self, problems, params=None):
        """mulls_gicp_batch: many problems per call in lock step, each with the bits of its gicp call.  problems: as _ndt_problem takes them.  One
        params for the whole batch (its scratch_limit_bytes sizes the sub-batches).  Returns [mulls_gicp_result, ...]."""
        keep, B = [], len(problems)
        arr, res = (abi.GicpProblem * max(B, 1))(), (abi.GicpResult * max(B, 1))()
        for b, prob in enumerate(problems):
            arr[b] = self._ndt_problem(prob, keep)
        p = params if params is not None else abi.gicp_params()
        rc = self.lib.mulls_gicp_batch(self.h, arr, B, C.byref(p), res)
        if rc != 0:
            raise MullsError("mulls_gicp_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return [abi.GicpResult.from_buffer_copy(res[b]) for b in range(B)]

    # --- classical ICP registration -----------------------------------------------------------------------------------
    def pcl_icp(self, tgt, src, tgt_bound, src_bound, init_guess=None, params=None):
        """CRegistration::pcl_icp, the part that is plain ICP (mulls_pcl_icp).  The arguments are ndt's.  Returns the mulls_pcl_icp_result."""
        keep = []
        P = self._ndt_problem((tgt, src, tgt_bound, src_bound, init_guess), keep)
        p = params if params is not None else abi.pcl_icp_params()
        res = abi.PclIcpResult()
        rc = self.lib.mulls_pcl_icp(self.h, C.byref(P), C.byref(p), C.byref(res))
        if rc != 0:
            raise MullsError("mulls_pcl_icp failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return res

    def pcl_icp_batch(self, problems, params=None):
        """mulls_pcl_icp_batch: many problems per call in lock step, each with the bits of its pcl_icp call.  problems: as _ndt_problem takes them.
        One params for the whole batch (its scratch_limit_bytes sizes the sub-batches).  Returns [mulls_pcl_icp_result, ...]."""
        keep, B = [], len(problems)
        arr, res = (abi.PclIcpProblem * max(B, 1))(), (abi.PclIcpResult * max(B, 1))()
        for b, prob in enumerate(problems):
            arr[b] = self._ndt_problem(prob, keep)
        p = params if params is not None else abi.pcl_icp_params()
        rc = self.lib.mulls_pcl_icp_batch(self.h, arr, B, C.byref(p), res)
        if rc != 0:
            raise MullsError("mulls_pcl_icp_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return [abi.PclIcpResult.from_buffer_copy(res[b]) for b in range(B)]

    # --- FPFH descriptors and SAC-IA coarse registration -----------------------------------------------------------------
    @staticmethod
    def _normal_cloud(k, keep):
        """a cloud with normals: a POINT_DTYPE array, a (pts, normals) pair of (n, 3) arrays, or an abi.Cloud (host or device memory, stride >= 28)"""
        if isinstance(k, abi.Cloud):
            return k
        raw = abi.make_points(k[0], k[1]) if isinstance(k, tuple) else np.ascontiguousarray(abi.as_points(k))
        keep.append(raw)
        return abi.as_cloud(raw)

    def fpfh(self, cloud, params=None):
        """CRegistration::compute_fpfh_feature (mulls_fpfh).  cloud: as _normal_cloud takes it.  Returns (hist (n, 33) float32, n_neighbours (n,) uint32)."""
        keep = []
        c = self._normal_cloud(cloud, keep)
        p = params if params is not None else abi.fpfh_params()
        hist, k = np.zeros((max(c.n, 1), abi.FPFH_DIMS), np.float32), np.zeros(max(c.n, 1), np.uint32)
        rc = self.lib.mulls_fpfh(self.h, C.byref(c), C.byref(p), hist.ctypes.data, k.ctypes.data)
        if rc != 0:
            raise MullsError("mulls_fpfh failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return hist[: c.n], k[: c.n]

    def coarse_reg_fpfhsac(self, tgt, src, params=None):
        """CRegistration::coarse_reg_fpfhsac (mulls_coarse_reg_fpfhsac).  tgt, src: as _normal_cloud takes them.  Returns the mulls_fpfhsac_result;
        np.array(res.T).reshape(4, 4).T is the pose, source to target."""
        keep = []
        ct, cs = self._normal_cloud(tgt, keep), self._normal_cloud(src, keep)
        p = params if params is not None else abi.fpfhsac_params()
        res = abi.FpfhSacResult()
        rc = self.lib.mulls_coarse_reg_fpfhsac(self.h, C.byref(ct), C.byref(cs), C.byref(p), C.byref(res))
        if rc != 0:
            raise MullsError("mulls_coarse_reg_fpfhsac failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return res

    def _normal_clouds(self, items, keep):
        """_normal_cloud of every item; the same Python object given twice becomes the same mulls_cloud, so that the batch calls see a shared cloud"""
        seen = {}
        out = []
        for k in items:
            if id(k) not in seen:
                seen[id(k)] = self._normal_cloud(k, keep)
                keep.append(k)
            out.append(seen[id(k)])
        return out

    def fpfh_batch(self, clouds, params=None, scratch_limit=0):
        """mulls_compute_fpfh_batch: the descriptors of many clouds per call, each with the bits of its fpfh() call.  clouds: as _normal_cloud takes them; an
        object given twice is one cloud, computed once.  Returns [(hist (n, 33) float32, n_neighbours (n,) uint32), ...]."""
        keep, n = [], len(clouds)
        cl = self._normal_clouds(clouds, keep)
        arr = (abi.Cloud * max(n, 1))(*cl)
        p = params if params is not None else abi.fpfh_params()
        out = [(np.zeros((max(c.n, 1), abi.FPFH_DIMS), np.float32), np.zeros(max(c.n, 1), np.uint32)) for c in cl]
        hp, kp = (C.c_void_p * max(n, 1))(*[h.ctypes.data for h, _ in out]), (C.c_void_p * max(n, 1))(*[k.ctypes.data for _, k in out])
        rc = self.lib.mulls_compute_fpfh_batch(self.h, arr, n, C.byref(p), hp, kp, scratch_limit)
        if rc != 0:
            raise MullsError("mulls_compute_fpfh_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return [(h[: c.n], k[: c.n]) for (h, k), c in zip(out, cl)]

    def coarse_reg_fpfhsac_batch(self, problems, params=None, scratch_limit=0):
        """mulls_coarse_reg_fpfhsac_batch: many SAC-IA problems per call in lock step, each with the bytes of its coarse_reg_fpfhsac call.  problems:
        (tgt, src) pairs as _normal_cloud takes them; an object given twice (as a source, a target or both) is one cloud, staged once with its
        descriptors computed once per sub-batch.  One params for the whole batch.  Returns [mulls_fpfhsac_result, ...]."""
        keep, B = [], len(problems)
        flat = self._normal_clouds([k for prob in problems for k in prob], keep)
        arr, res = (abi.FpfhSacProblem * max(B, 1))(), (abi.FpfhSacResult * max(B, 1))()
        for b in range(B):
            arr[b].tgt, arr[b].src = flat[2 * b], flat[2 * b + 1]
        p = params if params is not None else abi.fpfhsac_params()
        rc = self.lib.mulls_coarse_reg_fpfhsac_batch(self.h, arr, B, C.byref(p), scratch_limit, res)
        if rc != 0:
            raise MullsError("mulls_coarse_reg_fpfhsac_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return [abi.FpfhSacResult.from_buffer_copy(res[b]) for b in range(B)]

    # --- pose graph optimisation --------------------------------------------------------------------------------------
    def pgo_optimize(self, poses, fixed, stable, edges, params=None):
        """optimize_pose_graph_ceres (mulls_pgo_optimize).  poses: (n, 4, 4) pose_init; fixed, stable: (n,) flags; edges: a list of
        (a, b, type, T (4, 4), info (6, 6)).  Returns (result, poses_out (n, 4, 4), edge_wrong (n_edges,) uint8)."""
        poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        n, m = len(poses), len(edges)
        p = params if params is not None else abi.pgo_params()
        nodes, earr = abi.pgo_nodes(poses, fixed, stable), abi.pgo_edges(edges)
        out, wrong, res = np.zeros((max(n, 1), 16)), np.zeros(max(m, 1), np.uint8), abi.PgoResult()
        rc = self.lib.mulls_pgo_optimize(self.h, C.addressof(nodes) if n else None, n, C.addressof(earr) if m else None, m, C.byref(p),
                                         out.ctypes.data if n else None, wrong.ctypes.data, C.byref(res))
        if rc != 0:
            raise MullsError("mulls_pgo_optimize failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return res, out[:n].reshape(n, 4, 4).transpose(0, 2, 1).copy(), wrong[:m].copy()

    def pgo_optimize_batch(self, problems, params=None, scratch_limit=0):
        """mulls_pgo_optimize_batch: many independent problems per call, each with the bits of its pgo_optimize call.  problems: a list of
        (poses, fixed, stable, edges) as pgo_optimize takes them.  One params for the whole batch.  scratch_limit: scratch_limit_bytes (0: the
        library's default).  Returns [(result, poses_out, edge_wrong), ...]."""
        B = len(problems)
        p = params if params is not None else abi.pgo_params()
        arr, res, keep = (abi.PgoProblem * max(B, 1))(), (abi.PgoResult * max(B, 1))(), []
        for b, (poses, fixed, stable, edges) in enumerate(problems):
            poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
            n, m = len(poses), len(edges)
            nodes, earr = abi.pgo_nodes(poses, fixed, stable), abi.pgo_edges(edges)
            out, wrong = np.zeros((max(n, 1), 16)), np.zeros(max(m, 1), np.uint8)
            keep.append((nodes, earr, out, wrong, n, m))
            arr[b].nodes, arr[b].n_nodes = (C.addressof(nodes) if n else None), n
            arr[b].edges, arr[b].n_edges = (C.addressof(earr) if m else None), m
            arr[b].poses_out, arr[b].edge_wrong = (out.ctypes.data if n else None), wrong.ctypes.data
        rc = self.lib.mulls_pgo_optimize_batch(self.h, arr, B, C.byref(p), int(scratch_limit), res)
        if rc != 0:
            raise MullsError("mulls_pgo_optimize_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return [(abi.PgoResult.from_buffer_copy(res[b]), out[:n].reshape(n, 4, 4).transpose(0, 2, 1).copy(), wrong[:m].copy())
                for b, (_, _, out, wrong, n, m) in enumerate(keep)]

    # --- statistical outlier removal ---------------------------------------------------------------------------------
    def sor_filter(self, pts, params=None, want_dist=False):
        """CFilter::sor_filter (mulls_sor_filter).  pts: a host cloud (POINT_DTYPE records or raw (n, 48) bytes) or a device-resident abi.Cloud.
        Returns (kept, kept_idx, report), with the (n,) float32 mean neighbour distances behind them when want_dist: kept are the kept records as raw
        (n_kept, 48) bytes, kept_idx their ascending indices, report the abi.SorReport."""
        if isinstance(pts, abi.Cloud):
            c, raw = pts, None
        else:
            raw = abi.records(pts)
            c = abi.Cloud()
            c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
        n = c.n
        p = params if params is not None else abi.sor_params()
        out = np.zeros((n + 1, abi.POINT_BYTES), np.uint8)
        idx = np.full(n + 1, -1, np.int32)  # one slot past n: checked to be left alone
        dist = np.zeros(n, np.float32) if want_dist else None
        rep, n_out = abi.SorReport(), C.c_uint32(0)
        rc = self.lib.mulls_sor_filter(self.h, C.byref(c), C.byref(p), out.ctypes.data_as(C.c_void_p), n, C.byref(n_out), idx.ctypes.data_as(C.c_void_p), n,
                                       dist.ctypes.data_as(C.c_void_p) if want_dist else None, C.byref(rep))
        if rc != 0:
            raise MullsError("mulls_sor_filter failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        assert idx[n] == -1 and n_out.value <= n
        res = (out[: n_out.value].copy(), idx[: n_out.value].copy(), rep)
        return res + (dist,) if want_dist else res

    # --- key-point non-maximum suppression ---------------------------------------------------------------------------
    def non_max_suppress(self, pts, radius=0.25, path=0):
        """CFilter::non_max_suppress (mulls_non_max_suppress).  pts: a host cloud (POINT_DTYPE records or raw (n, 48) bytes) or a device-resident abi.Cloud.
        Returns (kept, kept_idx, order, report): the kept records as raw (n_kept, 48) bytes in visiting order, their indices into the input, the whole
        visiting permutation (the identity under the gate of 10 points), the abi.NmsReport.  path: 0 = the library chooses (the multi-launch path),
        1 = one workgroup (at most abi.NMS_LDS_MAX_POINTS points), 2 = multi-launch; the outputs are the same bytes."""
        if isinstance(pts, abi.Cloud):
            c, raw = pts, None
        else:
            raw = abi.records(pts)
            c = abi.Cloud()
            c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
        n = c.n
        p = abi.nms_params(radius, path)
        out = np.zeros((n + 1, abi.POINT_BYTES), np.uint8)
        idx = np.full(n + 1, -1, np.int32)  # one slot past n: checked to be left alone
        order = np.full(n + 1, -1, np.int32)
        rep, n_out = abi.NmsReport(), C.c_uint32(0)
        rc = self.lib.mulls_non_max_suppress(self.h, C.byref(c), C.byref(p), out.ctypes.data_as(C.c_void_p), n, C.byref(n_out), idx.ctypes.data_as(C.c_void_p), n,
                                             order.ctypes.data_as(C.c_void_p), C.byref(rep))
        if rc != 0:
            raise MullsError("mulls_non_max_suppress failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        assert idx[n] == -1 and order[n] == -1 and n_out.value <= n
        return out[: n_out.value].copy(), idx[: n_out.value].copy(), order[:n].copy(), rep

    def non_max_suppress_batch(self, clouds, radius=0.25, path=0, scratch_limit_bytes=0):
        """mulls_non_max_suppress_batch: many clouds per call.  clouds: a list of what non_max_suppress takes (the same object may appear more than once).
        Returns a list with, per cloud, what non_max_suppress returns: (kept, kept_idx, order, report).  path: 0 = the library chooses per cloud (one
        workgroup per cloud up to abi.NMS_LDS_MAX_POINTS points, all of them in one launch; the multi-launch path beyond), 1 and 2 force a path."""
        n = len(clouds)
        arr, reps, keep, bufs = (abi.NmsProblem * max(n, 1))(), (abi.NmsReport * max(n, 1))(), [], []
        for b, pts in enumerate(clouds):
            if isinstance(pts, abi.Cloud):
                c = pts
            else:
                raw = abi.records(pts)
                c = abi.Cloud()
                c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
                keep.append(raw)
            m = c.n
            out, idx, order = np.zeros((m + 1, abi.POINT_BYTES), np.uint8), np.full(m + 1, -1, np.int32), np.full(m + 1, -1, np.int32)  # one slot past m: left alone
            arr[b].cloud, arr[b].out, arr[b].kept_idx, arr[b].order, arr[b].cap, arr[b].idx_cap = c, out.ctypes.data, idx.ctypes.data, order.ctypes.data, m, m
            bufs.append((out, idx, order))
        p = abi.nms_params(radius, path)
        rc = self.lib.mulls_non_max_suppress_batch(self.h, arr, n, C.byref(p), int(scratch_limit_bytes), reps)
        if rc != 0:
            raise MullsError("mulls_non_max_suppress_batch failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        res = []
        for b in range(n):
            out, idx, order = bufs[b]
            m, nk = arr[b].cloud.n, reps[b].n_kept
            assert idx[m] == -1 and order[m] == -1 and nk <= m
            rep = abi.NmsReport.from_buffer_copy(reps[b])
            res.append((out[:nk].copy(), idx[:nk].copy(), order[:m].copy(), rep))
        return res

    # --- scan preparation ----------------------------------------------------------------------------------------------
    def scan_prepare(self, pts, params):
        """The raw-scan steps of CFilter (mulls_scan_prepare: calibration, dist filter, thinning, time ratio) on a copy of a host cloud.  Returns (kept, report):
        the records that stay as raw (n_out, 48) bytes in input order, the abi.ScanPrepReport.  (A device buffer is prepared in place by the C call itself.)"""
        raw = abi.records(pts).copy()
        rep, n_out = abi.ScanPrepReport(), C.c_uint32(0)
        rc = self.lib.mulls_scan_prepare(self.h, C.c_void_p(raw.ctypes.data) if len(raw) else None, len(raw), abi.POINT_BYTES, C.byref(params), C.byref(n_out), C.byref(rep))
        if rc != 0:
            raise MullsError("mulls_scan_prepare failed with %d: %s" % (rc, self.lib.mulls_last_error(self.h).decode()), rc)
        return raw[: n_out.value].copy(), rep

    def mapper(self, capacity_points):
        return Mapper(self, capacity_points)

    # --- the pictures of a cloud ----------------------------------------------------------------------------------------
    GUARD = 0xA5  # what the image buffers are filled with, and what their one slot past the end must still hold

    @staticmethod
    def _image_cloud(pts, keep):
        """a host cloud (POINT_DTYPE records or raw (n, 48) bytes) or a device-resident abi.Cloud as an abi.Cloud"""
        if isinstance(pts, abi.Cloud):
            return pts
        raw = abi.records(pts)
        keep.append(raw)
        c = abi.Cloud()
        c.pts, c.n, c.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
        return c

    def _image_raise(self, rc, what):
        raise MullsError("%s failed with %d: %s" % (what, rc, self.lib.mulls_last_error(self.h).decode()), rc)

    def cloud_centre(self, pts):
        """CloudUtility::get_cloud_cpt (mulls_cloud_centre): the (3,) float64 centre point of a host cloud or a device-resident abi.Cloud"""
        keep, c = [], np.zeros(3, np.float64)
        cl = self._image_cloud(pts, keep)
        rc = self.lib.mulls_cloud_centre(self.h, C.byref(cl), c.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != 0:
            self._image_raise(rc, "mulls_cloud_centre")
        return c

    def map_image_2d(self, pts, params=None, want_counts=False):
        """CFilter::generate_2d_map (mulls_map_image_2d).  Returns (image, report), or (image, counts, report) when want_counts: the (map_height, map_width)
        uint8 picture, the int32 counts behind it, the abi.Image2dReport."""
        p = params if params is not None else abi.image2d_params()
        keep = []
        cl = self._image_cloud(pts, keep)
        npix = max(p.map_width, 0) * max(p.map_height, 0)
        img = np.full(npix + 1, self.GUARD, np.uint8)  # one slot past the end: checked to be left alone
        cnt = np.full(npix + 1, -7, np.int32) if want_counts else None
        rep = abi.Image2dReport()
        rc = self.lib.mulls_map_image_2d(self.h, C.byref(cl), C.byref(p), img.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p) if want_counts else None, C.byref(rep))
        if rc != 0:
            self._image_raise(rc, "mulls_map_image_2d")
        assert img[npix] == self.GUARD and (cnt is None or cnt[npix] == -7)
        img = img[:npix].reshape(p.map_height, p.map_width).copy()
        return (img, cnt[:npix].reshape(p.map_height, p.map_width).copy(), rep) if want_counts else (img, rep)

    def range_image(self, pts, params=None):
        """CFilter::pointcloud_to_rangeimage (mulls_range_image): the (height, width) uint8 range image"""
        p = params if params is not None else abi.range_image_params()
        keep = []
        cl = self._image_cloud(pts, keep)
        npix = max(p.width, 0) * max(p.height, 0)
        img = np.full(npix + 1, self.GUARD, np.uint8)
        rc = self.lib.mulls_range_image(self.h, C.byref(cl), C.byref(p), img.ctypes.data_as(C.c_void_p))
        if rc != 0:
            self._image_raise(rc, "mulls_range_image")
        assert img[npix] == self.GUARD
        return img[:npix].reshape(p.height, p.width).copy()

    def scan_images_batch(self, scans, range_params=None, bev_params=None):
        """mulls_scan_images_batch: the range image and / or the 2-D map image of many scans in one call.  scans: a list of what map_image_2d takes.
        Returns (range images or None, 2-D map images or None, reports or None): lists with one entry per scan."""
        n, keep = len(scans), []
        arr = (abi.Cloud * max(n, 1))()
        for k, s in enumerate(scans):
            arr[k] = self._image_cloud(s, keep)

        def outputs(npix):
            bufs = [np.full(npix + 1, self.GUARD, np.uint8) for _ in range(n)]
            return bufs, (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])

        rp, bp = range_params, bev_params
        rpix = rp.width * rp.height if rp is not None else 0
        bpix = bp.map_width * bp.map_height if bp is not None else 0
        rbufs, rptr = outputs(rpix) if rp is not None else (None, None)
        bbufs, bptr = outputs(bpix) if bp is not None else (None, None)
        reps = (abi.Image2dReport * max(n, 1))() if bp is not None else None
        rc = self.lib.mulls_scan_images_batch(self.h, arr, n, C.byref(rp) if rp is not None else None, C.byref(bp) if bp is not None else None, rptr, bptr, reps)
        if rc != 0:
            self._image_raise(rc, "mulls_scan_images_batch")
        for bufs, npix in ((rbufs, rpix), (bbufs, bpix)):
            assert bufs is None or all(b[npix] == self.GUARD for b in bufs)
        return (None if rbufs is None else [b[:rpix].reshape(rp.height, rp.width).copy() for b in rbufs],
                None if bbufs is None else [b[:bpix].reshape(bp.map_height, bp.map_width).copy() for b in bbufs],
                None if reps is None else [abi.Image2dReport.from_buffer_copy(reps[k]) for k in range(n)])

    def submaps(self, capacity_points, capacity_submaps):
        """a device-resident submap archive (mulls_submaps_*)"""
        return Submaps(self, capacity_points, capacity_submaps)

    # --- stage-level entry points --------------------------------------------------------------------------------
    def motion_compensate(self, pts, Tran, s_ambiguous_thre=0.0):
        """CFilter::apply_motion_compensation on a copy of a host cloud (structured array of 48-byte records)."""
        raw = abi.records(pts).copy()  # every byte of the records kept (a copy of a record array would drop the bytes between its fields)
        Tc = abi.colmajor16(Tran)
        self._check(self.lib.mulls_motion_compensate(self.h, C.c_void_p(raw.ctypes.data), len(raw), abi.POINT_BYTES, Tc, C.c_float(s_ambiguous_thre)), "mulls_motion_compensate")
        return abi.points_of(raw)

    def transform(self, pts, T):
        pts = np.ascontiguousarray(pts).copy()
        Tc = (C.c_double * 16)(*np.asarray(T, dtype=np.float64).T.reshape(-1))
        self._check(self.lib.mulls_stage_transform(self.h, pts.ctypes.data, len(pts), abi.POINT_BYTES, Tc), "mulls_stage_transform")
        return pts

    def correspond(self, src, tgt, dis_thre, normal_check=True, angle_deg=45.0):
        n = len(src)
        match = np.zeros(n, np.int32)
        d2 = np.zeros(n, np.float32)
        flags = np.zeros(n, np.uint8)
        cs, ct = abi.as_cloud(src), abi.as_cloud(tgt)
        self._check(self.lib.mulls_stage_correspond(self.h, C.byref(cs), C.byref(ct), dis_thre, int(normal_check), angle_deg,
                                                    match.ctypes.data, d2.ctypes.data, flags.ctypes.data), "mulls_stage_correspond")
        return match, d2, flags

    def accumulate(self, metric, src, tgt, corr_src, corr_tgt, corr_d2, iter_num, class_weight, dist_w, resid_w, inten_w, window):
        corr_src = np.ascontiguousarray(corr_src, np.int32)
        corr_tgt = np.ascontiguousarray(corr_tgt, np.int32)
        corr_d2 = np.ascontiguousarray(corr_d2, np.float32)
        out = np.zeros(27, np.float64)
        w = np.zeros(len(corr_src), np.float32)
        cs, ct = abi.as_cloud(src), abi.as_cloud(tgt)
        self._check(self.lib.mulls_stage_accumulate(self.h, int(metric), C.byref(cs), C.byref(ct), corr_src.ctypes.data, corr_tgt.ctypes.data,
                                                    corr_d2.ctypes.data, len(corr_src), int(iter_num), class_weight, int(dist_w), int(resid_w),
                                                    int(inten_w), window, out.ctypes.data, w.ctypes.data), "mulls_stage_accumulate")
        return out, w


class Batch:
    """mulls_batch: pairs staged in HBM once, registered any number of times."""

    def __init__(self, ctx, pairs):
        self.ctx = ctx
        self.n = len(pairs)
        self._pairs = pairs  # keep numpy storage alive during create
        arr = abi.make_pair_array(pairs)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.mulls_batch_create(ctx.h, arr, self.n, C.byref(self.h)), "mulls_batch_create")

    def run(self, params, trace_cap=0, results=None):
        res = results if results is not None else abi.make_result_array(self.n, trace_cap)
        self.ctx._check(self.ctx.lib.mulls_batch_run(self.ctx.h, self.h, C.byref(params), res), "mulls_batch_run")
        return res

    def close(self):
        if self.h:
            self.ctx.lib.mulls_batch_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Block:
    """mulls_block: the feature clouds of one scan, device-resident (mulls_extract_features_resident)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        self.n = [0] * abi.EX_COUNT
        ctx._check(ctx.lib.mulls_block_create(ctx.h, C.byref(self.h)), "mulls_block_create")

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.mulls_block_destroy(self.ctx.h, self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def extract(self, scan, params):
        raw_in = abi.records(scan)
        nout = (C.c_uint32 * abi.EX_COUNT)()
        self.ctx._check(self.ctx.lib.mulls_extract_features_resident(self.ctx.h, raw_in.ctypes.data_as(C.c_void_p), len(raw_in), abi.POINT_BYTES, C.byref(params), self.h, nout),
                        "mulls_extract_features_resident")
        self.n = list(nout)
        return self

    def cloud(self, which):
        """device-resident mulls_cloud of cloud `which` (enum mulls_extract_cloud: abi.EX_*)"""
        c = abi.Cloud()
        self.ctx._check(self.ctx.lib.mulls_block_cloud(self.ctx.h, self.h, which, C.byref(c)), "mulls_block_cloud")
        return c

    def download(self, which):
        n = C.c_uint32(0)
        self.ctx._check(self.ctx.lib.mulls_block_download(self.ctx.h, self.h, which, None, 0, C.byref(n)), "mulls_block_download")
        out = np.zeros((n.value, abi.POINT_BYTES), np.uint8)
        if n.value:
            self.ctx._check(self.ctx.lib.mulls_block_download(self.ctx.h, self.h, which, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "mulls_block_download")
        return out

    def motion_compensate(self, Tran, undistort_keypoints=False):
        """the two batch_apply_motion_compensation calls of test/mulls_slam.cpp:706-710 on the block's clouds, in place on the device"""
        self.ctx._check(self.ctx.lib.mulls_block_motion_compensate(self.ctx.h, self.h, abi.colmajor16(Tran), 1 if undistort_keypoints else 0), "mulls_block_motion_compensate")

    def class_clouds(self, down):
        """the six class clouds in the ABI's order (ground, pillar, facade, beam, roof, vertex) as device clouds: the *_down ones (+ pc_vertex) or the full ones"""
        P = abi.EX_PILLAR
        which = [abi.EX_GROUND_DOWN, P + 4, P + 6, P + 5, P + 7, abi.EX_VERTEX] if down else [abi.EX_GROUND, P, P + 2, P + 1, P + 3, abi.EX_VERTEX]
        return [self.cloud(k) for k in which]


class Mapper:
    """mulls_mapper: the merged map mulls_slam exports (test/mulls_slam.cpp:959-1015), device-resident."""

    def __init__(self, ctx, capacity_points):
        self.ctx = ctx
        self.h = C.c_void_p()
        self.last_report, self.last_counts = None, None
        rc = ctx.lib.mulls_mapper_create(ctx.h, int(capacity_points), C.byref(self.h))
        if rc != 0:
            raise MullsError("mulls_mapper_create failed with %d: %s" % (rc, ctx.lib.mulls_last_error(ctx.h).decode()), rc)

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.mulls_mapper_destroy(self.ctx.h, self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def adjacent_tran(pose, pose_before):
        """pose_i^-1 * pose_{i-1} (test/mulls_slam.cpp:979)"""
        return np.linalg.inv(np.asarray(pose, np.float64)) @ np.asarray(pose_before, np.float64)

    @staticmethod
    def marshal(frames):
        """frames as add() takes them -> (mulls_mapper_frame array, what it borrows from)"""
        keep, arr = [], (abi.MapperFrame * max(len(frames), 1))()
        for k, fr in enumerate(frames):
            scan, pose, adj = (tuple(fr) + (None,))[:3]
            if isinstance(scan, abi.Cloud):
                arr[k].scan = scan
            else:
                raw = abi.records(scan)
                keep.append(raw)
                arr[k].scan.pts, arr[k].scan.n, arr[k].scan.stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
            arr[k].pose = abi.colmajor16(pose)
            if adj is not None:
                arr[k].adjacent_tran, arr[k].compensate = abi.colmajor16(adj), 1
        return arr, keep

    def add(self, frames, prep):
        """mulls_mapper_add.  frames: a list of (scan, pose) or (scan, pose, adjacent_tran): scan a host cloud or a device-resident abi.Cloud, adjacent_tran None
        for a frame that is not compensated.  Returns (frame_n_out, report), also kept in last_counts / last_report when the call is refused."""
        arr, keep = self.marshal(frames)
        counts, rep = (C.c_uint32 * max(len(frames), 1))(), abi.MapperReport()
        rc = self.ctx.lib.mulls_mapper_add(self.ctx.h, self.h, arr, len(frames), C.byref(prep), counts, C.byref(rep))
        self.last_counts, self.last_report = list(counts)[: len(frames)], rep
        if rc != 0:
            raise MullsError("mulls_mapper_add failed with %d: %s" % (rc, self.ctx.lib.mulls_last_error(self.ctx.h).decode()), rc)
        return self.last_counts, rep

    def cloud(self):
        """the map as a device-resident mulls_cloud (valid until the next add / clear)"""
        c = abi.Cloud()
        self.ctx._check(self.ctx.lib.mulls_mapper_cloud(self.ctx.h, self.h, C.byref(c)), "mulls_mapper_cloud")
        return c

    def download(self, first=0):
        n = C.c_uint32(0)
        self.ctx._check(self.ctx.lib.mulls_mapper_download(self.ctx.h, self.h, first, None, 0, C.byref(n)), "mulls_mapper_download")
        out = np.zeros((n.value, abi.POINT_BYTES), np.uint8)
        if n.value:
            self.ctx._check(self.ctx.lib.mulls_mapper_download(self.ctx.h, self.h, first, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "mulls_mapper_download")
        return out

    def clear(self):
        self.ctx._check(self.ctx.lib.mulls_mapper_clear(self.ctx.h, self.h), "mulls_mapper_clear")


class Submaps:
    """mulls_submaps: the submaps of the back end in one device arena, their bounds and loop closure's candidate edges."""

    def __init__(self, ctx, capacity_points, capacity_submaps):
        self.ctx = ctx
        self.h = C.c_void_p()
        self.last_info = None
        rc = ctx.lib.mulls_submaps_create(ctx.h, int(capacity_points), int(capacity_submaps), C.byref(self.h))
        if rc != 0:
            raise MullsError("mulls_submaps_create failed with %d: %s" % (rc, ctx.lib.mulls_last_error(ctx.h).decode()), rc)

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.mulls_submaps_destroy(self.ctx.h, self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what):
        if rc != 0:
            raise MullsError("%s failed with %d: %s" % (what, rc, self.ctx.lib.mulls_last_error(self.ctx.h).decode()), rc)

    def push(self, clouds, pose_lo, id_in_strip=0, vertex_nms_radius=0.0):
        """mulls_submaps_push.  clouds: six class clouds in the ABI's order, each a point array, raw (n, 48) records or a device-resident abi.Cloud.
        Returns the abi.SubmapInfo, also kept in last_info when the push is refused."""
        arr, keep = (abi.Cloud * abi.NCLASS)(), []
        for c in range(abi.NCLASS):
            if isinstance(clouds[c], abi.Cloud):
                arr[c] = clouds[c]
            else:
                raw = abi.records(clouds[c] if clouds[c] is not None else np.zeros(0, abi.POINT_DTYPE))
                keep.append(raw)
                arr[c].pts, arr[c].n, arr[c].stride = (raw.ctypes.data if len(raw) else None), len(raw), abi.POINT_BYTES
        info = abi.SubmapInfo()
        rc = self.ctx.lib.mulls_submaps_push(self.ctx.h, self.h, arr, abi.colmajor16(pose_lo), int(id_in_strip), float(vertex_nms_radius), C.byref(info))
        self.last_info = info
        self._raise(rc, "mulls_submaps_push")
        return info

    def push_map(self, local_map, id_in_strip=0, vertex_nms_radius=0.0):
        """mulls_submaps_push_map: a LocalMap's clouds and pose, device to device"""
        info = abi.SubmapInfo()
        rc = self.ctx.lib.mulls_submaps_push_map(self.ctx.h, self.h, local_map.h, int(id_in_strip), float(vertex_nms_radius), C.byref(info))
        self.last_info = info
        self._raise(rc, "mulls_submaps_push_map")
        return info

    def count(self):
        """-> (submaps, points)"""
        n, p = C.c_uint32(0), C.c_uint64(0)
        self._raise(self.ctx.lib.mulls_submaps_count(self.ctx.h, self.h, C.byref(n), C.byref(p)), "mulls_submaps_count")
        return n.value, p.value

    def info(self, sid):
        info = abi.SubmapInfo()
        self._raise(self.ctx.lib.mulls_submaps_info(self.ctx.h, self.h, int(sid), C.byref(info)), "mulls_submaps_info")
        return info

    def cloud(self, sid, which):
        """device-resident mulls_cloud: which = a class (0..5), abi.SUBMAP_MERGED or abi.SUBMAP_MERGED_NO_GROUND; valid until clear / close"""
        c = abi.Cloud()
        self._raise(self.ctx.lib.mulls_submaps_cloud(self.ctx.h, self.h, int(sid), int(which), C.byref(c)), "mulls_submaps_cloud")
        return c

    def download(self, sid, which):
        """raw (n, 48) records of one view"""
        n = C.c_uint32(0)
        self._raise(self.ctx.lib.mulls_submaps_download(self.ctx.h, self.h, int(sid), int(which), None, 0, C.byref(n)), "mulls_submaps_download")
        out = np.zeros((n.value, abi.POINT_BYTES), np.uint8)
        if n.value:
            self._raise(self.ctx.lib.mulls_submaps_download(self.ctx.h, self.h, int(sid), int(which), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "mulls_submaps_download")
        return out

    def clear(self):
        self._raise(self.ctx.lib.mulls_submaps_clear(self.ctx.h, self.h), "mulls_submaps_clear")

    def set_poses(self, first, poses, update_bbx=True):
        """mulls_submaps_set_poses (update_optimized_nodes): poses a sequence of 4 x 4 matrices for submaps first, first + 1, ..."""
        poses = [np.asarray(P, np.float64) for P in poses]
        flat = np.ascontiguousarray(np.concatenate([P.T.reshape(-1) for P in poses]) if poses else np.zeros(0), np.float64)
        self._raise(self.ctx.lib.mulls_submaps_set_poses(self.ctx.h, self.h, int(first), len(poses), flat.ctypes.data_as(C.POINTER(C.c_double)), int(bool(update_bbx))),
                    "mulls_submaps_set_poses")

    def find_overlap(self, query_id, params=None, cap=None):
        """mulls_submaps_find_overlap -> (the first `cap` edges as a list of abi.SubmapEdge, the full count); cap None: all of them"""
        params = abi.overlap_params() if params is None else params
        n = C.c_uint32(0)
        if cap is None:
            self._raise(self.ctx.lib.mulls_submaps_find_overlap(self.ctx.h, self.h, int(query_id), C.byref(params), None, 0, C.byref(n)), "mulls_submaps_find_overlap")
            cap = n.value
        arr = (abi.SubmapEdge * max(int(cap), 1))()
        self._raise(self.ctx.lib.mulls_submaps_find_overlap(self.ctx.h, self.h, int(query_id), C.byref(params), arr, int(cap), C.byref(n)), "mulls_submaps_find_overlap")
        return [arr[k] for k in range(min(int(cap), n.value))], n.value

    def pairs(self, edges):
        """mulls_submaps_pairs: a mulls_pair array for mulls_icp_batch (Context.icp_batch(..., marshalled=(pairs, results)))"""
        arr = (abi.SubmapEdge * max(len(edges), 1))(*edges)
        out = (abi.Pair * max(len(edges), 1))()
        self._raise(self.ctx.lib.mulls_submaps_pairs(self.ctx.h, self.h, arr, len(edges), out), "mulls_submaps_pairs")
        return out


class LocalMap:
    """mulls_map: the six undown class clouds of the reference's local_map cloudblock, kept in HBM between frames."""

    def __init__(self, ctx, clouds=None, pose=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx._check(ctx.lib.mulls_map_create(ctx.h, C.byref(self.h)), "mulls_map_create")
        if clouds is not None:
            self.set(clouds, np.eye(4) if pose is None else pose)

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.mulls_map_destroy(self.ctx.h, self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _clouds(clouds):
        """six clouds, each a point array or an abi.Cloud (a device cloud of a Block / LocalMap)"""
        keep = [c if isinstance(c, abi.Cloud) else abi.as_points(c) for c in clouds]
        arr = (abi.Cloud * abi.NCLASS)()
        for c in range(abi.NCLASS):
            arr[c] = keep[c] if isinstance(keep[c], abi.Cloud) else abi.as_cloud(keep[c])
        return arr, keep

    def set(self, clouds, pose):
        arr, keep = self._clouds(clouds)
        self.ctx._check(self.ctx.lib.mulls_map_set(self.ctx.h, self.h, arr, abi.colmajor16(pose)), "mulls_map_set")

    def update(self, frame_down, frame_pose, params):
        """update_local_map with last_target_cblock = (frame_down[0..4] = pc_*_down, frame_down[5] = pc_vertex, frame_pose)."""
        arr, keep = self._clouds(frame_down)
        rep = abi.MapReport()
        self.ctx._check(self.ctx.lib.mulls_map_update(self.ctx.h, self.h, arr, abi.colmajor16(frame_pose), C.byref(params), C.byref(rep)),
                        "mulls_map_update")
        return rep

    def cloud(self, cls):
        """Device-resident mulls_cloud of class `cls` (usable as a registration target until the next set / update)."""
        c = abi.Cloud()
        self.ctx._check(self.ctx.lib.mulls_map_cloud(self.ctx.h, self.h, cls, C.byref(c)), "mulls_map_cloud")
        return c

    def pose(self):
        m = (C.c_double * 16)()
        self.ctx._check(self.ctx.lib.mulls_map_pose(self.ctx.h, self.h, m), "mulls_map_pose")
        return np.array(m[:]).reshape(4, 4).T.copy()

    def _download(self, fn, name, cls):
        n = C.c_uint32(0)
        self.ctx._check(fn(self.ctx.h, self.h, cls, None, 0, C.byref(n)), name)
        out = np.zeros(n.value, abi.POINT_DTYPE)
        if n.value:
            self.ctx._check(fn(self.ctx.h, self.h, cls, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), name)
        return out

    def download(self, cls):
        return self._download(self.ctx.lib.mulls_map_download, "mulls_map_download", cls)

    def frame_download(self, cls):
        return self._download(self.ctx.lib.mulls_map_frame_download, "mulls_map_frame_download", cls)

    def icp(self, src, params, init_guess=None, tgt_bound=None, trace_cap=0):
        """mm_lls_icp with this map as block1 (target clouds stay on the device) and `src` as block2's six source clouds."""
        keep = [s if isinstance(s, abi.Cloud) else abi.as_points(s) for s in src]
        pair = abi.Pair()
        for c in range(abi.NCLASS):
            pair.tgt[c] = self.cloud(c)
            pair.src[c] = keep[c] if isinstance(keep[c], abi.Cloud) else abi.as_cloud(keep[c])
            pair.src_down[c] = abi.as_cloud(None)
        for k in range(6):
            pair.tgt_bound[k] = float(tgt_bound[k])
        g = np.asarray(np.eye(4) if init_guess is None else init_guess, dtype=np.float64).T.reshape(-1)
        for k in range(16):
            pair.init_guess[k] = float(g[k])
        res = abi.make_result_array(1, trace_cap)
        self.ctx._check(self.ctx.lib.mulls_icp(self.ctx.h, C.byref(pair), C.byref(params), res), "mulls_icp")
        return res
