"""ctypes mirror of include/mulls_hip.h (the C ABI of libmulls_hip.so).

Pure declarations: structs, constants and helpers that turn numpy arrays into ``mulls_cloud`` / ``mulls_pair``
records.  No compute happens here.  The struct layout must stay in lock-step with include/mulls_hip.h
(tests/test_abi.py checks sizes against the compiled library).
"""
import ctypes as C

import numpy as np

NCLASS = 6
POINT_BYTES = 48
GROUND, PILLAR, FACADE, BEAM, ROOF, VERTEX = range(6)
CLASS_NAMES = ("ground", "pillar", "facade", "beam", "roof", "vertex")

MULLS_OK = 0
MULLS_E_INVALID = -100
MULLS_E_HIP = -101
MULLS_E_NO_DEVICE = -102
MULLS_E_UNSUPPORTED = -103
MULLS_E_IO = -104
MULLS_E_NOMEM = -105

# enum mulls_option (slots 1 and 2 are reserved: mulls_set_option / mulls_get_option refuse them)
(OPT_HOST_STEP, _OPT_RESERVED_1, _OPT_RESERVED_2, OPT_FEW_LAUNCHES_MAX_PAIRS, OPT_SUBBATCHES, OPT_TWO_STREAMS, OPT_CERTIFICATES, OPT_CERT_SLACK_MIN,
 OPT_CERT_SLACK_MAX, OPT_CERT_SLACK_RATE, OPT_LDS_DEDUP, OPT_GRID_H0, OPT_BM_H0, OPT_LEAN_STAGING, OPT_DEBUG_STOP, OPT_DEBUG_TICK, OPT_SPLIT_MIN_PAIRS, OPT_SPLIT_MAX_PAIRS,
 OPT_FUSED_TGT_SETUP, OPT_STAGGER, OPT_STEP_LAUNCH_MAX_PAIRS, OPT_MIXED_TIERS, OPT_BIG_EARLY_SETS, OPT_KCERT, OPT_KCERT_MIN, OPT_ACCUM_WAVE_MIN_TRIPS, OPT_FIRST_DIRECT, OPT_SUM_STEP, OPT_TEASER_DEVICE_SEARCH, OPT_COUNT) = range(30)

# numpy view of pcl::PointXYZINormal (48 B)
POINT_DTYPE = np.dtype(
    {
        "names": ["x", "y", "z", "nx", "ny", "nz", "intensity", "curvature"],
        "formats": [np.float32] * 8,
        "offsets": [0, 4, 8, 16, 20, 24, 32, 36],
        "itemsize": POINT_BYTES,
    }
)


class Cloud(C.Structure):
    _fields_ = [("pts", C.c_void_p), ("n", C.c_uint32), ("stride", C.c_uint32)]


class Pair(C.Structure):
    _fields_ = [
        ("tgt", Cloud * NCLASS),
        ("src", Cloud * NCLASS),
        ("src_down", Cloud * NCLASS),
        ("tgt_bound", C.c_double * 6),
        ("init_guess", C.c_double * 16),
    ]


class Params(C.Structure):
    _fields_ = [
        ("max_iter_num", C.c_int32),
        ("dis_thre_unit", C.c_float),
        ("converge_translation", C.c_float),
        ("converge_rotation_d", C.c_float),
        ("dis_thre_min", C.c_float),
        ("dis_thre_update_rate", C.c_float),
        ("used_feature_type", C.c_char * 8),
        ("weight_strategy", C.c_char * 8),
        ("z_xy_balanced_ratio", C.c_float),
        ("pt2pt_residual_window", C.c_float),
        ("pt2pl_residual_window", C.c_float),
        ("pt2li_residual_window", C.c_float),
        ("apply_intersection_filter", C.c_uint8),
        ("apply_motion_undistortion", C.c_uint8),
        ("normal_shooting_on", C.c_uint8),
        ("use_more_points", C.c_uint8),
        ("normal_bearing", C.c_float),
        ("keep_less_source_points", C.c_uint8),
        ("faithful", C.c_uint8),
        ("rejector_strict", C.c_uint8),
        ("reserved_", C.c_uint8),
        ("sigma_thre", C.c_float),
        ("min_neccessary_corr_ratio", C.c_float),
        ("max_bearable_rotation_d", C.c_float),
        ("rng_seed", C.c_uint64),
    ]


class IterTrace(C.Structure):
    _fields_ = [
        ("iter", C.c_int32),
        ("ncorr", C.c_uint32 * NCLASS),
        ("nsrc", C.c_uint32 * NCLASS),
        ("thr", C.c_float * NCLASS),
        ("atpa", C.c_double * 36),
        ("atpb", C.c_double * 6),
        ("x", C.c_double * 6),
    ]


class Result(C.Structure):
    _fields_ = [
        ("code", C.c_int32),
        ("iters", C.c_int32),
        ("T", C.c_double * 16),
        ("info", C.c_double * 36),
        ("sigma", C.c_float),
        ("confidence", C.c_float),
        ("ncorr", C.c_uint32 * NCLASS),
        ("nsrc0", C.c_uint32 * NCLASS),
        ("ntgt0", C.c_uint32 * NCLASS),
        ("singular", C.c_int32),
        ("cropped", C.c_int32),
        ("crop_box", C.c_double * 6),
        ("ms_total", C.c_float),
        ("trace", C.POINTER(IterTrace)),
        ("trace_cap", C.c_int32),
        ("trace_len", C.c_int32),
    ]

    # convenience views (row-major numpy matrices)
    def T_matrix(self):
        return np.array(self.T[:], dtype=np.float64).reshape(4, 4).T.copy()

    def info_matrix(self):
        return np.array(self.info[:], dtype=np.float64).reshape(6, 6).T.copy()



class MapParams(C.Structure):
    """mulls_map_params: MapManager::update_local_map's positional arguments (map_manager.h:21-31) + seed + tree state."""
    _fields_ = [
        ("local_map_radius", C.c_float),
        ("max_num_pts", C.c_int32),
        ("kept_vertex_num", C.c_int32),
        ("last_frame_reliable_radius", C.c_float),
        ("map_based_dynamic_removal_on", C.c_int32),
        ("used_feature_type", C.c_char * 8),
        ("dynamic_removal_center_radius", C.c_float),
        ("dynamic_dist_thre_min", C.c_float),
        ("dynamic_dist_thre_max", C.c_float),
        ("near_dist_thre", C.c_float),
        ("recalculate_feature_on", C.c_int32),
        ("rng_seed", C.c_uint64),
        ("tree_mode", C.c_int32),
        ("tree_used", C.c_char * 8),
        ("tree_box", C.c_double * 6),
    ]


class MapReport(C.Structure):
    _fields_ = [
        ("n", C.c_uint32 * NCLASS),
        ("frame_n", C.c_uint32 * NCLASS),
        ("feature_point_num", C.c_int32),
        ("dynamic_removal_ran", C.c_int32),
        ("local_bound", C.c_double * 6),
        ("bound", C.c_double * 6),
        ("ms_total", C.c_float),
    ]


class MapUpdateItem(C.Structure):
    """mulls_map_update_item: one map's update inside mulls_map_update_batch"""

    _fields_ = [("map", C.c_void_p), ("frame_down", C.POINTER(Cloud)), ("frame_pose_lo", C.c_double * 16), ("params", C.POINTER(MapParams))]


class MapBatchResult(C.Structure):
    """mulls_map_batch_result"""

    _fields_ = [("status", C.c_int32), ("path", C.c_uint32), ("report", MapReport)]


class MapBatchStats(C.Structure):
    """mulls_map_batch_stats"""

    _fields_ = [("n_groups", C.c_uint32), ("n_lockstep", C.c_uint32), ("n_single_path", C.c_uint32), ("n_kernel_launches", C.c_uint32), ("n_syncs", C.c_uint32)]


def map_params(**kw):
    """update_local_map defaults (map_manager.h:21-31), overridden by keyword."""
    p = MapParams()
    p.local_map_radius, p.max_num_pts, p.kept_vertex_num, p.last_frame_reliable_radius = 80.0, 20000, 800, 60.0
    p.map_based_dynamic_removal_on = 0
    p.used_feature_type = b"111110"
    p.dynamic_removal_center_radius, p.dynamic_dist_thre_min, p.dynamic_dist_thre_max, p.near_dist_thre = 30.0, 0.3, 3.0, 0.03
    p.recalculate_feature_on, p.rng_seed, p.tree_mode, p.tree_used = 0, 0, 0, b"000000"
    for k, v in kw.items():
        if k == "tree_box":
            for i in range(6):
                p.tree_box[i] = float(v[i])
        elif k in ("used_feature_type", "tree_used"):
            setattr(p, k, v.encode() if isinstance(v, str) else v)
        else:
            setattr(p, k, v)
    return p


def colmajor16(M):
    return (C.c_double * 16)(*np.asarray(M, dtype=np.float64).T.reshape(-1))

class GroundParams(C.Structure):
    _fields_ = [
        ("min_grid_pt_num", C.c_int32),
        ("grid_resolution", C.c_float),
        ("max_height_difference", C.c_float),
        ("neighbor_height_diff", C.c_float),
        ("max_ground_height", C.c_float),
        ("ground_random_down_rate", C.c_int32),
        ("ground_random_down_down_rate", C.c_int32),
        ("nonground_random_down_rate", C.c_int32),
        ("reliable_neighbor_grid_num_thre", C.c_int32),
        ("estimate_ground_normal_method", C.c_int32),
        ("distance_weight_downsampling_method", C.c_int32),
        ("standard_distance", C.c_float),
        ("fixed_num_downsampling", C.c_uint8),
        ("apply_grid_wise_outlier_filter", C.c_uint8),
        ("reserved_", C.c_uint8 * 2),
        ("down_ground_fixed_num", C.c_int32),
        ("intensity_thre", C.c_float),
        ("outlier_std_scale", C.c_float),
        ("normal_estimation_radius", C.c_float),
        ("reserved2_", C.c_uint32),
        ("rng_seed", C.c_uint64),
    ]


def ground_params(**overrides):
    """fast_ground_filter's arguments as extract_semantic_pts passes them with script/config/lo_gflag_list_kitti_urban.txt, except
    the ground normal method (0 instead of the RANSAC of method 3) and the distance-inverse sampling (0 instead of 2)."""
    p = GroundParams()
    kw = dict(min_grid_pt_num=6, grid_resolution=2.5, max_height_difference=0.25, neighbor_height_diff=1.5, max_ground_height=2.0,
              ground_random_down_rate=12, ground_random_down_down_rate=3, nonground_random_down_rate=3, reliable_neighbor_grid_num_thre=0,
              estimate_ground_normal_method=0, distance_weight_downsampling_method=0, standard_distance=15.0, fixed_num_downsampling=0,
              apply_grid_wise_outlier_filter=0, down_ground_fixed_num=800, intensity_thre=150.0, outlier_std_scale=3.0, normal_estimation_radius=2.0,
              rng_seed=0)
    kw.update(overrides)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class ClassifyParams(C.Structure):
    _fields_ = [
        ("neighbor_searching_radius", C.c_float),
        ("neighbor_k", C.c_int32),
        ("neigh_k_min", C.c_int32),
        ("pca_down_rate", C.c_int32),
        ("edge_thre", C.c_float),
        ("planar_thre", C.c_float),
        ("edge_thre_down", C.c_float),
        ("planar_thre_down", C.c_float),
        ("extract_vertex_points_method", C.c_int32),
        ("curvature_thre", C.c_float),
        ("vertex_curvature_non_max_radius", C.c_float),
        ("linear_vertical_sin_high_thre", C.c_float),
        ("linear_vertical_sin_low_thre", C.c_float),
        ("planar_vertical_sin_high_thre", C.c_float),
        ("planar_vertical_sin_low_thre", C.c_float),
        ("fixed_num_downsampling", C.c_uint8),
        ("sharpen_with_nms", C.c_uint8),
        ("use_distance_adaptive_pca", C.c_uint8),
        ("reserved_", C.c_uint8),
        ("pillar_down_fixed_num", C.c_int32),
        ("facade_down_fixed_num", C.c_int32),
        ("beam_down_fixed_num", C.c_int32),
        ("roof_down_fixed_num", C.c_int32),
        ("unground_down_fixed_num", C.c_int32),
        ("beam_height_max", C.c_float),
        ("roof_height_min", C.c_float),
        ("feature_pts_ratio_guess", C.c_float),
        ("rng_seed", C.c_uint64),
    ]


CL_PILLAR, CL_BEAM, CL_FACADE, CL_ROOF, CL_PILLAR_DOWN, CL_BEAM_DOWN, CL_FACADE_DOWN, CL_ROOF_DOWN, CL_VERTEX, CL_COUNT = range(10)
CL_NAMES = ("pillar", "beam", "facade", "roof", "pillar_down", "beam_down", "facade_down", "roof_down", "vertex")


def classify_params(**overrides):
    """classify_nground_pts's arguments as extract_semantic_pts passes them for script/run_mulls_reg.sh (mulls_classify_default_params)."""
    p = ClassifyParams()
    kw = dict(neighbor_searching_radius=1.0, neighbor_k=50, neigh_k_min=8, pca_down_rate=1, edge_thre=0.65, planar_thre=0.65, edge_thre_down=0.75,
              planar_thre_down=0.75, extract_vertex_points_method=2, curvature_thre=0.10, vertex_curvature_non_max_radius=1.5,
              linear_vertical_sin_high_thre=0.94, linear_vertical_sin_low_thre=0.17, planar_vertical_sin_high_thre=0.98,
              planar_vertical_sin_low_thre=0.34, fixed_num_downsampling=0, sharpen_with_nms=1, use_distance_adaptive_pca=0, pillar_down_fixed_num=200,
              facade_down_fixed_num=800, beam_down_fixed_num=200, roof_down_fixed_num=200, unground_down_fixed_num=20000,
              beam_height_max=3.4028234663852886e38, roof_height_min=0.0, feature_pts_ratio_guess=0.3, rng_seed=0)
    kw.update(overrides)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class ExtractParams(C.Structure):
    _fields_ = [
        ("ground", GroundParams),
        ("classify", ClassifyParams),
        ("apply_scanner_filter", C.c_uint8),
        ("apply_dist_filter", C.c_uint8),
        ("reserved_", C.c_uint8 * 2),
        ("self_ring_radius", C.c_float),
        ("ghost_radius", C.c_float),
        ("z_min", C.c_float),
        ("z_min_min", C.c_float),
        ("vf_downsample_resolution", C.c_float),
        ("min_dist_used", C.c_double),
        ("max_dist_used", C.c_double),
    ]


EX_RAW, EX_GROUND, EX_GROUND_DOWN, EX_UNGROUND, EX_PILLAR, EX_VERTEX, EX_DOWN, EX_COUNT = 0, 1, 2, 3, 4, 12, 13, 14


class ExtractBatchResult(C.Structure):
    """mulls_extract_batch_result: one scan of mulls_extract_features_batch"""

    _fields_ = [("status", C.c_int32), ("path", C.c_uint32), ("n_out", C.c_uint32 * EX_COUNT)]


class ExtractBatchStats(C.Structure):
    """mulls_extract_batch_stats"""

    _fields_ = [("n_subbatches", C.c_uint32), ("n_lockstep", C.c_uint32), ("n_single_path", C.c_uint32), ("n_kernel_launches", C.c_uint32), ("n_syncs", C.c_uint32),
                ("promote_rounds", C.c_uint32), ("nms_rounds", C.c_uint32)]


EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES = 12 << 30  # MULLS_EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES


def extract_params(ground=None, classify=None, apply_scanner_filter=0, approx_scanner_height=2.0, underground_thre=-7.0, apply_dist_filter=0,
                   min_dist_used=1.0, max_dist_used=120.0, vf_downsample_resolution=0.0):
    """The frame front end: dist_filter (test/mulls_slam.cpp:359-360) -> scanner filter (cfilter.hpp:2338-2346) -> voxel_downsample ->
    fast_ground_filter -> classify_nground_pts."""
    p = ExtractParams()
    p.ground = ground if ground is not None else ground_params()
    p.classify = classify if classify is not None else classify_params()
    p.apply_scanner_filter = apply_scanner_filter
    p.self_ring_radius, p.ghost_radius = 1.75, 20.0
    p.z_min = np.float32(-np.float32(approx_scanner_height) - 4.0)
    p.z_min_min = np.float32(-np.float32(approx_scanner_height) + np.float32(underground_thre))
    p.apply_dist_filter = apply_dist_filter
    p.min_dist_used, p.max_dist_used = min_dist_used, max_dist_used
    p.vf_downsample_resolution = vf_downsample_resolution
    return p


class NccParams(C.Structure):
    """mulls_ncc_params: find_feature_correspondence_ncc's arguments behind the clouds (cregistration.hpp:411)"""

    _fields_ = [("fixed_num_corr", C.c_int32), ("corr_num", C.c_int32), ("reciprocal_on", C.c_int32), ("reserved", C.c_int32)]


def ncc_params(fixed_num_corr=0, corr_num=2000, reciprocal_on=1):
    p = NccParams()
    p.fixed_num_corr, p.corr_num, p.reciprocal_on = int(fixed_num_corr), int(corr_num), int(reciprocal_on)
    return p


class NccProblem(C.Structure):
    """mulls_ncc_problem: one problem of mulls_ncc_correspond_batch"""

    _fields_ = [("tgt", Cloud), ("src", Cloud), ("tgt_idx", C.c_void_p), ("src_idx", C.c_void_p), ("cap", C.c_uint32), ("reserved", C.c_uint32)]


class NccResult(C.Structure):
    """mulls_ncc_result"""

    _fields_ = [("ret", C.c_int32), ("n_corr", C.c_uint32)]


NCC_BATCH_DEFAULT_SCRATCH_BYTES = 512 << 20  # MULLS_NCC_BATCH_DEFAULT_SCRATCH_BYTES


class RansacParams(C.Structure):
    """mulls_ransac_params: coarse_reg_ransac's arguments behind the clouds (cregistration.hpp:607), and upstream's setRefineModel(true)"""

    _fields_ = [("noise_bound", C.c_float), ("min_inlier_num", C.c_int32), ("max_iter_num", C.c_int32), ("refine", C.c_int32)]


class RansacResult(C.Structure):
    """mulls_ransac_result"""

    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("best_iteration", C.c_int32), ("refine_iterations", C.c_int32),
                ("n_inliers", C.c_uint32), ("T", C.c_double * 16)]


def ransac_params(noise_bound=0.2, min_inlier_num=8, max_iter_num=20000, refine=1):
    p = RansacParams()
    p.noise_bound, p.min_inlier_num, p.max_iter_num, p.refine = float(noise_bound), int(min_inlier_num), int(max_iter_num), int(refine)
    return p


class RansacProblem(C.Structure):
    """mulls_ransac_problem: one problem of mulls_coarse_reg_ransac_batch"""

    _fields_ = [("tgt", Cloud), ("src", Cloud), ("tgt_idx", C.c_void_p), ("src_idx", C.c_void_p), ("n_corr", C.c_uint32), ("inlier_cap", C.c_uint32),
                ("inliers", C.c_void_p)]


RANSAC_BATCH_DEFAULT_SCRATCH_BYTES = 512 << 20  # MULLS_RANSAC_BATCH_DEFAULT_SCRATCH_BYTES


class TeaserParams(C.Structure):
    """mulls_teaser_params: coarse_reg_teaser's arguments behind the clouds (cregistration.hpp:666), and the clique search's node budget"""

    _fields_ = [("noise_bound", C.c_float), ("min_inlier_num", C.c_int32), ("clique_node_budget", C.c_uint64)]


class TeaserResult(C.Structure):
    """mulls_teaser_result"""

    _fields_ = [("status", C.c_int32), ("max_core", C.c_int32), ("n_edges", C.c_uint64), ("clique_size", C.c_int32), ("clique_exact", C.c_int32),
                ("clique_nodes", C.c_uint64), ("gnc_iterations", C.c_int32), ("n_rotation_inliers", C.c_int32), ("n_translation_inliers", C.c_int32),
                ("reserved", C.c_int32), ("cost", C.c_double), ("search_seconds", C.c_double), ("T", C.c_double * 16)]


class TeaserProblem(C.Structure):
    """mulls_teaser_problem: one problem of mulls_coarse_reg_teaser_batch"""

    _fields_ = [("tgt", Cloud), ("src", Cloud), ("tgt_idx", C.c_void_p), ("src_idx", C.c_void_p), ("n_corr", C.c_uint32), ("clique_cap", C.c_uint32),
                ("clique", C.c_void_p)]


TEASER_DEFAULT_NODE_BUDGET = 1 << 28  # MULLS_TEASER_DEFAULT_NODE_BUDGET
TEASER_BATCH_DEFAULT_SCRATCH_BYTES = 512 << 20  # MULLS_TEASER_BATCH_DEFAULT_SCRATCH_BYTES


def teaser_params(noise_bound=0.2, min_inlier_num=8, clique_node_budget=TEASER_DEFAULT_NODE_BUDGET):
    p = TeaserParams()
    p.noise_bound, p.min_inlier_num, p.clique_node_budget = float(noise_bound), int(min_inlier_num), int(clique_node_budget)
    return p


class SorParams(C.Structure):
    """mulls_sor_params: sor_filter's arguments behind the cloud (cfilter.hpp:204)"""

    _fields_ = [("mean_k", C.c_int32), ("reserved", C.c_int32), ("std_mul", C.c_double)]


class SorReport(C.Structure):
    """mulls_sor_report"""

    _fields_ = [("n_in", C.c_uint32), ("n_kept", C.c_uint32), ("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double),
                ("ms_total", C.c_float), ("n_fallback", C.c_uint32)]


def sor_params(mean_k=20, std_mul=2.0):
    p = SorParams()
    p.mean_k, p.reserved, p.std_mul = int(mean_k), 0, float(std_mul)
    return p


class PgoNode(C.Structure):
    """mulls_pgo_node: cloudblock_t's pose_init (column-major), pose_fixed, pose_stable"""

    _fields_ = [("pose_init", C.c_double * 16), ("fixed", C.c_uint8), ("stable", C.c_uint8), ("reserved", C.c_uint8 * 6)]


class PgoEdge(C.Structure):
    """mulls_pgo_edge: constraint_t's block ids, con_type, Trans1_2 and information_matrix (column-major)"""

    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("type", C.c_int32), ("reserved", C.c_int32), ("T", C.c_double * 16), ("info", C.c_double * 36)]


class PgoParams(C.Structure):
    """mulls_pgo_params"""

    _fields_ = [("num_iterations", C.c_int32), ("robustify", C.c_uint8), ("use_equal_weight", C.c_uint8), ("use_diagonal_information_matrix", C.c_uint8),
                ("free_all_nodes", C.c_uint8), ("only_limit_translation", C.c_uint8), ("reserved0", C.c_uint8 * 3), ("robust_delta", C.c_float),
                ("quat_tran_ratio", C.c_float), ("reserved1", C.c_int32), ("t_limit", C.c_double), ("r_limit", C.c_double), ("function_tolerance", C.c_double),
                ("wrong_edge_translation_thre", C.c_float), ("wrong_edge_rotation_thre", C.c_float), ("wrong_edge_ratio_thre", C.c_float),
                ("reserved2", C.c_uint32)]


class PgoResult(C.Structure):
    """mulls_pgo_result"""

    _fields_ = [("status", C.c_int32), ("termination", C.c_int32), ("iterations", C.c_int32), ("successful_steps", C.c_int32), ("n_free", C.c_uint32),
                ("n_boxed", C.c_uint32), ("n_fixed", C.c_uint32), ("n_edges_used", C.c_uint32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("wrong_edges", C.c_int32), ("correct_reg_edges", C.c_int32), ("edges_ok", C.c_int32), ("reserved", C.c_int32)]


class PgoProblem(C.Structure):
    """mulls_pgo_problem: one problem of mulls_pgo_optimize_batch"""

    _fields_ = [("nodes", C.c_void_p), ("n_nodes", C.c_uint32), ("edges", C.c_void_p), ("n_edges", C.c_uint32), ("poses_out", C.c_void_p),
                ("edge_wrong", C.c_void_p)]


PGO_REGISTRATION, PGO_ADJACENT, PGO_HISTORY, PGO_SMOOTH, PGO_NONE = range(5)  # enum mulls_pgo_edge_type
(PGO_TERM_NOT_RUN, PGO_TERM_MAX_ITERATIONS, PGO_TERM_FUNCTION_TOLERANCE, PGO_TERM_GRADIENT, PGO_TERM_STEP, PGO_TERM_RADIUS,
 PGO_TERM_NO_FREE) = range(7)  # enum mulls_pgo_termination
PGO_MAX_NODES, PGO_MAX_EDGES, PGO_MAX_BLOCKS = 4096, 131072, 262144
PGO_BATCH_DEFAULT_SCRATCH_BYTES = 256 << 20  # MULLS_PGO_BATCH_DEFAULT_SCRATCH_BYTES


def pgo_params(**kw):
    """mulls_pgo_default_params' values, then the keyword arguments"""
    p = PgoParams()
    p.num_iterations, p.robust_delta, p.quat_tran_ratio, p.t_limit, p.r_limit, p.function_tolerance = 100, 1.0, 1000.0, 2.0, 0.05, 1e-16
    p.wrong_edge_translation_thre, p.wrong_edge_rotation_thre, p.wrong_edge_ratio_thre = 5.0, 25.0, 0.1
    for k, v in kw.items():
        getattr(p, k)
        setattr(p, k, v)
    return p


def pgo_nodes(poses, fixed, stable):
    """poses (n, 4, 4) row-major numpy matrices -> an array of mulls_pgo_node"""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    arr = (PgoNode * max(len(poses), 1))()
    for i, T in enumerate(poses):
        arr[i].pose_init[:] = T.T.reshape(-1).tolist()
        arr[i].fixed, arr[i].stable = int(bool(fixed[i])), int(bool(stable[i]))
    return arr


def pgo_edges(edges):
    """a list of (a, b, type, T (4, 4), info (6, 6)) -> an array of mulls_pgo_edge"""
    arr = (PgoEdge * max(len(edges), 1))()
    for k, (a, b, typ, T, info) in enumerate(edges):
        arr[k].a, arr[k].b, arr[k].type = int(a), int(b), int(typ)
        arr[k].T[:] = np.asarray(T, np.float64).reshape(4, 4).T.reshape(-1).tolist()
        arr[k].info[:] = np.asarray(info, np.float64).reshape(6, 6).T.reshape(-1).tolist()
    return arr


class NdtParams(C.Structure):
    """mulls_ndt_params"""

    _fields_ = [("resolution", C.c_float), ("search_method", C.c_int32), ("apply_intersection_filter", C.c_int32), ("fitness_score_thre", C.c_float),
                ("scratch_limit_bytes", C.c_uint64), ("step_size", C.c_double), ("transformation_epsilon", C.c_double), ("outlier_ratio", C.c_double),
                ("min_covar_eigvalue_mult", C.c_double), ("max_iterations", C.c_int32), ("max_step_iterations", C.c_int32),
                ("min_points_per_voxel", C.c_int32), ("reserved", C.c_int32)]


class NdtProblem(C.Structure):
    """mulls_ndt_problem"""

    _fields_ = [("tgt", Cloud), ("src", Cloud), ("tgt_bound", C.c_double * 6), ("src_bound", C.c_double * 6), ("init_guess", C.c_double * 16)]


class NdtResult(C.Structure):
    """mulls_ndt_result"""

    _fields_ = [("code", C.c_int32), ("iterations", C.c_int32), ("evaluations", C.c_int32), ("converged", C.c_int32), ("n_leaves", C.c_uint32),
                ("n_leaves_used", C.c_uint32), ("n_src", C.c_uint32), ("n_tgt", C.c_uint32), ("T", C.c_double * 16), ("fitness", C.c_double),
                ("trans_probability", C.c_double), ("gauss_d1", C.c_double), ("gauss_d2", C.c_double), ("gauss_d3", C.c_double),
                ("line_search_reversals", C.c_int32), ("inner_steps", C.c_int32)]


NDT_KDTREE, NDT_DIRECT26, NDT_DIRECT7, NDT_DIRECT1 = range(4)  # enum mulls_ndt_search
NDT_TREE = 4096  # MULLS_NDT_TREE


def ndt_params(**kw):
    """mulls_ndt_default_params' values, then the keyword arguments"""
    p = NdtParams()
    p.resolution, p.search_method, p.apply_intersection_filter, p.fitness_score_thre = 1.0, NDT_DIRECT7, 1, 10.0
    p.step_size, p.transformation_epsilon, p.outlier_ratio, p.min_covar_eigvalue_mult = 0.1, 0.1, 0.55, 0.01
    p.max_iterations, p.max_step_iterations, p.min_points_per_voxel = 35, 10, 6
    for k, v in kw.items():
        getattr(p, k)
        setattr(p, k, v)
    return p


class GicpParams(C.Structure):
    """mulls_gicp_params"""

    _fields_ = [("voxel_resolution", C.c_float), ("k_correspondences", C.c_int32), ("max_iterations", C.c_int32), ("apply_intersection_filter", C.c_int32),
                ("rotation_epsilon", C.c_double), ("transformation_epsilon", C.c_double), ("fitness_score_thre", C.c_float), ("using_voxel_gicp", C.c_int32),
                ("start_rotvec", C.c_float * 3), ("reserved", C.c_int32), ("scratch_limit_bytes", C.c_uint64)]


GicpProblem = NdtProblem  # mulls_gicp_problem is mulls_ndt_problem


class GicpResult(C.Structure):
    """mulls_gicp_result"""

    _fields_ = [("code", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32), ("stop", C.c_int32), ("n_src", C.c_uint32), ("n_tgt", C.c_uint32),
                ("n_voxels", C.c_uint32), ("n_corr", C.c_uint32), ("T", C.c_double * 16), ("fitness", C.c_double), ("loss", C.c_double)]


GICP_STOP_NONE, GICP_STOP_CONVERGED, GICP_STOP_MAX_ITERATIONS, GICP_STOP_SINGULAR = range(4)  # enum mulls_gicp_stop


def gicp_params(**kw):
    """mulls_gicp_default_params' values, then the keyword arguments (start_rotvec: three numbers)"""
    p = GicpParams()
    p.voxel_resolution, p.k_correspondences, p.max_iterations, p.apply_intersection_filter = 1.0, 20, 64, 0
    p.rotation_epsilon, p.transformation_epsilon, p.fitness_score_thre, p.using_voxel_gicp = 2e-3, 5e-4, 10.0, 1
    p.start_rotvec[:] = [0.005773503] * 3
    for k, v in kw.items():
        getattr(p, k)
        if k == "start_rotvec":
            p.start_rotvec[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


class PclIcpParams(C.Structure):
    """mulls_pcl_icp_params"""

    _fields_ = [("max_iter_num", C.c_int32), ("dis_thre_unit", C.c_float), ("metrics", C.c_int32), ("ce", C.c_int32), ("te", C.c_int32),
                ("use_reciprocal_correspondence", C.c_int32), ("use_trimmed_rejector", C.c_int32), ("neighbor_radius", C.c_float),
                ("apply_intersection_filter", C.c_int32), ("fitness_score_thre", C.c_float), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double), ("scratch_limit_bytes", C.c_uint64)]


PclIcpProblem = NdtProblem  # mulls_pcl_icp_problem is mulls_ndt_problem


class PclIcpResult(C.Structure):
    """mulls_pcl_icp_result"""

    _fields_ = [("code", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32), ("stop", C.c_int32), ("n_src", C.c_uint32), ("n_tgt", C.c_uint32),
                ("n_corr", C.c_uint32), ("n_fit", C.c_uint32), ("mse", C.c_double), ("T", C.c_double * 16), ("fitness", C.c_double)]


PCL_ICP_POINT2POINT, PCL_ICP_POINT2PLANE, PCL_ICP_PLANE2PLANE = range(3)  # enum mulls_pcl_icp_metric
PCL_ICP_NN, PCL_ICP_NS = range(2)  # enum mulls_pcl_icp_ce
PCL_ICP_SVD, PCL_ICP_LM, PCL_ICP_LLS = range(3)  # enum mulls_pcl_icp_te
(PCL_ICP_STOP_NONE, PCL_ICP_STOP_ITERATIONS, PCL_ICP_STOP_TRANSFORM, PCL_ICP_STOP_ABS_MSE, PCL_ICP_STOP_REL_MSE, PCL_ICP_STOP_NO_CORRESPONDENCES,
 PCL_ICP_STOP_SINGULAR) = range(7)  # enum mulls_pcl_icp_stop


def pcl_icp_params(**kw):
    """mulls_pcl_icp_default_params' values, then the keyword arguments"""
    p = PclIcpParams()
    p.max_iter_num, p.dis_thre_unit, p.metrics, p.ce, p.te = 20, 1.5, PCL_ICP_POINT2POINT, PCL_ICP_NN, PCL_ICP_SVD
    p.neighbor_radius, p.apply_intersection_filter, p.fitness_score_thre = 2.0, 1, 10.0
    p.transformation_epsilon, p.euclidean_fitness_epsilon = 1e-8, 1e-5
    for k, v in kw.items():
        getattr(p, k)
        setattr(p, k, v)
    return p


class FpfhParams(C.Structure):
    """mulls_fpfh_params"""

    _fields_ = [("search_radius", C.c_float), ("reserved", C.c_int32)]


class FpfhSacParams(C.Structure):
    """mulls_fpfhsac_params"""

    _fields_ = [("search_radius", C.c_float), ("nr_samples", C.c_int32), ("k_correspondences", C.c_int32), ("max_iterations", C.c_int32),
                ("min_sample_distance", C.c_float), ("max_correspondence_distance", C.c_float), ("error_function", C.c_int32), ("seed", C.c_uint32)]


class FpfhSacResult(C.Structure):
    """mulls_fpfhsac_result"""

    _fields_ = [("best_iteration", C.c_int32), ("iterations", C.c_int32), ("n_src", C.c_uint32), ("n_tgt", C.c_uint32), ("best_error", C.c_double),
                ("fitness", C.c_double), ("T", C.c_double * 16)]


class FpfhSacProblem(C.Structure):
    """mulls_fpfhsac_problem"""

    _fields_ = [("tgt", Cloud), ("src", Cloud)]


SACIA_TRUNCATED, SACIA_HUBER = range(2)  # enum mulls_sacia_error
FPFHSAC_BATCH_DEFAULT_SCRATCH_BYTES = 1024 << 20  # MULLS_FPFHSAC_BATCH_DEFAULT_SCRATCH_BYTES
FPFH_DIMS = 33
FPFH_MAX_CELL_POINTS = 16384  # MULLS_FPFH_MAX_CELL_POINTS
FPFH_HYP_CHUNK = 1024  # MULLS_FPFH_HYP_CHUNK (csrc/fpfh_launch.h): hypotheses whose nearest-target distances are held at a time


def fpfh_params(search_radius=1.0):
    """mulls_fpfh_default_params' values, then the argument"""
    p = FpfhParams()
    p.search_radius = search_radius
    return p


def fpfhsac_params(**kw):
    """mulls_fpfhsac_default_params' values, then the keyword arguments"""
    p = FpfhSacParams()
    p.search_radius, p.nr_samples, p.k_correspondences, p.max_iterations = 1.0, 3, 15, 10
    p.min_sample_distance, p.max_correspondence_distance, p.error_function, p.seed = 0.0, float("inf"), SACIA_TRUNCATED, 0
    for k, v in kw.items():
        getattr(p, k)
        setattr(p, k, v)
    return p


class NmsParams(C.Structure):
    """mulls_nms_params: non_max_suppress' radius (cfilter.hpp:1183) and which path runs it"""

    _fields_ = [("non_max_radius", C.c_float), ("path", C.c_int32)]


class NmsReport(C.Structure):
    """mulls_nms_report"""

    _fields_ = [("n_in", C.c_uint32), ("n_kept", C.c_uint32), ("ran", C.c_int32), ("path", C.c_int32), ("rounds", C.c_uint32), ("ms_total", C.c_float)]


NMS_MAX_POINTS = 1 << 18  # MULLS_NMS_MAX_POINTS
NMS_LDS_MAX_POINTS = 4096  # MULLS_NMS_LDS_MAX_POINTS: the one-workgroup path's limit


class NmsProblem(C.Structure):
    """mulls_nms_problem: one problem of mulls_non_max_suppress_batch"""

    _fields_ = [("cloud", Cloud), ("out", C.c_void_p), ("kept_idx", C.c_void_p), ("order", C.c_void_p), ("cap", C.c_uint32), ("idx_cap", C.c_uint32)]


NMS_BATCH_DEFAULT_SCRATCH_BYTES = 512 << 20  # MULLS_NMS_BATCH_DEFAULT_SCRATCH_BYTES


def nms_params(non_max_radius=0.25, path=0):
    p = NmsParams()
    p.non_max_radius, p.path = float(non_max_radius), int(path)
    return p


class ScanPrepParams(C.Structure):
    """mulls_scan_prep_params: the raw-scan steps of CFilter in front of the feature extraction and of the map export"""

    _fields_ = [("calib_on", C.c_uint8), ("dist_filter_on", C.c_uint8), ("calib_first", C.c_uint8), ("reserved_", C.c_uint8), ("downsample_ratio", C.c_int32),
                ("timestamp_mode", C.c_int32), ("scan_duration_ms", C.c_float), ("vertical_ang_correction_deg", C.c_double), ("min_dist", C.c_double),
                ("max_dist", C.c_double), ("scan_begin_ang_deg", C.c_double)]


class ScanPrepReport(C.Structure):
    """mulls_scan_prep_report"""

    _fields_ = [("n_in", C.c_uint32), ("n_after_dist", C.c_uint32), ("n_out", C.c_uint32), ("reserved", C.c_uint32), ("first_timestamp", C.c_double),
                ("last_timestamp", C.c_double), ("scan_duration_used", C.c_float), ("ms_total", C.c_float)]


class MapperFrame(C.Structure):
    """mulls_mapper_frame: one frame of the merged map (test/mulls_slam.cpp:963-990)"""

    _fields_ = [("scan", Cloud), ("pose", C.c_double * 16), ("adjacent_tran", C.c_double * 16), ("compensate", C.c_int32), ("reserved", C.c_int32)]


class MapperReport(C.Structure):
    """mulls_mapper_report"""

    _fields_ = [("frames_added", C.c_uint32), ("n_before", C.c_uint32), ("n_after", C.c_uint32), ("reserved", C.c_uint32), ("n_needed", C.c_uint64),
                ("ms_total", C.c_float), ("reserved2", C.c_uint32)]


SCAN_CHUNK = 256  # MULLS_SCAN_CHUNK
SCAN_MAX_POINTS = 1 << 24  # MULLS_SCAN_MAX_POINTS


def scan_prep_params(calib_on=0, dist_filter_on=0, calib_first=0, downsample_ratio=1, timestamp_mode=0, scan_duration_ms=100.0, vertical_ang_correction_deg=0.0,
                     min_dist=1.0, max_dist=120.0, scan_begin_ang_deg=180.0):
    """upstream's defaults (cfilter.hpp:250, :414; test/mulls_slam.cpp:52-53)"""
    p = ScanPrepParams()
    p.calib_on, p.dist_filter_on, p.calib_first, p.reserved_ = int(calib_on), int(dist_filter_on), int(calib_first), 0
    p.downsample_ratio, p.timestamp_mode, p.scan_duration_ms = int(downsample_ratio), int(timestamp_mode), float(scan_duration_ms)
    p.vertical_ang_correction_deg, p.min_dist, p.max_dist, p.scan_begin_ang_deg = float(vertical_ang_correction_deg), float(min_dist), float(max_dist), float(scan_begin_ang_deg)
    return p


class Image2dParams(C.Structure):
    """mulls_image2d_params: generate_2d_map's arguments (cfilter.hpp:2751-2752) and which form of the counting pass runs"""

    _fields_ = [("m2pix", C.c_double), ("map_width", C.c_int32), ("map_height", C.c_int32), ("min_points_in_pix", C.c_int32), ("max_points_in_pix", C.c_int32),
                ("min_height", C.c_double), ("max_height", C.c_double), ("shift", C.c_int32), ("count_form", C.c_int32)]


class Image2dReport(C.Structure):
    """mulls_image2d_report"""

    _fields_ = [("centre", C.c_double * 3), ("n_counted", C.c_uint32), ("n_skipped_height", C.c_uint32), ("n_skipped_frame", C.c_uint32), ("ms_total", C.c_float)]


class RangeImageParams(C.Structure):
    """mulls_range_image_params: pointcloud_to_rangeimage's constants (cfilter.hpp:2717-2721)"""

    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("f_up_deg", C.c_float), ("f_down_deg", C.c_float), ("max_distance", C.c_float), ("reserved", C.c_int32)]


IMAGE_MAX_PIXELS = 1 << 26  # MULLS_IMAGE_MAX_PIXELS
FLT_MAX = 3.4028234663852886e38


def image2d_params(m2pix=1.0, map_width=1920, map_height=1080, min_points_in_pix=20, max_points_in_pix=1000, min_height=-FLT_MAX, max_height=FLT_MAX, shift=1,
                   count_form=0):
    """the export's values (test/mulls_slam.cpp:1018)"""
    p = Image2dParams()
    p.m2pix, p.map_width, p.map_height, p.min_points_in_pix, p.max_points_in_pix = float(m2pix), int(map_width), int(map_height), int(min_points_in_pix), int(max_points_in_pix)
    p.min_height, p.max_height, p.shift, p.count_form = float(min_height), float(max_height), int(shift), int(count_form)
    return p


def bev_params(**kw):
    """the per-frame bird's-eye view (test/mulls_slam.cpp:731)"""
    d = dict(m2pix=4.0, map_width=400, map_height=400, min_points_in_pix=2, max_points_in_pix=50, min_height=-5.0, max_height=15.0, shift=0)
    d.update(kw)
    return image2d_params(**d)


def range_image_params(width=900, height=64, f_up_deg=3.0, f_down_deg=25.0, max_distance=70.0):
    """upstream's HDL-64 constants (cfilter.hpp:2717-2721)"""
    p = RangeImageParams()
    p.width, p.height, p.f_up_deg, p.f_down_deg, p.max_distance, p.reserved = int(width), int(height), float(f_up_deg), float(f_down_deg), float(max_distance), 0
    return p


class SubmapInfo(C.Structure):
    """mulls_submap_info: one submap of the device-resident archive (n in the ABI's class order; bounds as {min xyz, max xyz})"""

    _fields_ = [("n", C.c_uint32 * NCLASS), ("id_in_strip", C.c_int32), ("submaps_needed", C.c_uint32), ("offset", C.c_uint64), ("points_needed", C.c_uint64),
                ("pose_lo", C.c_double * 16), ("local_bound", C.c_double * 6), ("bound", C.c_double * 6)]


class OverlapParams(C.Structure):
    """mulls_overlap_params: find_overlap_registration_constraint's arguments (build_pose_graph.h:43-44)"""

    _fields_ = [("neighbor_search_dist", C.c_float), ("min_iou_thre", C.c_float), ("adjacent_id_thre", C.c_int32), ("search_2d", C.c_int32),
                ("max_neighbor", C.c_int32), ("reserved", C.c_int32)]


class SubmapEdge(C.Structure):
    """mulls_submap_edge: a candidate registration edge (tgt = the history submap, src = the query)"""

    _fields_ = [("tgt_id", C.c_int32), ("src_id", C.c_int32), ("overlapping_ratio", C.c_double), ("Trans1_2", C.c_double * 16)]


SUBMAP_CHUNK = 1024  # MULLS_SUBMAP_CHUNK
SUBMAP_MERGED = 6  # MULLS_SUBMAP_MERGED
SUBMAP_MERGED_NO_GROUND = 7  # MULLS_SUBMAP_MERGED_NO_GROUND
SUBMAP_MERGE_ORDER = (0, 2, 1, 3, 4, 5)  # cloudblock_t::merge_feature_points: ground, facade, pillar, beam, roof, vertex


def overlap_params(neighbor_search_dist=50.0, min_iou_thre=0.25, adjacent_id_thre=3, search_2d=1, max_neighbor=10):
    """upstream's defaults (build_pose_graph.h:43-44)"""
    p = OverlapParams()
    p.neighbor_search_dist, p.min_iou_thre = float(neighbor_search_dist), float(min_iou_thre)
    p.adjacent_id_thre, p.search_2d, p.max_neighbor, p.reserved = int(adjacent_id_thre), int(search_2d), int(max_neighbor), 0
    return p


def records(a):
    """Any point array (POINT_DTYPE records or raw (n, 48) bytes) as contiguous raw (n, 48) uint8 records, every byte kept."""
    a = np.asarray(a)
    if a.dtype == np.uint8 and a.ndim == 2 and a.shape[1] == POINT_BYTES:
        return np.ascontiguousarray(a)
    pts = as_points(a)
    return pts.view(np.uint8).reshape(len(pts), POINT_BYTES)


def points_of(raw):
    """Raw (n, 48) records viewed as POINT_DTYPE (no copy)."""
    raw = np.ascontiguousarray(raw)
    return raw.reshape(-1).view(POINT_DTYPE)


class Profile(C.Structure):
    _fields_ = [
        ("ms_setup", C.c_double),
        ("ms_nn", C.c_double),
        ("ms_filter", C.c_double),
        ("ms_accum", C.c_double),
        ("ms_residual", C.c_double),
        ("launches_nn", C.c_int32),
        ("iterations", C.c_int32),
        ("nn_pair_evals", C.c_uint64),
        ("nn_src_pts", C.c_uint64),
        ("nn_tgt_pts", C.c_uint64),
        ("ms_host_step", C.c_double),
        ("ms_host_wait", C.c_double),
        ("ms_host_launch", C.c_double),
        ("nn_tgt_unique", C.c_uint64),
        ("nn_corr_pts", C.c_uint64),
        ("icp_fused_ms", C.c_double * 6),
        ("icp_search_ms", C.c_double * 24),
        ("icp_phase_ms", C.c_double * 6),
        ("ms_stage", C.c_double),
        ("ms_stage_pack", C.c_double),
        ("stage_bytes", C.c_uint64),
    ]


def default_params(**overrides):
    """mm_lls_icp's default arguments (cregistration.hpp:1114-1123)."""
    p = Params()
    p.max_iter_num = 20
    p.dis_thre_unit = 1.5
    p.converge_translation = 0.002
    p.converge_rotation_d = 0.01
    p.dis_thre_min = 0.4
    p.dis_thre_update_rate = 1.1
    p.used_feature_type = b"111110"
    p.weight_strategy = b"1101"
    p.z_xy_balanced_ratio = 1.0
    p.pt2pt_residual_window = 0.1
    p.pt2pl_residual_window = 0.1
    p.pt2li_residual_window = 0.1
    p.apply_intersection_filter = 1
    p.apply_motion_undistortion = 0
    p.normal_shooting_on = 0
    p.use_more_points = 0
    p.normal_bearing = 45.0
    p.keep_less_source_points = 0
    p.faithful = 1
    p.rejector_strict = 1
    p.sigma_thre = 0.5
    p.min_neccessary_corr_ratio = 0.03
    p.max_bearable_rotation_d = 45.0
    p.rng_seed = 0
    for k, v in overrides.items():
        if isinstance(v, str):
            v = v.encode()
        setattr(p, k, v)
    return p


def kitti_params(**overrides):
    """The positional values test/mulls_slam.cpp:642-648 passes with script/config/lo_gflag_list_kitti_urban.txt
    (column s2s/s2m)."""
    kw = dict(
        max_iter_num=20,
        dis_thre_unit=1.4,
        converge_translation=0.0005,
        converge_rotation_d=0.001,
        dis_thre_min=0.5,
        dis_thre_update_rate=1.1,
        used_feature_type="111000",
        weight_strategy="1111",
        z_xy_balanced_ratio=1.0,
        pt2pt_residual_window=0.05,
        pt2pl_residual_window=0.05,
        pt2li_residual_window=0.05,
        apply_intersection_filter=1,
        normal_bearing=20.0,
        sigma_thre=0.35,
        min_neccessary_corr_ratio=0.03,
        max_bearable_rotation_d=45.0,
    )
    kw.update(overrides)
    return default_params(**kw)


def make_points(xyz, normals=None, intensity=None, curvature=None):
    """Build a (n,) POINT_DTYPE array from column arrays."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    pts = np.zeros(n, dtype=POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
        pts["nx"], pts["ny"], pts["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if intensity is not None:
        pts["intensity"] = np.asarray(intensity, dtype=np.float32)
    if curvature is not None:
        pts["curvature"] = np.asarray(curvature, dtype=np.float32)
    return pts


def normal3(pts):
    """normal[3] of every record (offset 28; not a named field: the registration never reads it, the map's PCA refresh writes it)."""
    pts = np.ascontiguousarray(pts)
    return pts.view(np.uint8).reshape(len(pts), POINT_BYTES)[:, 28:32].copy().view(np.float32).reshape(len(pts))


def as_points(a):
    """Coerce any structured array carrying the eight point fields to a contiguous POINT_DTYPE array."""
    if a is None:
        return np.zeros(0, dtype=POINT_DTYPE)
    a = np.asarray(a)
    if a.dtype == POINT_DTYPE and a.flags["C_CONTIGUOUS"]:
        return a
    out = np.zeros(len(a), dtype=POINT_DTYPE)
    for k in POINT_DTYPE.names:
        out[k] = a[k]
    return out


def as_cloud(pts):
    """mulls_cloud borrowing a POINT_DTYPE numpy array (caller keeps the array alive)."""
    c = Cloud()
    if pts is None or len(pts) == 0:
        c.pts, c.n, c.stride = None, 0, POINT_BYTES
        return c
    assert pts.dtype == POINT_DTYPE and pts.flags["C_CONTIGUOUS"]
    c.pts = pts.ctypes.data
    c.n = len(pts)
    c.stride = POINT_BYTES
    return c


class PairData:
    """Owns the numpy arrays of one registration problem and exposes the ctypes ``Pair`` borrowing them."""

    def __init__(self, tgt, src, init_guess=None, tgt_bound=None, src_down=None):
        self.tgt = [as_points(t) for t in tgt]
        self.src = [as_points(s) for s in src]
        self.src_down = None if src_down is None else [as_points(s) for s in src_down]
        self.init_guess = np.eye(4) if init_guess is None else np.asarray(init_guess, dtype=np.float64)
        if tgt_bound is None:
            allp = [t for t in self.tgt if len(t)]
            if allp:
                mn = [min(float(t[k].min()) for t in allp) for k in ("x", "y", "z")]
                mx = [max(float(t[k].max()) for t in allp) for k in ("x", "y", "z")]
            else:
                mn, mx = [0.0] * 3, [0.0] * 3
            tgt_bound = mn + mx
        self.tgt_bound = [float(v) for v in tgt_bound]

    def fill(self, pair):
        for c in range(NCLASS):
            pair.tgt[c] = as_cloud(self.tgt[c])
            pair.src[c] = as_cloud(self.src[c])
            pair.src_down[c] = as_cloud(self.src_down[c]) if self.src_down is not None else as_cloud(None)
        for k in range(6):
            pair.tgt_bound[k] = self.tgt_bound[k]
        g = np.asarray(self.init_guess, dtype=np.float64).T.reshape(-1)  # column-major
        for k in range(16):
            pair.init_guess[k] = float(g[k])
        return pair

    def as_pair(self):
        return self.fill(Pair())


def make_pair_array(pairs):
    arr = (Pair * len(pairs))()
    for i, p in enumerate(pairs):
        p.fill(arr[i])
    return arr


def make_result_array(n, trace_cap=0):
    res = (Result * n)()
    traces = []
    if trace_cap:
        for i in range(n):
            t = (IterTrace * trace_cap)()
            traces.append(t)
            res[i].trace = C.cast(t, C.POINTER(IterTrace))
            res[i].trace_cap = trace_cap
    res._traces = traces  # keep alive
    return res
