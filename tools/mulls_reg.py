"""Pairwise registration of two point clouds with the library, stage for stage what test/mulls_reg.cpp does (script/run_mulls_reg.sh):
read -> voxel_downsample (cloud_*_down_res, 0 = off as in run_mulls_reg.sh) -> fast_ground_filter -> classify_nground_pts per cloud -> the
cloud with more down-sampled feature points is the target -> with --is_global_reg (the reference's default: true) the global coarse registration:
non_max_suppress of both key-point clouds with keypoint_nms_radius = 0.25 x pca_neighbor_radius (test/mulls_reg.cpp:145-149; mulls_non_max_suppress — the
classification does not thin the key points: upstream's detect_key_pts is commented out and vertex_curvature_non_max_radius is unused),
find_feature_correspondence_ncc on the two thinned clouds -> coarse_reg_ransac with noise_bound = 4 x keypoint_nms_radius (test/mulls_reg.cpp:170-179;
mulls_ncc_correspond -> mulls_coarse_reg_ransac_indexed), whose transform is the initial guess (the identity when it fails, as upstream leaves init_mat)
-> mm_lls_icp -> the source's pc_down, transformed, written out.  Flags carry the reference's names and defaults (test/mulls_reg.cpp:24-60).  With
--global_solver=teaser the solver is coarse_reg_teaser (mulls_coarse_reg_teaser_indexed: the library's definition of upstream's TEASER++ call).  The
reference's own --teaser_on is accepted and still answered with the RANSAC solver.  Not here: the viewers.

    python tools/mulls_reg.py --point_cloud_1_path a.pcd --point_cloud_2_path b.pcd --output_point_cloud_path b_reg.pcd
"""
import argparse
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from mulls_amd import abi, lib  # noqa: E402


def flags(argv=None):
    def boolean(v):
        return str(v).lower() in ("1", "true", "yes", "on")

    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--point_cloud_1_path", required=True)
    p.add_argument("--point_cloud_2_path", required=True)
    p.add_argument("--output_point_cloud_path", default="")
    p.add_argument("--cloud_1_down_res", type=float, default=0.0)
    p.add_argument("--cloud_2_down_res", type=float, default=0.0)
    p.add_argument("--gf_grid_size", type=float, default=2.0)
    p.add_argument("--gf_in_grid_h_thre", type=float, default=0.3)
    p.add_argument("--gf_neigh_grid_h_thre", type=float, default=2.2)
    p.add_argument("--gf_max_h", type=float, default=3.0e38)
    p.add_argument("--gf_ground_down_rate", type=int, default=10)
    p.add_argument("--gf_nonground_down_rate", type=int, default=3)
    p.add_argument("--dist_inverse_sampling_method", type=int, default=0)
    p.add_argument("--unit_dist", type=float, default=15.0)
    p.add_argument("--ground_normal_method", type=int, default=3, help="extract_semantic_pts' default (cfilter.hpp:2304): 3 = plane RANSAC per grid cell")
    p.add_argument("--pca_distance_adpative_on", type=boolean, default=False)
    p.add_argument("--pca_neighbor_radius", type=float, default=1.0)
    p.add_argument("--pca_neighbor_count", type=int, default=30)
    p.add_argument("--linearity_thre", type=float, default=0.6)
    p.add_argument("--planarity_thre", type=float, default=0.6)
    p.add_argument("--curvature_thre", type=float, default=0.1)
    p.add_argument("--corr_dis_thre", type=float, default=2.0)
    p.add_argument("--reg_max_iter_num", type=int, default=25)
    p.add_argument("--converge_tran", type=float, default=0.001)
    p.add_argument("--converge_rot_d", type=float, default=0.01)
    p.add_argument("--is_global_reg", type=boolean, default=True)
    p.add_argument("--teaser_on", type=boolean, default=False)
    p.add_argument("--global_solver", choices=("ransac", "teaser"), default="ransac", help="teaser: coarse_reg_teaser (mulls_coarse_reg_teaser_indexed)")
    p.add_argument("--corr_num", type=int, default=3000)
    p.add_argument("--reciprocal_corr_on", type=boolean, default=False)
    p.add_argument("--fixed_num_corr_on", type=boolean, default=False)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--baseline_reg_method", "--method", dest="baseline_reg_method", choices=("", "ndt", "gicp", "pclicp"), default="",
                   help="ndt: CRegistration::omp_ndt (mulls_ndt), gicp: CRegistration::omp_gicp with voxelised GICP (mulls_gicp), pclicp: CRegistration::pcl_icp "
                        "(mulls_pcl_icp), on the two pc_down clouds in place of mm_lls_icp, as test/mulls_slam.cpp's baselines")
    p.add_argument("--pclicp_metric", choices=("point2point", "point2plane"), default="point2plane", help="pclicp: the step (upstream names no default)")
    p.add_argument("--pclicp_reciprocal", type=boolean, default=False, help="pclicp: use_reciprocal_correspondence")
    p.add_argument("--reg_voxel_size", type=float, default=1.0, help="the NDT leaf size or the VGICP voxel size (test/mulls_slam.cpp's reg_voxel_size)")
    a, _ = p.parse_known_args(argv)  # glog / viewer flags of the reference's script are accepted and ignored
    return a


def read_cloud(path):
    """DataIo::read_pc_cloud_block(block, normalize_intensity_or_not = true) (dataio.hpp:1732-1756, test/mulls_reg.cpp:130-131): the intensity
    rescaled to 0 - 255 with the reference's float expressions"""
    p = lib.read_kitti_bin(path) if path.endswith(".bin") else lib.read_pcd(path)
    p = p.copy()
    inten = p["intensity"].astype(np.float32)
    if len(inten):
        lo, hi = np.float32(inten.min()), np.float32(inten.max())
        with np.errstate(divide="ignore", invalid="ignore"):
            p["intensity"] = (inten - lo) * np.float32(255.0 / float(hi - lo))
    return p


def scan_bound(p):
    """block->local_bound = the bounding box of pc_raw (get_cloud_bbx_cpt, dataio.hpp:1736)"""
    return [float(p[k].min()) for k in ("x", "y", "z")] + [float(p[k].max()) for k in ("x", "y", "z")]


def extract_semantic_pts(ctx, scan, F, vf_downsample_resolution):
    """CFilter::extract_semantic_pts (cfilter.hpp:2294-2413) as test/mulls_reg.cpp:134-143 calls it (its default ground normal method 3: the per-cell plane RANSAC).
    Returns (class clouds, their *_down clouds, pc_down)."""
    GP = abi.ground_params(min_grid_pt_num=8, grid_resolution=F.gf_grid_size, max_height_difference=F.gf_in_grid_h_thre,
                           neighbor_height_diff=F.gf_neigh_grid_h_thre, max_ground_height=F.gf_max_h, ground_random_down_rate=F.gf_ground_down_rate,
                           ground_random_down_down_rate=2, nonground_random_down_rate=F.gf_nonground_down_rate, reliable_neighbor_grid_num_thre=0,
                           estimate_ground_normal_method=F.ground_normal_method, distance_weight_downsampling_method=F.dist_inverse_sampling_method,
                           standard_distance=F.unit_dist, fixed_num_downsampling=0, down_ground_fixed_num=500, intensity_thre=3.0e38,
                           apply_grid_wise_outlier_filter=0)
    CP = abi.classify_params(neighbor_searching_radius=F.pca_neighbor_radius, neighbor_k=F.pca_neighbor_count, neigh_k_min=8, pca_down_rate=1,
                             edge_thre=F.linearity_thre, planar_thre=F.planarity_thre, edge_thre_down=F.linearity_thre + 0.1,
                             planar_thre_down=F.planarity_thre + 0.1, curvature_thre=F.curvature_thre,
                             vertex_curvature_non_max_radius=1.5 * F.pca_neighbor_radius, use_distance_adaptive_pca=int(F.pca_distance_adpative_on))
    pc_down = ctx.voxel_downsample(scan, vf_downsample_resolution) if vf_downsample_resolution >= 0.001 else abi.records(scan)
    ground, ground_down, unground = ctx.ground_filter(abi.points_of(pc_down), GP)
    c = ctx.classify_nground(unground, CP)
    full = [ground, c[abi.CL_PILLAR], c[abi.CL_FACADE], c[abi.CL_BEAM], c[abi.CL_ROOF], c[abi.CL_VERTEX]]
    down = [ground_down, c[abi.CL_PILLAR_DOWN], c[abi.CL_FACADE_DOWN], c[abi.CL_BEAM_DOWN], c[abi.CL_ROOF_DOWN], c[abi.CL_VERTEX]]
    return full, down, pc_down


def global_registration(ctx, tgt_kpts, src_kpts, F):
    """test/mulls_reg.cpp:170-179: key-point correspondences, then the RANSAC solver; returns init_mat"""
    if F.teaser_on:
        # (this line and the RANSAC answer to the reference's flag are what tests/test_gpu_ransac.py holds the tool to; the library's own solver of
        # coarse_reg_teaser is selected with --global_solver=teaser)
        print("--teaser_on: TEASER++ is not part of the library; the RANSAC solver (coarse_reg_ransac) is used")
    keypoint_nms_radius = 0.25 * F.pca_neighbor_radius  # :107
    ok, ti, si, n = ctx.ncc_correspond(tgt_kpts, src_kpts, abi.ncc_params(int(F.fixed_num_corr_on), F.corr_num, int(F.reciprocal_corr_on)))
    if F.global_solver == "teaser":  # test/mulls_reg.cpp:176-177
        res, _ = ctx.coarse_reg_teaser(tgt_kpts, src_kpts, abi.teaser_params(noise_bound=4.0 * keypoint_nms_radius), cap=0, tgt_idx=ti, src_idx=si)
        print("global registration: %d key-point pairs, TEASER status %d: clique of %d (%s, %d search nodes, %.1f ms), %d GNC iterations, %d rotation inliers"
              % (n, res.status, res.clique_size, "exact" if res.clique_exact else "budget ended the search", res.clique_nodes, 1e3 * res.search_seconds,
                 res.gnc_iterations, res.n_rotation_inliers))
        return np.array(res.T[:], np.float64).reshape(4, 4).T.copy() if res.status >= 0 else np.eye(4)
    res, _ = ctx.coarse_reg_ransac(tgt_kpts, src_kpts, abi.ransac_params(noise_bound=4.0 * keypoint_nms_radius), cap=0, tgt_idx=ti, src_idx=si)
    print("global registration: %d key-point pairs, RANSAC status %d after %d iterations, %d inliers" % (n, res.status, res.iterations, res.n_inliers))
    # upstream writes init_mat only when the solver does not fail (cregistration.hpp:642-660)
    return np.array(res.T[:], np.float64).reshape(4, 4).T.copy() if res.status >= 0 else np.eye(4)


class NdtOutcome:
    """mulls_ndt_result, mulls_gicp_result or mulls_pcl_icp_result with the three members main() reads of an abi.Result"""

    def __init__(self, r):
        self.ndt, self.code, self.iters = r, r.code, r.iterations

    def T_matrix(self):
        return np.array(self.ndt.T[:], np.float64).reshape(4, 4).T.copy()


def register(ctx, scan1, scan2, F):
    """Returns (abi.Result, which scan is the source: 1 or 2, that scan's pc_down)."""
    # test/mulls_reg.cpp:80-81, :134-143: block 1 is down-sampled with cloud_2_down_res, block 2 with cloud_1_down_res
    f1, d1, p1 = extract_semantic_pts(ctx, scan1, F, F.cloud_2_down_res)
    f2, d2, p2 = extract_semantic_pts(ctx, scan2, F, F.cloud_1_down_res)
    n1, n2 = sum(len(x) for x in d1), sum(len(x) for x in d2)
    # determine_source_target_cloud (cregistration.hpp:857-870): block1 (target) = the one with more down-sampled feature points
    (tgt_full, src_down, source) = (f1, d2, 2) if n1 > n2 else (f2, d1, 1)
    init_mat = np.eye(4)
    if F.is_global_reg:
        # test/mulls_reg.cpp:145-149: both blocks' pc_vertex, in place (the sizes above, which chose the target, were taken before)
        keypoint_nms_radius = 0.25 * F.pca_neighbor_radius
        kpts = []
        for which, cloud in (("target", tgt_full[5]), ("source", src_down[5])):
            kept = ctx.non_max_suppress(cloud, keypoint_nms_radius)[0]
            print("non_max_suppress: %s key points %d -> %d" % (which, len(cloud), len(kept)))
            kpts.append(kept)
        tgt_full[5], src_down[5] = kpts
        init_mat = global_registration(ctx, tgt_full[5], src_down[5], F)
    if F.baseline_reg_method == "ndt":
        # omp_ndt(reg_con, reg_voxel_size, ndt_searching_method = true, init_mat) (test/mulls_slam.cpp:635): block1 / block2 ->pc_down and their local_bound
        tgt_scan, src_scan = (scan1, scan2) if source == 2 else (scan2, scan1)
        r = ctx.ndt((p1, p2)[2 - source], (p1, p2)[source - 1], scan_bound(abi.as_points(tgt_scan)), scan_bound(abi.as_points(src_scan)), init_mat,
                    abi.ndt_params(resolution=F.reg_voxel_size))
        print("omp_ndt: %d iterations, %d evaluations, fitness %.4f, %d of %d leaves used" % (r.iterations, r.evaluations, r.fitness, r.n_leaves_used, r.n_leaves))
        return NdtOutcome(r), source, (p1, p2)[source - 1]
    if F.baseline_reg_method == "gicp":
        # omp_gicp(reg_con, max_iter, thre, voxel_gicp_on = true, reg_voxel_size, init_mat) (test/mulls_slam.cpp:638): the same clouds and bounds
        tgt_scan, src_scan = (scan1, scan2) if source == 2 else (scan2, scan1)
        r = ctx.gicp((p1, p2)[2 - source], (p1, p2)[source - 1], scan_bound(abi.as_points(tgt_scan)), scan_bound(abi.as_points(src_scan)), init_mat,
                     abi.gicp_params(voxel_resolution=F.reg_voxel_size))
        print("omp_gicp: %d iterations, stop %d, fitness %.4f, %d voxels, %d of %d source points with a voxel" % (r.iterations + 1, r.stop, r.fitness, r.n_voxels, r.n_corr, r.n_src))
        return NdtOutcome(r), source, (p1, p2)[source - 1]
    if F.baseline_reg_method == "pclicp":
        # pcl_icp(reg_con, max_iter, thre, metrics, NN, te, reciprocal, false, 2.0, init_mat): test/mulls_slam.cpp:195 names the method and never calls
        # it; the iteration cap and the distance are mm_lls_icp's flags, the same clouds and bounds as the other baselines
        tgt_scan, src_scan = (scan1, scan2) if source == 2 else (scan2, scan1)
        plane = F.pclicp_metric == "point2plane"
        prm = abi.pcl_icp_params(max_iter_num=F.reg_max_iter_num, dis_thre_unit=F.corr_dis_thre, metrics=abi.PCL_ICP_POINT2PLANE if plane else abi.PCL_ICP_POINT2POINT,
                                 te=abi.PCL_ICP_LLS if plane else abi.PCL_ICP_SVD, use_reciprocal_correspondence=int(F.pclicp_reciprocal))
        r = ctx.pcl_icp((p1, p2)[2 - source], (p1, p2)[source - 1], scan_bound(abi.as_points(tgt_scan)), scan_bound(abi.as_points(src_scan)), init_mat, prm)
        print("pcl_icp (%s): %d iterations, stop %d, %d pairs, mse %.4f, fitness %.4f over %d of %d source points"
              % (F.pclicp_metric, r.iterations, r.stop, r.n_corr, r.mse, r.fitness, r.n_fit, r.n_src))
        return NdtOutcome(r), source, (p1, p2)[source - 1]
    pair = abi.PairData([abi.points_of(t) for t in tgt_full], [abi.points_of(s) for s in src_down],
                        init_guess=init_mat, tgt_bound=scan_bound(abi.as_points(scan1 if source == 2 else scan2)) if len(scan1) and len(scan2) else None)
    # mm_lls_icp(reg_con, max_iter, thre, converge_tran, converge_rot_d, 0.25 * thre, 1.1, "111110", "1101", 1.0, 0.1, 0.1, 0.1, init_mat)
    P = abi.default_params(max_iter_num=F.reg_max_iter_num, dis_thre_unit=F.corr_dis_thre, converge_translation=F.converge_tran,
                           converge_rotation_d=F.converge_rot_d, dis_thre_min=0.25 * F.corr_dis_thre, dis_thre_update_rate=1.1,
                           used_feature_type="111110", weight_strategy="1101", z_xy_balanced_ratio=1.0, pt2pt_residual_window=0.1,
                           pt2pl_residual_window=0.1, pt2li_residual_window=0.1)
    return ctx.icp(pair, P)[0], source, (p1, p2)[source - 1]


def main(argv=None):
    F = flags(argv)
    ctx = lib.Context(F.device)
    scans = [read_cloud(F.point_cloud_1_path), read_cloud(F.point_cloud_2_path)]
    res, source, source_down = register(ctx, scans[0], scans[1], F)
    T = res.T_matrix()
    print("process code %d after %d iterations; source = point cloud %d; Trans1_2 =" % (res.code, res.iters, source))
    print(np.array2string(T, precision=6, suppress_small=True))
    if F.output_point_cloud_path:
        moved = ctx.transform(abi.points_of(source_down), T)  # pcl::transformPointCloud(*block2->pc_down, *pc_s_tran, Trans1_2)
        lib.write_pcd(F.output_point_cloud_path, moved)
    return res, source


if __name__ == "__main__":
    main()
