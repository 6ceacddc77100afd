// cregistration_hip.hpp — drop-in bridge from MULLS' CRegistration<PointT>::mm_lls_icp() to libmulls_hip.so.
//
// The reference has no plugin/FFI layer: mm_lls_icp is a public member of the header-only class template
// lo::CRegistration<PointT> (include/common/cregistration.hpp:1114-1440), called positionally from
// test/mulls_reg.cpp:194 and test/mulls_slam.cpp:477,560,642,679.  This header keeps that exact signature (argument
// order, types, defaults) as a free function template, lo::hip::mm_lls_icp<PointT>(), so that the one-line binding a
// maintainer adds at cregistration.hpp:1125
//
//     #ifdef MULLS_USE_HIP
//         return lo::hip::mm_lls_icp<PointT>(registration_cons, max_iter_num, dis_thre_unit, converge_translation,
//                 converge_rotation_d, dis_thre_min, dis_thre_update_rate, used_feature_type, weight_strategy,
//                 z_xy_balanced_ratio, pt2pt_residual_window, pt2pl_residual_window, pt2li_residual_window,
//                 initial_guess, apply_intersection_filter, apply_motion_undistortion_while_registration,
//                 normal_shooting_on, normal_bearing, use_more_points, keep_less_source_points, sigma_thre,
//                 min_neccessary_corr_ratio, max_bearable_rotation_d);
//     #endif
//
// leaves every call site, cloudblock_t and constraint_t (include/common/utility.hpp:233-590) untouched.
// See INTEGRATION.md for the build flags and for what is and is not reproduced (kd-tree side effect, logging).
//
// Requirements on the including translation unit: MULLS' utility.hpp (lo::constraint_t, lo::cloudblock_t, Matrix6d),
// PCL point types and Eigen must already be visible — exactly what cregistration.hpp includes before line 1114.
#ifndef MULLS_CREGISTRATION_HIP_HPP
#define MULLS_CREGISTRATION_HIP_HPP

#include <algorithm>
#include <cstring>
#include <array>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mulls_hip.h"
#include "cregistration_fpfh_hip.hpp" // the library context of a thread, borrow(), and the FPFH / SAC-IA bridge, which needs no type of utility.hpp

namespace lo
{
namespace hip
{

// When set (default), block1->tree_{ground,pillar,beam,facade,roof,vertex} are rebuilt on the cropped target clouds
// like cregistration.hpp:1209-1232 does, because MapManager::map_based_dynamic_close_removal (src/map_manager.cpp:187-243)
// queries them on the next frame.  The registration itself never uses a CPU kd-tree.  Benchmarks switch it off.
// The switch only matters while the process keeps NO device-resident local map: as soon as lo::hip::update_local_map() has
// created a mirror, the trees' one consumer runs on the device against that mirror and no registration builds them — neither
// the scan-to-map one (its block1 has the mirror) nor the scan-to-scan one against the previous frame's block.
inline bool &build_cpu_trees()
{
	static bool on = true;
	return on;
}

// ---- device-resident local map -------------------------------------------------------------------------
// A cloudblock_t that acts as the scan-to-map target can be given a mirror in HBM: lo::hip::update_local_map() (below)
// creates it on first use and keeps it up to date; lo::hip::mm_lls_icp() then takes block1's six class clouds straight
// from the device (no upload of the 20 k - 1 M point target per frame) and remembers which part of them the registration
// indexed, which is what MapManager::map_based_dynamic_close_removal looks at on the next frame (block1->tree_*).
struct MapMirror
{
	mulls_map *map = nullptr;
	int tree_mode = 0; // 0: no registration against this map yet; 1: whole clouds; 2: cropped to tree_box
	char tree_used[8] = {'0', '0', '0', '0', '0', '0', 0, 0};
	double tree_box[6] = {0, 0, 0, 0, 0, 0};
};
inline std::map<const cloudblock_t *, MapMirror> &map_mirrors()
{
	struct Holder
	{
		std::map<const cloudblock_t *, MapMirror> m;
		~Holder() // after thread_context()'s holder was constructed, so destroyed before it
		{
			for (auto &kv : m)
				if (kv.second.map)
					mulls_map_destroy(thread_context(), kv.second.map);
		}
	};
	thread_context();
	static thread_local Holder holder;
	return holder.m;
}
// When set (default), update_local_map copies the updated class clouds back into local_map->pc_* so that every other
// consumer of the block (viewer, sub-map cloning, loop closure) sees what the reference would have left there.
inline bool &sync_host_map()
{
	static bool on = true;
	return on;
}
// forget the mirror of a block whose host clouds were changed behind the bridge's back (it is rebuilt from them on next use)
inline void invalidate_map_mirror(const cloudblock_t *block)
{
	auto &m = map_mirrors();
	auto it = m.find(block);
	if (it != m.end())
	{
		mulls_map_destroy(thread_context(), it->second.map);
		m.erase(it);
	}
}
inline MapMirror &attach_local_map(const cloudblock_Ptr &block)
{
	auto &m = map_mirrors();
	auto it = m.find(block.get());
	if (it != m.end())
		return it->second;
	mulls_ctx *ctx = thread_context();
	MapMirror mir;
	int rc = mulls_map_create(ctx, &mir.map);
	if (rc == MULLS_OK)
	{
		const mulls_cloud clouds[6] = {borrow(block->pc_ground), borrow(block->pc_pillar), borrow(block->pc_facade),
									   borrow(block->pc_beam),	 borrow(block->pc_roof),   borrow(block->pc_vertex)};
		rc = mulls_map_set(ctx, mir.map, clouds, block->pose_lo.data());
	}
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("local map mirror failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	return m.emplace(block.get(), mir).first->second;
}

template <typename PointT>
int mm_lls_icp(constraint_t &registration_cons, // cblock_1 (target point cloud), cblock_2 (source point cloud)
			   int max_iter_num = 20, float dis_thre_unit = 1.5, float converge_translation = 0.002, float converge_rotation_d = 0.01,
			   float dis_thre_min = 0.4, float dis_thre_update_rate = 1.1, std::string used_feature_type = "111110",
			   std::string weight_strategy = "1101", float z_xy_balanced_ratio = 1.0, float pt2pt_residual_window = 0.1,
			   float pt2pl_residual_window = 0.1, float pt2li_residual_window = 0.1,
			   Eigen::Matrix4d initial_guess = Eigen::Matrix4d::Identity(), bool apply_intersection_filter = true,
			   bool apply_motion_undistortion_while_registration = false, bool normal_shooting_on = false, float normal_bearing = 45.0,
			   bool use_more_points = false, bool keep_less_source_points = false, float sigma_thre = 0.5,
			   float min_neccessary_corr_ratio = 0.03, float max_bearable_rotation_d = 45.0)
{
	mulls_ctx *ctx = thread_context();
	cloudblock_t &b1 = *registration_cons.block1; // target
	cloudblock_t &b2 = *registration_cons.block2; // source

	mulls_pair pair;
	std::memset(&pair, 0, sizeof(pair));
	// class index == used_feature_type character index (cregistration.hpp:1196-1201)
	pair.tgt[MULLS_GROUND] = borrow(b1.pc_ground);
	pair.tgt[MULLS_PILLAR] = borrow(b1.pc_pillar);
	pair.tgt[MULLS_FACADE] = borrow(b1.pc_facade);
	pair.tgt[MULLS_BEAM] = borrow(b1.pc_beam);
	pair.tgt[MULLS_ROOF] = borrow(b1.pc_roof);
	pair.tgt[MULLS_VERTEX] = borrow(b1.pc_vertex);
	MapMirror *mirror = nullptr;
	{
		auto &mm = map_mirrors();
		auto it = mm.find(&b1);
		if (it != mm.end())
		{
			mirror = &it->second; // block1 is a device-resident local map: its clouds are already in HBM
			// keep_less_source_points thins the target's ground / facade clouds before their kd-trees are built (cregistration.hpp:1190-1193,
			// time-seeded): the trees the next update_local_map's dynamic removal searches would hold that random subset, which the mirror's
			// tree state (crop box only) cannot describe — refused rather than silently searching a different point set
			if (keep_less_source_points)
				throw std::runtime_error("lo::hip::mm_lls_icp: keep_less_source_points with a device-resident block1 (local map mirror) is not supported; "
										 "call lo::hip::invalidate_map_mirror(block1) first or pass keep_less_source_points = false");
			for (int c = 0; c < 6; c++)
				if (mulls_map_cloud(ctx, mirror->map, c, &pair.tgt[c]) != MULLS_OK)
					throw std::runtime_error(std::string("mulls_map_cloud: ") + mulls_last_error(ctx));
		}
	}
	// clone_feature(..., !use_more_points): down-sampled features unless use_more_points; vertex always pc_vertex (utility.hpp:524-550)
	pair.src[MULLS_GROUND] = borrow(use_more_points ? b2.pc_ground : b2.pc_ground_down);
	pair.src[MULLS_PILLAR] = borrow(use_more_points ? b2.pc_pillar : b2.pc_pillar_down);
	pair.src[MULLS_FACADE] = borrow(use_more_points ? b2.pc_facade : b2.pc_facade_down);
	pair.src[MULLS_BEAM] = borrow(use_more_points ? b2.pc_beam : b2.pc_beam_down);
	pair.src[MULLS_ROOF] = borrow(use_more_points ? b2.pc_roof : b2.pc_roof_down);
	pair.src[MULLS_VERTEX] = borrow(b2.pc_vertex);
	// batch_apply_motion_compensation always starts from the _down clouds (cregistration.hpp:1251-1253)
	pair.src_down[MULLS_GROUND] = borrow(b2.pc_ground_down);
	pair.src_down[MULLS_PILLAR] = borrow(b2.pc_pillar_down);
	pair.src_down[MULLS_FACADE] = borrow(b2.pc_facade_down);
	pair.src_down[MULLS_BEAM] = borrow(b2.pc_beam_down);
	pair.src_down[MULLS_ROOF] = borrow(b2.pc_roof_down);
	pair.src_down[MULLS_VERTEX] = borrow(b2.pc_vertex);
	pair.tgt_bound[0] = b1.local_bound.min_x;
	pair.tgt_bound[1] = b1.local_bound.min_y;
	pair.tgt_bound[2] = b1.local_bound.min_z;
	pair.tgt_bound[3] = b1.local_bound.max_x;
	pair.tgt_bound[4] = b1.local_bound.max_y;
	pair.tgt_bound[5] = b1.local_bound.max_z;
	std::memcpy(pair.init_guess, initial_guess.data(), sizeof(pair.init_guess)); // Eigen::Matrix4d is column-major

	mulls_params P;
	mulls_default_params(&P);
	P.max_iter_num = max_iter_num;
	P.dis_thre_unit = dis_thre_unit;
	P.converge_translation = converge_translation;
	P.converge_rotation_d = converge_rotation_d;
	P.dis_thre_min = dis_thre_min;
	P.dis_thre_update_rate = dis_thre_update_rate;
	std::memset(P.used_feature_type, 0, sizeof(P.used_feature_type));
	std::memset(P.weight_strategy, 0, sizeof(P.weight_strategy));
	std::strncpy(P.used_feature_type, used_feature_type.c_str(), sizeof(P.used_feature_type) - 1);
	std::strncpy(P.weight_strategy, weight_strategy.c_str(), sizeof(P.weight_strategy) - 1);
	P.z_xy_balanced_ratio = z_xy_balanced_ratio;
	P.pt2pt_residual_window = pt2pt_residual_window;
	P.pt2pl_residual_window = pt2pl_residual_window;
	P.pt2li_residual_window = pt2li_residual_window;
	P.apply_intersection_filter = apply_intersection_filter;
	P.apply_motion_undistortion = apply_motion_undistortion_while_registration;
	P.normal_shooting_on = normal_shooting_on;
	P.use_more_points = use_more_points;
	P.normal_bearing = normal_bearing;
	P.keep_less_source_points = keep_less_source_points;
	P.faithful = 1;
	P.sigma_thre = sigma_thre;
	P.min_neccessary_corr_ratio = min_neccessary_corr_ratio;
	P.max_bearable_rotation_d = max_bearable_rotation_d;

	mulls_result R;
	std::memset(&R, 0, sizeof(R));
	const int rc = mulls_icp(ctx, &pair, &P, &R);
	if (rc != MULLS_OK) // infrastructure failure (no device, HIP error): the reference has no channel for it
		throw std::runtime_error(std::string("mulls_icp failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));

	// constraint_t outputs (cregistration.hpp:1405-1420)
	std::memcpy(registration_cons.Trans1_2.data(), R.T, sizeof(R.T));
	std::memcpy(registration_cons.information_matrix.data(), R.info, sizeof(R.info));
	registration_cons.sigma = R.sigma;
	registration_cons.confidence = R.confidence;

	if (mirror && max_iter_num > 0)
	{
		// what block1->tree_* hold from here on (cregistration.hpp:1209-1232), for the next update_local_map
		mirror->tree_mode = R.cropped ? 2 : 1;
		std::memcpy(mirror->tree_box, R.crop_box, sizeof(mirror->tree_box));
		for (int c = 0; c < 6; c++)
			mirror->tree_used[c] = (used_feature_type[c] == '1' && R.ntgt0[c] > 0) ? '1' : '0';
	}
	if (build_cpu_trees() && !mirror && map_mirrors().empty())
	{
		// kd-tree side effect of cregistration.hpp:1209-1232: trees over the intersection-filtered target clouds
		typedef typename pcl::PointCloud<PointT> Cloud;
		struct Item
		{
			int cls;
			typename Cloud::Ptr src;
			pcTreePtr tree;
		};
		const Item items[6] = {{MULLS_GROUND, b1.pc_ground, b1.tree_ground}, {MULLS_PILLAR, b1.pc_pillar, b1.tree_pillar},
							   {MULLS_FACADE, b1.pc_facade, b1.tree_facade}, {MULLS_BEAM, b1.pc_beam, b1.tree_beam},
							   {MULLS_ROOF, b1.pc_roof, b1.tree_roof},		 {MULLS_VERTEX, b1.pc_vertex, b1.tree_vertex}};
		for (const Item &it : items)
		{
			if (used_feature_type[it.cls] != '1')
				continue;
			typename Cloud::Ptr cropped(new Cloud);
			if (R.cropped)
			{
				for (const PointT &p : it.src->points) // CFilter::bbx_filter, strict inequalities (cfilter.hpp:959-961)
					if (p.x > R.crop_box[0] && p.x < R.crop_box[3] && p.y > R.crop_box[1] && p.y < R.crop_box[4] && p.z > R.crop_box[2] &&
						p.z < R.crop_box[5])
						cropped->points.push_back(p);
			}
			else
				*cropped = *it.src;
			if (cropped->points.size() > 0)
				it.tree->setInputCloud(cropped);
		}
	}
	return R.code;
}

// lls_icp_3dof_ground (cregistration.hpp:1443-1445), verbatim signature.  Like the reference it returns the process code cast
// to bool (true for 1, -1 and -2 alike) and only writes registration_cons.Trans1_2.
template <typename PointT>
bool lls_icp_3dof_ground(constraint_t &registration_cons, int max_iter_num = 20, float dis_thre_unit = 1.5, float converge_translation = 0.002,
						 float converge_rotation_d = 0.01, float dis_thre_min = 0.4, float dis_thre_update_rate = 1.1,
						 std::string weight_strategy = "1111", Eigen::Matrix4d initial_guess = Eigen::Matrix4d::Identity(),
						 bool keep_less_source_points = false, float max_bearable_rotation_d = 10.0)
{
	mulls_ctx *ctx = thread_context();
	mulls_pair pair;
	std::memset(&pair, 0, sizeof(pair));
	pair.tgt[MULLS_GROUND] = borrow(registration_cons.block1->pc_ground);
	pair.src[MULLS_GROUND] = borrow(registration_cons.block2->pc_ground_down);
	std::memcpy(pair.init_guess, initial_guess.data(), sizeof(pair.init_guess));
	mulls_params P;
	mulls_default_params(&P);
	P.max_iter_num = max_iter_num;
	P.dis_thre_unit = dis_thre_unit;
	P.converge_translation = converge_translation;
	P.converge_rotation_d = converge_rotation_d;
	P.dis_thre_min = dis_thre_min;
	P.dis_thre_update_rate = dis_thre_update_rate;
	std::memset(P.weight_strategy, 0, sizeof(P.weight_strategy));
	std::strncpy(P.weight_strategy, weight_strategy.c_str(), sizeof(P.weight_strategy) - 1);
	P.keep_less_source_points = keep_less_source_points;
	P.max_bearable_rotation_d = max_bearable_rotation_d;
	mulls_result R;
	std::memset(&R, 0, sizeof(R));
	const int rc = mulls_icp_3dof_ground(ctx, &pair, &P, &R);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_icp_3dof_ground failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	std::memcpy(registration_cons.Trans1_2.data(), R.T, sizeof(R.T));
	return R.code != 0;
}

// mm_lls_icp_4dof_global (cregistration.hpp:1584-1586), verbatim signature: all heading trials run as one batch.
template <typename PointT>
bool mm_lls_icp_4dof_global(constraint_t &registration_con, float heading_step_d, int max_iter_num = 20, float dis_thre_unit = 1.5,
							float converge_translation = 0.005, float converge_rotation_d = 0.05, float dis_thre_min = 0.5,
							float dis_thre_update_rate = 1.05, float max_bearable_rotation_d = 15.0)
{
	mulls_ctx *ctx = thread_context();
	cloudblock_t &b1 = *registration_con.block1;
	cloudblock_t &b2 = *registration_con.block2;
	mulls_pair pair;
	std::memset(&pair, 0, sizeof(pair));
	pair.tgt[MULLS_GROUND] = borrow(b1.pc_ground);
	pair.tgt[MULLS_PILLAR] = borrow(b1.pc_pillar);
	pair.tgt[MULLS_FACADE] = borrow(b1.pc_facade);
	pair.tgt[MULLS_BEAM] = borrow(b1.pc_beam);
	pair.tgt[MULLS_ROOF] = borrow(b1.pc_roof);
	pair.tgt[MULLS_VERTEX] = borrow(b1.pc_vertex);
	pair.src[MULLS_GROUND] = borrow(b2.pc_ground_down);
	pair.src[MULLS_PILLAR] = borrow(b2.pc_pillar_down);
	pair.src[MULLS_FACADE] = borrow(b2.pc_facade_down);
	pair.src[MULLS_BEAM] = borrow(b2.pc_beam_down);
	pair.src[MULLS_ROOF] = borrow(b2.pc_roof_down);
	pair.src[MULLS_VERTEX] = borrow(b2.pc_vertex);
	pair.tgt_bound[0] = b1.local_bound.min_x;
	pair.tgt_bound[1] = b1.local_bound.min_y;
	pair.tgt_bound[2] = b1.local_bound.min_z;
	pair.tgt_bound[3] = b1.local_bound.max_x;
	pair.tgt_bound[4] = b1.local_bound.max_y;
	pair.tgt_bound[5] = b1.local_bound.max_z;
	const double station[3] = {b2.local_station.x, b2.local_station.y, b2.local_station.z};
	mulls_result R;
	std::memset(&R, 0, sizeof(R));
	int success = 0;
	float best_heading = 0.0f;
	const int rc = mulls_icp_4dof_global(ctx, &pair, heading_step_d, station, max_iter_num, dis_thre_unit, converge_translation, converge_rotation_d,
										 dis_thre_min, dis_thre_update_rate, max_bearable_rotation_d, &R, &success, &best_heading);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_icp_4dof_global failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	if (success == 1) // the reference only touches registration_con when a succeeded trial also took the best score (:1645-1657)
	{
		std::memcpy(registration_con.Trans1_2.data(), R.T, sizeof(R.T));
		std::memcpy(registration_con.information_matrix.data(), R.info, sizeof(R.info));
		registration_con.sigma = R.sigma;
		registration_con.confidence = R.confidence;
	}
	return success != 0;
}

// MapManager::update_local_map (include/pgo/map_manager.h:21-31, src/map_manager.cpp:18-140), verbatim signature.  The binding
// a maintainer adds is one early return at the top of the member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::update_local_map(local_map, last_target_cblock, local_map_radius, max_num_pts, ...);
//     #endif
// Differences: pcl::RandomSample is seeded with time(NULL) upstream, here with `map_rng_seed()`; with recalculate_feature_on the
// refreshed directions agree with pcl::PCA's up to Eigen's float eigen-solver accuracy and the direction's sign.
inline uint64_t &map_rng_seed()
{
	static uint64_t seed = 0;
	return seed;
}
// (the two halves of an update the single call and the batch share: the parameters of one map's update, and what goes back into the two blocks)
inline mulls_map_params map_update_params(const MapMirror &mir, float local_map_radius, int max_num_pts, int kept_vertex_num, float last_frame_reliable_radius,
										  bool map_based_dynamic_removal_on, const std::string &used_feature_type, float dynamic_removal_center_radius,
										  float dynamic_dist_thre_min, float dynamic_dist_thre_max, float near_dist_thre, bool recalculate_feature_on)
{
	mulls_map_params P;
	mulls_map_default_params(&P);
	P.local_map_radius = local_map_radius;
	P.max_num_pts = max_num_pts;
	P.kept_vertex_num = kept_vertex_num;
	P.last_frame_reliable_radius = last_frame_reliable_radius;
	P.map_based_dynamic_removal_on = map_based_dynamic_removal_on;
	std::memset(P.used_feature_type, 0, sizeof(P.used_feature_type));
	std::strncpy(P.used_feature_type, used_feature_type.c_str(), sizeof(P.used_feature_type) - 1);
	P.dynamic_removal_center_radius = dynamic_removal_center_radius;
	P.dynamic_dist_thre_min = dynamic_dist_thre_min;
	P.dynamic_dist_thre_max = dynamic_dist_thre_max;
	P.near_dist_thre = near_dist_thre;
	P.recalculate_feature_on = recalculate_feature_on;
	P.rng_seed = map_rng_seed()++;
	P.tree_mode = mir.tree_mode;
	std::memcpy(P.tree_used, mir.tree_used, sizeof(P.tree_used));
	std::memcpy(P.tree_box, mir.tree_box, sizeof(P.tree_box));
	return P;
}
inline void map_update_take(mulls_ctx *ctx, MapMirror &mir, const mulls_map_report &rep, cloudblock_t &m, cloudblock_t &f)
{
	typedef typename std::remove_reference<decltype(*f.pc_ground_down)>::type Cloud;
	auto fetch = [&](int (*fn)(mulls_ctx *, const mulls_map *, int, void *, uint32_t, uint32_t *), int cls, Cloud &dst, uint32_t n) {
		dst.points.resize(n);
		uint32_t got = 0;
		if (fn(ctx, mir.map, cls, n ? static_cast<void *>(dst.points.data()) : nullptr, n, &got) != MULLS_OK || got != n)
			throw std::runtime_error(std::string("local map download: ") + mulls_last_error(ctx));
	};
	static_assert(sizeof(f.pc_ground_down->points[0]) == MULLS_POINT_BYTES, "download expects 48-byte point records");
	// last_target_cblock->pc_*_down were moved to the map frame and filtered in place by the reference (:32, :37-47)
	Cloud *fd[5] = {f.pc_ground_down.get(), f.pc_pillar_down.get(), f.pc_facade_down.get(), f.pc_beam_down.get(), f.pc_roof_down.get()};
	for (int c = 0; c < 5; c++)
		fetch(mulls_map_frame_download, c, *fd[c], rep.frame_n[c]);
	if (sync_host_map())
	{
		Cloud *mc[6] = {m.pc_ground.get(), m.pc_pillar.get(), m.pc_facade.get(), m.pc_beam.get(), m.pc_roof.get(), m.pc_vertex.get()};
		for (int c = 0; c < 6; c++)
			fetch(mulls_map_download, c, *mc[c], rep.n[c]);
	}
	m.pose_lo = f.pose_lo; // :58-59
	m.pose_gt = f.pose_gt;
	m.local_bound.min_x = rep.local_bound[0], m.local_bound.min_y = rep.local_bound[1], m.local_bound.min_z = rep.local_bound[2];
	m.local_bound.max_x = rep.local_bound[3], m.local_bound.max_y = rep.local_bound[4], m.local_bound.max_z = rep.local_bound[5];
	m.bound.min_x = rep.bound[0], m.bound.min_y = rep.bound[1], m.bound.min_z = rep.bound[2];
	m.bound.max_x = rep.bound[3], m.bound.max_y = rep.bound[4], m.bound.max_z = rep.bound[5];
	m.feature_point_num = rep.feature_point_num; // :128-130
	m.free_tree();								 // :132-133
	m.free_raw_cloud();
	mir.tree_mode = 0; // the kd-trees are gone until the next registration against this map
}
inline bool update_local_map(cloudblock_Ptr local_map, cloudblock_Ptr last_target_cblock, float local_map_radius = 80, int max_num_pts = 20000,
							 int kept_vertex_num = 800, float last_frame_reliable_radius = 60, bool map_based_dynamic_removal_on = false,
							 std::string used_feature_type = "111110", float dynamic_removal_center_radius = 30.0,
							 float dynamic_dist_thre_min = 0.3, float dynamic_dist_thre_max = 3.0, float near_dist_thre = 0.03,
							 bool recalculate_feature_on = false)
{
	mulls_ctx *ctx = thread_context();
	MapMirror &mir = attach_local_map(local_map);
	cloudblock_t &f = *last_target_cblock;
	const mulls_cloud frame[6] = {borrow(f.pc_ground_down), borrow(f.pc_pillar_down), borrow(f.pc_facade_down),
								  borrow(f.pc_beam_down),	borrow(f.pc_roof_down),	  borrow(f.pc_vertex)};
	const mulls_map_params P = map_update_params(mir, local_map_radius, max_num_pts, kept_vertex_num, last_frame_reliable_radius, map_based_dynamic_removal_on,
												 used_feature_type, dynamic_removal_center_radius, dynamic_dist_thre_min, dynamic_dist_thre_max, near_dist_thre,
												 recalculate_feature_on);
	mulls_map_report rep;
	const int rc = mulls_map_update(ctx, mir.map, frame, f.pose_lo.data(), &P, &rep);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_map_update failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	map_update_take(ctx, mir, rep, *local_map, f);
	return true;
}

// update_local_map for several streams at once (several drives replayed side by side, several vehicles): one (local map block, last target block) pair per
// stream and update_local_map's trailing arguments, shared by all.  One mulls_map_update_batch call, every device step once for all streams (mulls_hip.h);
// each stream gets what its own lo::hip::update_local_map call would have left in its two blocks, a seed of map_rng_seed()'s sequence in the streams' order
// included.  The blocks must be distinct.
inline bool update_local_map_batch(const std::vector<std::pair<cloudblock_Ptr, cloudblock_Ptr>> &streams, float local_map_radius = 80, int max_num_pts = 20000,
								   int kept_vertex_num = 800, float last_frame_reliable_radius = 60, bool map_based_dynamic_removal_on = false,
								   std::string used_feature_type = "111110", float dynamic_removal_center_radius = 30.0,
								   float dynamic_dist_thre_min = 0.3, float dynamic_dist_thre_max = 3.0, float near_dist_thre = 0.03,
								   bool recalculate_feature_on = false)
{
	mulls_ctx *ctx = thread_context();
	const size_t n = streams.size();
	std::vector<MapMirror *> mirs(n);
	std::vector<std::array<mulls_cloud, 6>> frames(n);
	std::vector<mulls_map_params> params(n);
	std::vector<mulls_map_update_item> items(n);
	std::vector<mulls_map_batch_result> results(n);
	for (size_t i = 0; i < n; i++)
	{
		mirs[i] = &attach_local_map(streams[i].first); // (std::map: a reference stays valid while others are inserted)
		cloudblock_t &f = *streams[i].second;
		frames[i] = {borrow(f.pc_ground_down), borrow(f.pc_pillar_down), borrow(f.pc_facade_down), borrow(f.pc_beam_down), borrow(f.pc_roof_down), borrow(f.pc_vertex)};
		params[i] = map_update_params(*mirs[i], local_map_radius, max_num_pts, kept_vertex_num, last_frame_reliable_radius, map_based_dynamic_removal_on,
									  used_feature_type, dynamic_removal_center_radius, dynamic_dist_thre_min, dynamic_dist_thre_max, near_dist_thre,
									  recalculate_feature_on);
	}
	for (size_t i = 0; i < n; i++)
	{
		items[i].map = mirs[i]->map;
		items[i].frame_down = frames[i].data();
		std::memcpy(items[i].frame_pose_lo, streams[i].second->pose_lo.data(), sizeof(items[i].frame_pose_lo));
		items[i].params = &params[i];
	}
	const int rc = mulls_map_update_batch(ctx, items.data(), (uint32_t)n, nullptr, 0, results.data(), nullptr);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_map_update_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (size_t i = 0; i < n; i++)
		map_update_take(ctx, *mirs[i], results[i].report, *streams[i].first, *streams[i].second);
	return true;
}

// ------------------------------------------------------------------------------------------------------------------
// Feature extraction: CFilter<PointT>::fast_ground_filter (include/common/cfilter.hpp:1658-2036) and
// CFilter<PointT>::classify_nground_pts (:2058-2290), verbatim signatures.  The binding a maintainer adds is one early return at the top of
// each member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::fast_ground_filter<PointT>(cloud_in, cloud_ground, cloud_ground_down, cloud_unground, cloud_curb, min_grid_pt_num, ...);
//     #endif
// Differences: what PCL computes inside estimate_ground_normal_method 1 - 3 (NormalEstimationOMP, SACSegmentation) is the library's restatement of
// it (include/mulls_hip.h: mulls_ground_params), fast_ground_filter's cloud_in
// keeps its contents (upstream writes normals and data[3] into it; the clouds handed out carry them), the fixed-number selections are seeded with
// `feature_rng_seed()` (upstream: pcl::RandomSample seeded with time(NULL)), and what pcl::PCA / Eigen compute inside classify_nground_pts is
// the library's restatement.
inline uint64_t &feature_rng_seed()
{
	static uint64_t seed = 0;
	return seed;
}
template <typename PointT, typename CloudPtr>
inline void take_cloud(CloudPtr &dst, const std::vector<unsigned char> &raw, uint32_t n, bool append)
{
	static_assert(sizeof(PointT) == MULLS_POINT_BYTES, "48-byte point records expected");
	const size_t before = append ? dst->points.size() : 0;
	dst->points.resize(before + n);
	if (n)
		std::memcpy(static_cast<void *>(&dst->points[before]), raw.data(), (size_t)n * MULLS_POINT_BYTES);
}
template <typename PointT>
inline bool fast_ground_filter(const typename pcl::PointCloud<PointT>::Ptr &cloud_in, typename pcl::PointCloud<PointT>::Ptr &cloud_ground,
							   typename pcl::PointCloud<PointT>::Ptr &cloud_ground_down, typename pcl::PointCloud<PointT>::Ptr &cloud_unground,
							   typename pcl::PointCloud<PointT>::Ptr &cloud_curb, int min_grid_pt_num, float grid_resolution, float max_height_difference,
							   float neighbor_height_diff, float max_ground_height, int ground_random_down_rate, int ground_random_down_down_rate,
							   int nonground_random_down_rate, int reliable_neighbor_grid_num_thre, int estimate_ground_normal_method,
							   float normal_estimation_radius, int distance_weight_downsampling_method, float standard_distance,
							   bool fixed_num_downsampling = false, int down_ground_fixed_num = 1000, bool detect_curb_or_not = false,
							   float intensity_thre = FLT_MAX, bool apply_grid_wise_outlier_filter = false, float outlier_std_scale = 3.0)
{
	(void)cloud_curb, (void)detect_curb_or_not; // curb detection is commented out upstream (:1990-2010)
	mulls_ctx *ctx = thread_context();
	mulls_ground_params P;
	mulls_ground_default_params(&P);
	P.min_grid_pt_num = min_grid_pt_num;
	P.grid_resolution = grid_resolution;
	P.max_height_difference = max_height_difference;
	P.neighbor_height_diff = neighbor_height_diff;
	P.max_ground_height = max_ground_height;
	P.ground_random_down_rate = ground_random_down_rate;
	P.ground_random_down_down_rate = ground_random_down_down_rate;
	P.nonground_random_down_rate = nonground_random_down_rate;
	P.reliable_neighbor_grid_num_thre = reliable_neighbor_grid_num_thre;
	P.estimate_ground_normal_method = estimate_ground_normal_method;
	P.normal_estimation_radius = normal_estimation_radius;
	P.distance_weight_downsampling_method = distance_weight_downsampling_method;
	P.standard_distance = standard_distance;
	P.fixed_num_downsampling = fixed_num_downsampling;
	P.down_ground_fixed_num = down_ground_fixed_num;
	P.intensity_thre = intensity_thre;
	P.apply_grid_wise_outlier_filter = apply_grid_wise_outlier_filter;
	P.outlier_std_scale = outlier_std_scale;
	P.rng_seed = feature_rng_seed()++;
	const mulls_cloud in = borrow(cloud_in);
	std::vector<unsigned char> g((size_t)in.n * MULLS_POINT_BYTES), gd((size_t)in.n * MULLS_POINT_BYTES), u((size_t)in.n * MULLS_POINT_BYTES);
	uint32_t n_out[3] = {0, 0, 0};
	const int rc = mulls_ground_filter(ctx, in.pts, in.n, in.stride, &P, g.data(), in.n, gd.data(), in.n, u.data(), in.n, n_out);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_ground_filter failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	take_cloud<PointT>(cloud_ground, g, n_out[0], true); // upstream pushes back into the clouds it is given
	take_cloud<PointT>(cloud_ground_down, gd, n_out[1], true);
	take_cloud<PointT>(cloud_unground, u, n_out[2], true);
	return 1;
}
template <typename PointT>
inline bool classify_nground_pts(typename pcl::PointCloud<PointT>::Ptr &cloud_in, typename pcl::PointCloud<PointT>::Ptr &cloud_pillar,
								 typename pcl::PointCloud<PointT>::Ptr &cloud_beam, typename pcl::PointCloud<PointT>::Ptr &cloud_facade,
								 typename pcl::PointCloud<PointT>::Ptr &cloud_roof, typename pcl::PointCloud<PointT>::Ptr &cloud_pillar_down,
								 typename pcl::PointCloud<PointT>::Ptr &cloud_beam_down, typename pcl::PointCloud<PointT>::Ptr &cloud_facade_down,
								 typename pcl::PointCloud<PointT>::Ptr &cloud_roof_down, typename pcl::PointCloud<PointT>::Ptr &cloud_vertex,
								 float neighbor_searching_radius, int neighbor_k, int neigh_k_min, int pca_down_rate, float edge_thre, float planar_thre,
								 float edge_thre_down, float planar_thre_down, int extract_vertex_points_method, float curvature_thre,
								 float vertex_curvature_non_max_radius, float linear_vertical_sin_high_thre, float linear_vertical_sin_low_thre,
								 float planar_vertical_sin_high_thre, float planar_vertical_sin_low_thre, bool fixed_num_downsampling = false,
								 int pillar_down_fixed_num = 200, int facade_down_fixed_num = 800, int beam_down_fixed_num = 200, int roof_down_fixed_num = 100,
								 int unground_down_fixed_num = 20000, float beam_height_max = FLT_MAX, float roof_height_min = -FLT_MAX,
								 float feature_pts_ratio_guess = 0.3, bool sharpen_with_nms = true, bool use_distance_adaptive_pca = false)
{
	mulls_ctx *ctx = thread_context();
	mulls_classify_params P;
	mulls_classify_default_params(&P);
	P.neighbor_searching_radius = neighbor_searching_radius;
	P.neighbor_k = neighbor_k;
	P.neigh_k_min = neigh_k_min;
	P.pca_down_rate = pca_down_rate;
	P.edge_thre = edge_thre, P.planar_thre = planar_thre, P.edge_thre_down = edge_thre_down, P.planar_thre_down = planar_thre_down;
	P.extract_vertex_points_method = extract_vertex_points_method;
	P.curvature_thre = curvature_thre;
	P.vertex_curvature_non_max_radius = vertex_curvature_non_max_radius;
	P.linear_vertical_sin_high_thre = linear_vertical_sin_high_thre, P.linear_vertical_sin_low_thre = linear_vertical_sin_low_thre;
	P.planar_vertical_sin_high_thre = planar_vertical_sin_high_thre, P.planar_vertical_sin_low_thre = planar_vertical_sin_low_thre;
	P.fixed_num_downsampling = fixed_num_downsampling;
	P.sharpen_with_nms = sharpen_with_nms;
	P.use_distance_adaptive_pca = use_distance_adaptive_pca;
	P.pillar_down_fixed_num = pillar_down_fixed_num, P.facade_down_fixed_num = facade_down_fixed_num, P.beam_down_fixed_num = beam_down_fixed_num;
	P.roof_down_fixed_num = roof_down_fixed_num, P.unground_down_fixed_num = unground_down_fixed_num;
	P.beam_height_max = beam_height_max, P.roof_height_min = roof_height_min, P.feature_pts_ratio_guess = feature_pts_ratio_guess;
	P.rng_seed = feature_rng_seed()++;
	const mulls_cloud in = borrow(cloud_in);
	std::vector<unsigned char> raw[MULLS_CL_COUNT];
	void *out[MULLS_CL_COUNT];
	uint32_t cap[MULLS_CL_COUNT], n_out[MULLS_CL_COUNT];
	for (int k = 0; k < MULLS_CL_COUNT; k++)
	{
		raw[k].resize((size_t)in.n * MULLS_POINT_BYTES);
		out[k] = raw[k].data();
		cap[k] = in.n;
	}
	std::vector<unsigned char> after((size_t)in.n * MULLS_POINT_BYTES);
	uint32_t n_after = 0;
	const int rc = mulls_classify_nground(ctx, in.pts, in.n, in.stride, &P, out, cap, n_out, after.data(), &n_after);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_classify_nground failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	take_cloud<PointT>(cloud_in, after, n_after, false); // upstream works on cloud_in itself: thinned first (fixed numbers), normals written into it
	typename pcl::PointCloud<PointT>::Ptr *dst[MULLS_CL_COUNT] = {&cloud_pillar,	  &cloud_beam,		  &cloud_facade,	  &cloud_roof,	&cloud_pillar_down,
																	  &cloud_beam_down, &cloud_facade_down, &cloud_roof_down, &cloud_vertex};
	for (int k = 0; k < MULLS_CL_COUNT; k++)
		take_cloud<PointT>(*dst[k], raw[k], n_out[k], true);
	return 1;
}

// CFilter<PointT>::apply_motion_compensation (include/common/cfilter.hpp:470-491), verbatim signature: the frame's points moved by their time-stamp
// fraction of Tran, in place (mulls_motion_compensate: one upload, one kernel, one download).  test/mulls_slam.cpp:705 binds it with one early return.
template <typename PointT>
inline void apply_motion_compensation(typename pcl::PointCloud<PointT>::Ptr pc_in_out, Eigen::Matrix4d &Tran, float s_ambigous_thre = 0.000)
{
	static_assert(sizeof(PointT) == MULLS_POINT_BYTES, "in-place compensation expects 48-byte pcl::PointXYZINormal records");
	if (pc_in_out->points.empty())
		return;
	mulls_ctx *ctx = thread_context();
	const int rc = mulls_motion_compensate(ctx, pc_in_out->points.data(), static_cast<uint32_t>(pc_in_out->points.size()), MULLS_POINT_BYTES, Tran.data(), s_ambigous_thre);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_motion_compensate failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
}
// CFilter<PointT>::batch_apply_motion_compensation, the in-place overload (cfilter.hpp:519-531), verbatim signature (the argument NAMES are upstream's:
// test/mulls_slam.cpp:706-710 passes facade third and beam fourth, which makes no difference — every cloud gets the same treatment)
template <typename PointT>
inline void batch_apply_motion_compensation(typename pcl::PointCloud<PointT>::Ptr pc_ground, typename pcl::PointCloud<PointT>::Ptr pc_pillar,
											typename pcl::PointCloud<PointT>::Ptr pc_beam, typename pcl::PointCloud<PointT>::Ptr pc_facade,
											typename pcl::PointCloud<PointT>::Ptr pc_roof, typename pcl::PointCloud<PointT>::Ptr pc_vertex, Eigen::Matrix4d &Tran,
											bool undistort_keypoints_or_not = false)
{
	apply_motion_compensation<PointT>(pc_ground, Tran);
	apply_motion_compensation<PointT>(pc_pillar, Tran);
	apply_motion_compensation<PointT>(pc_beam, Tran);
	apply_motion_compensation<PointT>(pc_facade, Tran);
	apply_motion_compensation<PointT>(pc_roof, Tran);
	if (undistort_keypoints_or_not)
		apply_motion_compensation<PointT>(pc_vertex, Tran);
}

// CFilter<PointT>::voxel_downsample (include/common/cfilter.hpp:83-160), verbatim signature
template <typename PointT>
inline bool voxel_downsample(const typename pcl::PointCloud<PointT>::Ptr &cloud_in, typename pcl::PointCloud<PointT>::Ptr &cloud_out, float voxel_size)
{
	if (voxel_size < 0.001)
	{
		cloud_out = cloud_in; // :90-97
		return false;
	}
	mulls_ctx *ctx = thread_context();
	const mulls_cloud in = borrow(cloud_in);
	std::vector<unsigned char> raw((size_t)in.n * MULLS_POINT_BYTES);
	uint32_t n_out = 0;
	const int rc = mulls_voxel_downsample(ctx, in.pts, in.n, in.stride, voxel_size, raw.data(), in.n, &n_out);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_voxel_downsample failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	take_cloud<PointT>(cloud_out, raw, n_out, true); // `cloud_out->push_back(...)`: appended (:147)
	return 1;
}

// CRegistration<PointT>::find_feature_correspondence_ncc (include/common/cregistration.hpp:409-601), verbatim signature and defaults: the correspondence
// stage of the global (coarse) registration (test/mulls_reg.cpp:173-174, test/mulls_slam.cpp:532-540) in one device call (mulls_ncc_correspond).  The
// binding is one early return at the top of the member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::find_feature_correspondence_ncc<PointT>(target_kpts, source_kpts, target_corrs, source_corrs, fixed_num_corr, corr_num, reciprocal_on);
//     #endif
// The matched key points are appended to target_corrs / source_corrs (upstream push_backs).  With fixed_num_corr, pairs at exactly equal descriptor distances
// come in ascending (target index, source index) order — upstream's unstable std::sort leaves that order open (include/mulls_hip.h).  The solver behind it
// is coarse_reg_teaser or coarse_reg_ransac below.
template <typename PointT>
inline bool find_feature_correspondence_ncc(const typename pcl::PointCloud<PointT>::Ptr &target_kpts, const typename pcl::PointCloud<PointT>::Ptr &source_kpts,
											typename pcl::PointCloud<PointT>::Ptr &target_corrs, typename pcl::PointCloud<PointT>::Ptr &source_corrs,
											bool fixed_num_corr = false, int corr_num = 2000, bool reciprocal_on = true)
{
	mulls_ctx *ctx = thread_context();
	const mulls_cloud tgt = borrow(target_kpts), src = borrow(source_kpts);
	mulls_ncc_params P;
	mulls_ncc_default_params(&P);
	P.fixed_num_corr = fixed_num_corr ? 1 : 0;
	P.corr_num = corr_num;
	P.reciprocal_on = reciprocal_on ? 1 : 0;
	const uint32_t cap = fixed_num_corr ? (uint32_t)(corr_num > 0 ? corr_num : 0) : tgt.n;
	std::vector<int32_t> ti(cap ? cap : 1), si(cap ? cap : 1);
	uint32_t n = 0;
	const int rc = mulls_ncc_correspond(ctx, &tgt, &src, &P, ti.data(), si.data(), cap, &n);
	if (rc < 0)
		throw std::runtime_error(std::string("mulls_ncc_correspond failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (uint32_t k = 0; k < n && k < cap; k++)
	{
		target_corrs->points.push_back(target_kpts->points[ti[k]]); // :547-548, :584-585
		source_corrs->points.push_back(source_kpts->points[si[k]]);
	}
	return rc != 0;
}

// Many find_feature_correspondence_ncc calls in one (mulls_ncc_correspond_batch): the candidate edges of a loop-closure event (test/mulls_slam.cpp:517-557
// matches them one after another) or one scan against a list of submaps.  Pair k is target_kpts[k] / source_kpts[k]; target_corrs[k], source_corrs[k] and
// ok[k] are what find_feature_correspondence_ncc<PointT>(target_kpts[k], source_kpts[k], target_corrs[k], source_corrs[k], fixed_num_corr, corr_num,
// reciprocal_on) appends and returns.  The four cloud vectors have one length, the output clouds exist (they are appended to, as upstream push_backs); ok is
// resized.  The same cloud pointer in several pairs is uploaded once.  INTEGRATION.md shows it chained into coarse_reg_teaser_batch.
template <typename PointT>
inline void find_feature_correspondence_ncc_batch(const std::vector<typename pcl::PointCloud<PointT>::Ptr> &target_kpts,
												  const std::vector<typename pcl::PointCloud<PointT>::Ptr> &source_kpts,
												  std::vector<typename pcl::PointCloud<PointT>::Ptr> &target_corrs,
												  std::vector<typename pcl::PointCloud<PointT>::Ptr> &source_corrs, std::vector<bool> &ok, bool fixed_num_corr = false,
												  int corr_num = 2000, bool reciprocal_on = true)
{
	const size_t B = target_kpts.size();
	if (source_kpts.size() != B || target_corrs.size() != B || source_corrs.size() != B)
		throw std::invalid_argument("find_feature_correspondence_ncc_batch: the four cloud vectors must have one length");
	mulls_ctx *ctx = thread_context();
	mulls_ncc_params P;
	mulls_ncc_default_params(&P);
	P.fixed_num_corr = fixed_num_corr ? 1 : 0;
	P.corr_num = corr_num;
	P.reciprocal_on = reciprocal_on ? 1 : 0;
	std::vector<mulls_ncc_problem> problems(B);
	std::vector<std::vector<int32_t>> ti(B), si(B);
	for (size_t k = 0; k < B; k++)
	{
		problems[k] = mulls_ncc_problem();
		problems[k].tgt = borrow(target_kpts[k]);
		problems[k].src = borrow(source_kpts[k]);
		const uint32_t cap = fixed_num_corr ? (uint32_t)(corr_num > 0 ? corr_num : 0) : problems[k].tgt.n;
		ti[k].resize(cap ? cap : 1), si[k].resize(cap ? cap : 1);
		problems[k].tgt_idx = ti[k].data(), problems[k].src_idx = si[k].data(), problems[k].cap = cap;
	}
	std::vector<mulls_ncc_result> R(B ? B : 1);
	const int rc = mulls_ncc_correspond_batch(ctx, problems.data(), (uint32_t)B, &P, 0, R.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_ncc_correspond_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	ok.assign(B, false);
	for (size_t k = 0; k < B; k++)
	{
		for (uint32_t c = 0; c < R[k].n_corr && c < problems[k].cap; c++)
		{
			target_corrs[k]->points.push_back(target_kpts[k]->points[ti[k][c]]); // :547-548, :584-585
			source_corrs[k]->points.push_back(source_kpts[k]->points[si[k][c]]);
		}
		ok[k] = R[k].ret != 0;
	}
}

// CRegistration<PointT>::coarse_reg_ransac (include/common/cregistration.hpp:605-661), verbatim signature and defaults: the RANSAC solver of the global (coarse)
// registration (test/mulls_reg.cpp:179, test/mulls_slam.cpp:538) in one device call (mulls_coarse_reg_ransac).  The binding is one early return at the top of the
// member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::coarse_reg_ransac<PointT>(target_pts, source_pts, tran_mat, noise_bound, min_inlier_num, max_iter_num);
//     #endif
// Returns upstream's 1 (reliable) / 0 (need check) / -1 (failed); tran_mat is written only when the result is not -1, as upstream.  Where PCL's result rests
// on Eigen's decompositions this library defines its own (include/mulls_hip.h): the transform is the library's, not PCL's bits.
template <typename PointT>
inline int coarse_reg_ransac(const typename pcl::PointCloud<PointT>::Ptr &target_pts, const typename pcl::PointCloud<PointT>::Ptr &source_pts,
							 Eigen::Matrix4d &tran_mat, float noise_bound = 0.2, int min_inlier_num = 8, int max_iter_num = 20000)
{
	mulls_ctx *ctx = thread_context();
	const mulls_cloud tgt = borrow(target_pts), src = borrow(source_pts);
	mulls_ransac_params P;
	mulls_ransac_default_params(&P);
	P.noise_bound = noise_bound;
	P.min_inlier_num = min_inlier_num;
	P.max_iter_num = max_iter_num;
	mulls_ransac_result R;
	const int rc = mulls_coarse_reg_ransac(ctx, &tgt, &src, &P, &R, nullptr, 0);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_coarse_reg_ransac failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	if (R.status >= 0)
		for (int c = 0; c < 4; c++)
			for (int r = 0; r < 4; r++)
				tran_mat(r, c) = R.T[c * 4 + r];
	return R.status;
}

// Many coarse_reg_ransac calls in one (mulls_coarse_reg_ransac_batch): the candidate edges of a loop-closure event under
// --teaser_based_global_registration_on=false (test/mulls_slam.cpp:517-557 solves them one after another until one is accepted).  Pair k is targets[k] /
// sources[k] with trans[k]; the return value's entry k and trans[k] are what coarse_reg_ransac<PointT>(targets[k], sources[k], trans[k], noise_bound,
// min_inlier_num, max_iter_num) returns and writes (trans[k] is untouched on -1).  The three vectors have one length.  INTEGRATION.md shows the loop
// restructured around it.
template <typename PointT>
inline std::vector<int> coarse_reg_ransac_batch(const std::vector<typename pcl::PointCloud<PointT>::Ptr> &targets,
												const std::vector<typename pcl::PointCloud<PointT>::Ptr> &sources, std::vector<Eigen::Matrix4d> &trans,
												float noise_bound = 0.2, int min_inlier_num = 8, int max_iter_num = 20000)
{
	if (targets.size() != sources.size() || targets.size() != trans.size())
		throw std::invalid_argument("coarse_reg_ransac_batch: targets, sources and trans must have one length");
	mulls_ctx *ctx = thread_context();
	std::vector<mulls_ransac_problem> problems(targets.size());
	for (size_t k = 0; k < targets.size(); k++)
	{
		problems[k] = mulls_ransac_problem();
		problems[k].tgt = borrow(targets[k]);
		problems[k].src = borrow(sources[k]);
	}
	mulls_ransac_params P;
	mulls_ransac_default_params(&P);
	P.noise_bound = noise_bound;
	P.min_inlier_num = min_inlier_num;
	P.max_iter_num = max_iter_num;
	std::vector<mulls_ransac_result> R(targets.size());
	const int rc = mulls_coarse_reg_ransac_batch(ctx, problems.data(), (uint32_t)problems.size(), &P, 0, R.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_coarse_reg_ransac_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	std::vector<int> status(targets.size());
	for (size_t k = 0; k < targets.size(); k++)
	{
		status[k] = R[k].status;
		if (R[k].status >= 0)
			for (int c = 0; c < 4; c++)
				for (int r = 0; r < 4; r++)
					trans[k](r, c) = R[k].T[c * 4 + r];
	}
	return status;
}

// CRegistration<PointT>::coarse_reg_teaser (include/common/cregistration.hpp:664-759), verbatim signature and defaults: the TEASER solver of the global (coarse)
// registration every shipped configuration selects (test/mulls_reg.cpp:177, test/mulls_slam.cpp:537) in one call (mulls_coarse_reg_teaser).  The binding is
// one early return at the top of the member function, outside upstream's `#if TEASER_ON`: the bridge always solves, where upstream compiles the body out
// and returns -1 without TEASER++:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::coarse_reg_teaser<PointT>(target_pts, source_pts, tran_mat, noise_bound, min_inlier_num);
//     #endif
// Returns upstream's 1 (reliable) / 0 (need check) / -1 (failed; also unequal sizes and three pairs or fewer); tran_mat is untouched on -1, as upstream.
// The maximum clique is the lexicographically smallest one and the rotation fit is the library's (include/mulls_hip.h): the transform is not TEASER++'s bits.
template <typename PointT>
inline int coarse_reg_teaser(const typename pcl::PointCloud<PointT>::Ptr &target_pts, const typename pcl::PointCloud<PointT>::Ptr &source_pts,
							 Eigen::Matrix4d &tran_mat, float noise_bound = 0.2, int min_inlier_num = 8)
{
	mulls_ctx *ctx = thread_context();
	const mulls_cloud tgt = borrow(target_pts), src = borrow(source_pts);
	mulls_teaser_params P;
	mulls_teaser_default_params(&P);
	P.noise_bound = noise_bound;
	P.min_inlier_num = min_inlier_num;
	mulls_teaser_result R;
	const int rc = mulls_coarse_reg_teaser(ctx, &tgt, &src, &P, &R, nullptr, 0);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_coarse_reg_teaser failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	if (R.status >= 0)
		for (int c = 0; c < 4; c++)
			for (int r = 0; r < 4; r++)
				tran_mat(r, c) = R.T[c * 4 + r];
	return R.status;
}

// Many coarse_reg_teaser calls in one (mulls_coarse_reg_teaser_batch): the candidate edges of a loop-closure event (test/mulls_slam.cpp:517-557 solves them
// one after another until one is accepted) or one scan against a list of submaps.  Pair k is targets[k] / sources[k] with trans[k]; the return value's
// entry k and trans[k] are what coarse_reg_teaser<PointT>(targets[k], sources[k], trans[k], noise_bound, min_inlier_num) returns and writes (trans[k] is
// untouched on -1).  The three vectors have one length.  INTEGRATION.md shows the loop restructured around it.
template <typename PointT>
inline std::vector<int> coarse_reg_teaser_batch(const std::vector<typename pcl::PointCloud<PointT>::Ptr> &targets,
												const std::vector<typename pcl::PointCloud<PointT>::Ptr> &sources, std::vector<Eigen::Matrix4d> &trans,
												float noise_bound = 0.2, int min_inlier_num = 8)
{
	if (targets.size() != sources.size() || targets.size() != trans.size())
		throw std::invalid_argument("coarse_reg_teaser_batch: targets, sources and trans must have one length");
	mulls_ctx *ctx = thread_context();
	std::vector<mulls_teaser_problem> problems(targets.size());
	for (size_t k = 0; k < targets.size(); k++)
	{
		problems[k] = mulls_teaser_problem();
		problems[k].tgt = borrow(targets[k]);
		problems[k].src = borrow(sources[k]);
	}
	mulls_teaser_params P;
	mulls_teaser_default_params(&P);
	P.noise_bound = noise_bound;
	P.min_inlier_num = min_inlier_num;
	std::vector<mulls_teaser_result> R(targets.size());
	const int rc = mulls_coarse_reg_teaser_batch(ctx, problems.data(), (uint32_t)problems.size(), &P, 0, R.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_coarse_reg_teaser_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	std::vector<int> status(targets.size());
	for (size_t k = 0; k < targets.size(); k++)
	{
		status[k] = R[k].status;
		if (R[k].status >= 0)
			for (int c = 0; c < 4; c++)
				for (int r = 0; r < 4; r++)
					trans[k](r, c) = R[k].T[c * 4 + r];
	}
	return status;
}

// GlobalOptimize::optimize_pose_graph_ceres (src/graph_optimizer.cpp:385-417) in one device call (mulls_pgo_optimize): the nodes are the blocks in
// their order (a constraint's ends are found by block1 / block2 ->id_in_strip, as upstream's set_pgo_problem_ceres does), pose_init goes in, pose_optimized
// comes out.  t_limit / r_limit are upstream's moving_threshold_tran / _rot; params carries what upstream sets through GlobalOptimize's setters
// (set_robust_function, set_equal_weight, set_max_iter_num, set_diagonal_information_matrix, set_free_node; set_problem_size has no counterpart: there is one
// linear solver).  Returns upstream's bool: false — with pose_optimized untouched — when there are too few edges or the initial cost is not finite; with
// update_edge_or_not, false also when the edge check fails (update_optimized_edges, :713-776).  The consequences upstream draws there are applied here,
// since the library changes no edge: a wrong REGISTRATION edge's con_type becomes NONE, and when the check passes every ADJACENT edge's
// information_matrix takes the covariance ratio (first_time_updating_ratio the first time, life_long_updating_ratio afterwards; both 1.0 upstream).
// update_optimized_edges' second argument, fixed_reg_edge, which gates that ratio, is taken at its default true: upstream's only call passes none.
// include/mulls_hip.h says which lines of the definition are upstream's, which restate Ceres (from its documentation, not compared) and which are the library's.
namespace detail
{
template <typename Constraints>
inline void pgo_fill(const cloudblock_Ptrs &blocks, const Constraints &cons, std::vector<mulls_pgo_node> &nodes, std::vector<mulls_pgo_edge> &edges)
{
	nodes.assign(blocks.size(), mulls_pgo_node());
	for (size_t i = 0; i < blocks.size(); i++)
	{
		std::memcpy(nodes[i].pose_init, blocks[i]->pose_init.data(), sizeof(nodes[i].pose_init));
		nodes[i].fixed = blocks[i]->pose_fixed ? 1 : 0;
		nodes[i].stable = blocks[i]->pose_stable ? 1 : 0;
	}
	edges.assign(cons.size(), mulls_pgo_edge());
	for (size_t k = 0; k < cons.size(); k++)
	{
		edges[k].a = cons[k].block1->id_in_strip;
		edges[k].b = cons[k].block2->id_in_strip;
		edges[k].type = (int32_t)cons[k].con_type;
		std::memcpy(edges[k].T, cons[k].Trans1_2.data(), sizeof(edges[k].T));
		for (int c = 0; c < 6; c++)
			for (int r = 0; r < 6; r++)
				edges[k].info[r + 6 * c] = cons[k].information_matrix(r, c);
	}
}
template <typename Constraints>
inline bool pgo_take(const mulls_pgo_result &R, const double *poses, const uint8_t *wrong, cloudblock_Ptrs &blocks, Constraints &cons, bool update_edge_or_not,
					 float first_time_updating_ratio, float life_long_updating_ratio)
{
	if (R.status != 1)
		return false;
	for (size_t i = 0; i < blocks.size(); i++)
		for (int c = 0; c < 4; c++)
			for (int r = 0; r < 4; r++)
				blocks[i]->pose_optimized(r, c) = poses[16 * i + 4 * c + r];
	if (!update_edge_or_not)
		return true;
	for (size_t k = 0; k < cons.size(); k++)
		if (wrong[k] && cons[k].con_type == REGISTRATION)
			cons[k].con_type = NONE;
	if (!R.edges_ok)
		return false;
	for (size_t k = 0; k < cons.size(); k++)
		if (cons[k].con_type == ADJACENT)
		{
			const double ratio = cons[k].cov_updated ? life_long_updating_ratio : first_time_updating_ratio;
			for (int c = 0; c < 6; c++)
				for (int r = 0; r < 6; r++)
					cons[k].information_matrix(r, c) = ratio * cons[k].information_matrix(r, c);
			cons[k].cov_updated = true;
		}
	return true;
}
} // namespace detail

inline mulls_pgo_params pgo_params()
{
	mulls_pgo_params P;
	mulls_pgo_default_params(&P);
	return P;
}

// (Constraints: upstream's `constraints`, the aligned vector of constraint_t; a template parameter because that typedef follows the types this header is included behind)
template <typename Constraints>
inline bool optimize_pose_graph(mulls_ctx *ctx, cloudblock_Ptrs &all_blocks, Constraints &all_cons, double t_limit, double r_limit,
								bool update_edge_or_not = true, mulls_pgo_params params = pgo_params(), float first_time_updating_ratio = 1.0f,
								float life_long_updating_ratio = 1.0f)
{
	std::vector<mulls_pgo_node> nodes;
	std::vector<mulls_pgo_edge> edges;
	detail::pgo_fill(all_blocks, all_cons, nodes, edges);
	params.t_limit = t_limit, params.r_limit = r_limit;
	std::vector<double> poses(16 * nodes.size() + 1);
	std::vector<uint8_t> wrong(edges.size() + 1);
	mulls_pgo_result R;
	const int rc = mulls_pgo_optimize(ctx, nodes.data(), (uint32_t)nodes.size(), edges.data(), (uint32_t)edges.size(), &params, poses.data(), wrong.data(), &R);
	if (rc != MULLS_OK) // infrastructure failure or refused arguments: the reference has no channel for it
		throw std::runtime_error(std::string("mulls_pgo_optimize failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	return detail::pgo_take(R, poses.data(), wrong.data(), all_blocks, all_cons, update_edge_or_not, first_time_updating_ratio, life_long_updating_ratio);
}

// The inner-submap loop of test/mulls_slam.cpp:885-926 in one call (mulls_pgo_optimize_batch): problem k is (*graphs[k].first, *graphs[k].second), one
// chain of frames per submap.  Entry k of the return value is what optimize_pose_graph returns for it; the blocks and constraints are written as there.
template <typename Constraints>
inline std::vector<bool> optimize_pose_graph_batch(mulls_ctx *ctx, std::vector<std::pair<cloudblock_Ptrs *, Constraints *>> &graphs, double t_limit,
												   double r_limit, bool update_edge_or_not = false, mulls_pgo_params params = pgo_params(),
												   float first_time_updating_ratio = 1.0f, float life_long_updating_ratio = 1.0f)
{
	const size_t B = graphs.size();
	std::vector<std::vector<mulls_pgo_node>> nodes(B);
	std::vector<std::vector<mulls_pgo_edge>> edges(B);
	std::vector<std::vector<double>> poses(B);
	std::vector<std::vector<uint8_t>> wrong(B);
	std::vector<mulls_pgo_problem> problems(B);
	for (size_t k = 0; k < B; k++)
	{
		detail::pgo_fill(*graphs[k].first, *graphs[k].second, nodes[k], edges[k]);
		poses[k].resize(16 * nodes[k].size() + 1);
		wrong[k].resize(edges[k].size() + 1);
		problems[k].nodes = nodes[k].data(), problems[k].n_nodes = (uint32_t)nodes[k].size();
		problems[k].edges = edges[k].data(), problems[k].n_edges = (uint32_t)edges[k].size();
		problems[k].poses_out = poses[k].data(), problems[k].edge_wrong = wrong[k].data();
	}
	params.t_limit = t_limit, params.r_limit = r_limit;
	std::vector<mulls_pgo_result> R(B);
	const int rc = mulls_pgo_optimize_batch(ctx, problems.data(), (uint32_t)B, &params, 0, R.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_pgo_optimize_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	std::vector<bool> ok(B);
	for (size_t k = 0; k < B; k++)
		ok[k] = detail::pgo_take(R[k], poses[k].data(), wrong[k].data(), *graphs[k].first, *graphs[k].second, update_edge_or_not, first_time_updating_ratio,
								 life_long_updating_ratio);
	return ok;
}

// The submap archive (mulls_submaps_*): cblock_submaps[i] is submap i of `store`, pushed in that order.
// submaps_push is the deep copy of test/mulls_slam.cpp:454 (and, with vertex_nms_radius > 0, the non_max_suppress of :462) into the store: the block's six
// class clouds, pose_lo and id_in_strip go to the device once; later registrations take them from mulls_submaps_cloud / mulls_submaps_pairs.  The block's
// local_bound and bound are set to what the store holds.  update_optimized_nodes (src/graph_optimizer.cpp:778-798) and
// find_overlap_registration_constraint (src/build_pose_graph.cpp:123-209) keep upstream's remaining arguments and write the blocks and constraints as upstream
// does; the bounds come from the device and the overlap search reads the store's poses and bounds, which these functions keep equal to the blocks'.
// include/mulls_hip.h says which lines of the definition are upstream's and which are the library's.
inline mulls_submap_info submaps_push(mulls_ctx *ctx, mulls_submaps *store, const cloudblock_Ptr &block, float vertex_nms_radius = 0.0f)
{
	const mulls_cloud clouds[MULLS_NCLASS] = {borrow(block->pc_ground), borrow(block->pc_pillar), borrow(block->pc_facade),
											  borrow(block->pc_beam),	borrow(block->pc_roof),	  borrow(block->pc_vertex)};
	mulls_submap_info info;
	const int rc = mulls_submaps_push(ctx, store, clouds, block->pose_lo.data(), block->id_in_strip, vertex_nms_radius, &info);
	if (rc != MULLS_OK) // a full store included: the reference has no channel for it
		throw std::runtime_error(std::string("mulls_submaps_push failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	block->local_bound.min_x = info.local_bound[0], block->local_bound.min_y = info.local_bound[1], block->local_bound.min_z = info.local_bound[2];
	block->local_bound.max_x = info.local_bound[3], block->local_bound.max_y = info.local_bound[4], block->local_bound.max_z = info.local_bound[5];
	block->bound.min_x = info.bound[0], block->bound.min_y = info.bound[1], block->bound.min_z = info.bound[2];
	block->bound.max_x = info.bound[3], block->bound.max_y = info.bound[4], block->bound.max_z = info.bound[5];
	return info;
}

inline bool update_optimized_nodes(mulls_ctx *ctx, mulls_submaps *store, cloudblock_Ptrs &all_blocks, bool update_init_pose = false, bool update_bbx = false)
{
	std::vector<double> poses(16 * all_blocks.size() + 1);
	for (size_t i = 0; i < all_blocks.size(); i++)
	{
		all_blocks[i]->pose_lo = all_blocks[i]->pose_optimized;
		if (update_init_pose)
			all_blocks[i]->pose_init = all_blocks[i]->pose_lo;
		std::memcpy(&poses[16 * i], all_blocks[i]->pose_lo.data(), 16 * sizeof(double));
	}
	const int rc = mulls_submaps_set_poses(ctx, store, 0, (uint32_t)all_blocks.size(), poses.data(), update_bbx ? 1 : 0);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_submaps_set_poses failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (size_t i = 0; update_bbx && i < all_blocks.size(); i++)
	{
		mulls_submap_info info;
		if (mulls_submaps_info(ctx, store, (uint32_t)i, &info) != MULLS_OK)
			throw std::runtime_error(std::string("mulls_submaps_info failed: ") + mulls_last_error(ctx));
		all_blocks[i]->bound.min_x = info.bound[0], all_blocks[i]->bound.min_y = info.bound[1], all_blocks[i]->bound.min_z = info.bound[2];
		all_blocks[i]->bound.max_x = info.bound[3], all_blocks[i]->bound.max_y = info.bound[4], all_blocks[i]->bound.max_z = info.bound[5];
	}
	return true;
}

// (Constraints: upstream's `constraints`, as for optimize_pose_graph.)  The new edges are appended to cons and cons is sorted as a whole, as upstream does;
// equal ratios keep their order.
template <typename Constraints>
inline int find_overlap_registration_constraint(mulls_ctx *ctx, mulls_submaps *store, cloudblock_Ptrs &blocks, Constraints &cons, float neighbor_radius = 50.0,
												float min_iou_thre = 0.25, int adjacent_id_thre = 3, bool search_neighbor_2d = true, int max_neighbor = 10)
{
	if (blocks.empty())
		return 0;
	mulls_overlap_params P;
	mulls_overlap_default_params(&P);
	P.neighbor_search_dist = neighbor_radius, P.min_iou_thre = min_iou_thre, P.adjacent_id_thre = adjacent_id_thre;
	P.search_2d = search_neighbor_2d ? 1 : 0, P.max_neighbor = max_neighbor;
	const uint32_t cur = (uint32_t)blocks.size() - 1u;
	std::vector<mulls_submap_edge> edges(blocks.size());
	uint32_t n = 0;
	const int rc = mulls_submaps_find_overlap(ctx, store, cur, &P, edges.data(), (uint32_t)edges.size(), &n);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_submaps_find_overlap failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (uint32_t k = 0; k < n; k++)
	{
		typename Constraints::value_type registration_con;
		registration_con.block1 = blocks[(size_t)edges[k].tgt_id]; // history map (target)
		registration_con.block2 = blocks[(size_t)edges[k].src_id]; // current map (source)
		registration_con.con_type = REGISTRATION;
		std::memcpy(registration_con.Trans1_2.data(), edges[k].Trans1_2, 16 * sizeof(double));
		registration_con.overlapping_ratio = edges[k].overlapping_ratio;
		cons.push_back(registration_con);
	}
	std::stable_sort(cons.begin(), cons.end(), [](const typename Constraints::value_type &a, const typename Constraints::value_type &b) { return a.overlapping_ratio > b.overlapping_ratio; });
	return (int)n;
}

// CFilter<PointT>::sor_filter (include/common/cfilter.hpp:204-222 and :225-247), verbatim signatures (upstream gives no defaults): the statistical
// outlier removal of the merged map mulls_slam exports (test/mulls_slam.cpp:1008-1009, `cf.sor_filter(pc_map_merged, 20, 2.0)` under --map_filter_on) in one
// device call (mulls_sor_filter).  The binding is one early return at the top of each member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::sor_filter<PointT>(cloud_in, cloud_out, mean_k, n_std);      // resp. (cloud_in_out, mean_k, n_std)
//     #endif
// cloud_out is overwritten, as pcl::Filter::filter does.  Upstream's body is pcl::StatisticalOutlierRemoval; include/mulls_hip.h says which lines of the
// definition are PCL's (restated from memory, not compared) and which are the library's.  A cloud of 1 .. mean_k points, on which PCL reads past its
// neighbour search's result, throws here, as do non-finite coordinates.
template <typename PointT>
inline bool sor_filter(typename pcl::PointCloud<PointT>::Ptr &cloud_in, typename pcl::PointCloud<PointT>::Ptr &cloud_out, int mean_k, double n_std)
{
	mulls_ctx *ctx = thread_context();
	const mulls_cloud in = borrow(cloud_in);
	mulls_sor_params P;
	mulls_sor_default_params(&P);
	P.mean_k = mean_k;
	P.std_mul = n_std;
	std::vector<unsigned char> raw((size_t)in.n * MULLS_POINT_BYTES);
	uint32_t n_out = 0;
	const int rc = mulls_sor_filter(ctx, &in, &P, raw.data(), in.n, &n_out, nullptr, 0, nullptr, nullptr);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_sor_filter failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	take_cloud<PointT>(cloud_out, raw, n_out, false);
	return 1;
}
template <typename PointT>
inline bool sor_filter(typename pcl::PointCloud<PointT>::Ptr &cloud_in_out, int mean_k, double n_std)
{
	typename pcl::PointCloud<PointT>::Ptr cloud_temp(new pcl::PointCloud<PointT>());
	sor_filter<PointT>(cloud_in_out, cloud_temp, mean_k, n_std);
	cloud_temp->points.swap(cloud_in_out->points); // :239
	return 1;
}

// CFilter<PointT>::non_max_suppress (include/common/cfilter.hpp:1183-1240 and :1243-1312), verbatim signatures and defaults: the thinning of the key points
// in front of the global registration (test/mulls_reg.cpp:147-148) and of loop closure (test/mulls_slam.cpp:462) in one device call
// (mulls_non_max_suppress).  The binding is one early return at the top of each member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::non_max_suppress<PointT>(cloud_in_out, non_max_radius, kd_tree_already_built, built_tree);
//     #endif
// In place: the cloud becomes the kept points, in visiting order.  Out of place: cloud_in is left sorted, as upstream's std::sort leaves it, and the kept
// points are appended to cloud_out (upstream push_backs).  Both return false and touch nothing below 10 points.  distance_adaptive_on (set by no upstream
// call site) and kd_tree_already_built (upstream would query a tree over the unsorted cloud with sorted indices; mulls_slam.cpp:462 passes false) throw.
// A NaN key (normal[3]), on which upstream's sort is undefined, throws too, as do non-finite coordinates.
template <typename PointT>
inline bool non_max_suppress(typename pcl::PointCloud<PointT>::Ptr &cloud_in, typename pcl::PointCloud<PointT>::Ptr &cloud_out, float nms_radius,
							 bool distance_adaptive_on = false, float unit_dist = 35.0, bool kd_tree_already_built = false,
							 const typename pcl::search::KdTree<PointT>::Ptr &built_tree = NULL)
{
	(void)unit_dist, (void)built_tree;
	if (distance_adaptive_on || kd_tree_already_built)
		throw std::runtime_error("lo::hip::non_max_suppress: distance_adaptive_on and kd_tree_already_built are not supported");
	if (cloud_in->points.size() < 10) // :1251-1253
		return false;
	mulls_ctx *ctx = thread_context();
	const mulls_cloud in = borrow(cloud_in);
	mulls_nms_params P;
	mulls_nms_default_params(&P);
	P.non_max_radius = nms_radius;
	std::vector<unsigned char> raw((size_t)in.n * MULLS_POINT_BYTES);
	std::vector<int32_t> order(in.n);
	uint32_t n_out = 0;
	const int rc = mulls_non_max_suppress(ctx, &in, &P, raw.data(), in.n, &n_out, nullptr, 0, order.data(), nullptr);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_non_max_suppress failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	typename std::remove_reference<decltype(cloud_in->points)>::type sorted(in.n);
	for (uint32_t i = 0; i < in.n; i++)
		sorted[i] = cloud_in->points[order[i]]; // :1255
	cloud_in->points.swap(sorted);
	take_cloud<PointT>(cloud_out, raw, n_out, true); // :1280
	return true;
}
template <typename PointT>
inline bool non_max_suppress(typename pcl::PointCloud<PointT>::Ptr &cloud_in_out, float non_max_radius, bool kd_tree_already_built = false,
							 const typename pcl::search::KdTree<PointT>::Ptr &built_tree = NULL)
{
	(void)built_tree;
	if (kd_tree_already_built)
		throw std::runtime_error("lo::hip::non_max_suppress: kd_tree_already_built is not supported");
	if (cloud_in_out->points.size() < 10) // :1189-1191
		return false;
	mulls_ctx *ctx = thread_context();
	const mulls_cloud in = borrow(cloud_in_out);
	mulls_nms_params P;
	mulls_nms_default_params(&P);
	P.non_max_radius = non_max_radius;
	std::vector<unsigned char> raw((size_t)in.n * MULLS_POINT_BYTES);
	uint32_t n_out = 0;
	const int rc = mulls_non_max_suppress(ctx, &in, &P, raw.data(), in.n, &n_out, nullptr, 0, nullptr, nullptr);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_non_max_suppress failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	take_cloud<PointT>(cloud_in_out, raw, n_out, false); // :1230
	return true;
}
// The in-place overload applied to every cloud of a vector in one device call (mulls_non_max_suppress_batch): the key points of every scan of an event,
// or both clouds of mulls_reg.cpp:147-148.  ok[k] is what the in-place overload returns for cloud k (false, and the cloud untouched, below 10 points).
// The refusals are the single bridge's: distance_adaptive_on and kd_tree_already_built throw, as does a cloud the single call refuses (a NaN key, a
// non-finite coordinate); no cloud is changed then.
template <typename PointT>
inline std::vector<bool> non_max_suppress_batch(std::vector<typename pcl::PointCloud<PointT>::Ptr> &clouds_in_out, float non_max_radius,
												 bool distance_adaptive_on = false, bool kd_tree_already_built = false)
{
	if (distance_adaptive_on || kd_tree_already_built)
		throw std::runtime_error("lo::hip::non_max_suppress_batch: distance_adaptive_on and kd_tree_already_built are not supported");
	const size_t B = clouds_in_out.size();
	std::vector<bool> ok(B, false);
	if (B == 0)
		return ok;
	mulls_ctx *ctx = thread_context();
	mulls_nms_params P;
	mulls_nms_default_params(&P);
	P.non_max_radius = non_max_radius;
	std::vector<mulls_nms_problem> problems(B);
	std::vector<mulls_nms_report> reports(B);
	std::vector<std::vector<unsigned char>> raw(B);
	for (size_t k = 0; k < B; k++)
	{
		mulls_nms_problem &Q = problems[k];
		Q.cloud = borrow(clouds_in_out[k]);
		raw[k].resize((size_t)Q.cloud.n * MULLS_POINT_BYTES);
		Q.out = raw[k].empty() ? nullptr : raw[k].data();
		Q.cap = Q.cloud.n;
		Q.kept_idx = nullptr, Q.order = nullptr, Q.idx_cap = 0;
	}
	const int rc = mulls_non_max_suppress_batch(ctx, problems.data(), static_cast<uint32_t>(B), &P, 0, reports.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_non_max_suppress_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (size_t k = 0; k < B; k++)
	{
		if (clouds_in_out[k]->points.size() < 10) // :1189-1191
			continue;
		take_cloud<PointT>(clouds_in_out[k], raw[k], reports[k].n_kept, false); // :1230
		ok[k] = true;
	}
	return ok;
}

// The raw-scan steps of CFilter<PointT> in front of extract_semantic_pts and of the map export (test/mulls_slam.cpp:359-362, :404-412, :966-974), verbatim
// signatures and defaults, each one device call on the cloud's records in place (mulls_scan_prepare with one step switched on; a caller that owns the
// sequence fills mulls_scan_prep_params itself and runs all of them in one call).  include/mulls_hip.h has the definition.  The binding is one early
// return at the top of each member function.
template <typename PointT>
inline uint32_t scan_prepare(typename pcl::PointCloud<PointT>::Ptr &cloud_in_out, const mulls_scan_prep_params &P)
{
	static_assert(sizeof(PointT) == MULLS_POINT_BYTES, "the scan preparation expects 48-byte pcl::PointXYZINormal records");
	mulls_ctx *ctx = thread_context();
	uint32_t n_out = 0;
	const int rc = mulls_scan_prepare(ctx, cloud_in_out->points.data(), static_cast<uint32_t>(cloud_in_out->points.size()), MULLS_POINT_BYTES, &P, &n_out, nullptr);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_scan_prepare failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	cloud_in_out->points.resize(n_out);
	return n_out;
}
// cfilter.hpp:250-291
template <typename PointT>
inline bool vertical_intrinsic_calibration(typename pcl::PointCloud<PointT>::Ptr &cloud_in_out, double var_vertical_ang_d = 0.0, bool inverse_z = false)
{
	if (var_vertical_ang_d == 0)
		return false;
	if (var_vertical_ang_d >= 180.0)
		inverse_z = true;
	mulls_scan_prep_params P;
	mulls_scan_prep_default_params(&P);
	P.calib_on = 1;
	P.vertical_ang_correction_deg = inverse_z ? 180.0 : var_vertical_ang_d; // (180: the library's spelling of "negate z")
	scan_prepare<PointT>(cloud_in_out, P);
	return !inverse_z;
}
// cfilter.hpp:412-467
template <typename PointT>
inline bool get_pts_timestamp_ratio_in_frame(typename pcl::PointCloud<PointT>::Ptr &cloud_in_out, bool timestamp_availiable = true,
											 double scan_begin_ang_anticlock_x_positive_deg = 180.0, float scan_duration_ms = 100)
{
	mulls_scan_prep_params P;
	mulls_scan_prep_default_params(&P);
	P.timestamp_mode = timestamp_availiable ? 1 : 2;
	P.scan_begin_ang_deg = scan_begin_ang_anticlock_x_positive_deg;
	P.scan_duration_ms = scan_duration_ms;
	scan_prepare<PointT>(cloud_in_out, P);
	return true;
}
// cfilter.hpp:730-747 and :713-728
template <typename PointT>
inline bool random_downsample(typename pcl::PointCloud<PointT>::Ptr &cloud_in_out, int downsample_ratio)
{
	if (downsample_ratio <= 1)
		return 0;
	mulls_scan_prep_params P;
	mulls_scan_prep_default_params(&P);
	P.downsample_ratio = downsample_ratio;
	scan_prepare<PointT>(cloud_in_out, P);
	return 1;
}
template <typename PointT>
inline bool random_downsample(const typename pcl::PointCloud<PointT>::Ptr &cloud_in, typename pcl::PointCloud<PointT>::Ptr &cloud_out, int downsample_ratio)
{
	if (downsample_ratio <= 1)
		return 0;
	cloud_out->points = cloud_in->points; // (:718-723 clears cloud_out and pushes the kept points)
	return random_downsample<PointT>(cloud_out, downsample_ratio);
}
// cfilter.hpp:806-831
template <typename PointT>
inline bool dist_filter(typename pcl::PointCloud<PointT>::Ptr &cloud_in_out, double xy_dist_min, double xy_dist_max)
{
	mulls_scan_prep_params P;
	mulls_scan_prep_default_params(&P);
	P.dist_filter_on = 1;
	P.min_dist = xy_dist_min;
	P.max_dist = xy_dist_max;
	scan_prepare<PointT>(cloud_in_out, P);
	return 1;
}
// One frame of the merged map mulls_slam exports (test/mulls_slam.cpp:963-990) into a mapper (mulls_mapper_create): pc_raw as read from the file, its
// pose_optimized, and the pose of the frame before it — NULL for the first frame, which upstream does not compensate (:977 `i > 0`).  prep carries the
// flags of :966-974; compensated when prep.timestamp_mode > 0 (FLAGS_motion_compensation_method > 0) and there is a frame before.
template <typename PointT>
inline uint32_t merged_map_add(mulls_mapper *mapper, const typename pcl::PointCloud<PointT>::Ptr &pc_raw, const Eigen::Matrix4d &pose_optimized,
							   const Eigen::Matrix4d *pose_of_frame_before, const mulls_scan_prep_params &prep)
{
	static_assert(sizeof(PointT) == MULLS_POINT_BYTES, "the merged map expects 48-byte pcl::PointXYZINormal records");
	mulls_ctx *ctx = thread_context();
	mulls_mapper_frame F;
	std::memset(&F, 0, sizeof(F));
	F.scan = borrow(pc_raw);
	std::memcpy(F.pose, pose_optimized.data(), sizeof(F.pose));
	if (prep.timestamp_mode > 0 && pose_of_frame_before)
	{
		const Eigen::Matrix4d adjacent_tran = pose_optimized.inverse() * *pose_of_frame_before; // :979
		std::memcpy(F.adjacent_tran, adjacent_tran.data(), sizeof(F.adjacent_tran));
		F.compensate = 1;
	}
	uint32_t n_out = 0;
	const int rc = mulls_mapper_add(ctx, mapper, &F, 1, &prep, &n_out, nullptr);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_mapper_add failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	return n_out;
}

// The pictures of a cloud: CloudUtility<PointT>::get_cloud_cpt (include/common/utility.hpp:800-814), CFilter<PointT>::generate_2d_map (cfilter.hpp:2751-2790)
// and CFilter<PointT>::pointcloud_to_rangeimage (:2714-2746) with upstream's parameter lists, each one device call (mulls_cloud_centre, mulls_map_image_2d,
// mulls_range_image; include/mulls_hip.h has the definition and says what of it is upstream's, what restates OpenCV from memory and what is the library's).
// The pictures are filled into a std::vector<uint8_t>, row by row, plus width and height, so that the export needs no OpenCV (mulls_io_write_pgm writes
// them); the cv::Mat overloads with upstream's verbatim signatures exist under OPENCV_ON only.  image_2d_of_cloud takes a mulls_cloud, so that the merged
// map is pictured where it lies: lo::hip::generate_2d_map(mulls_mapper's cloud, ...) moves nothing but the picture.
template <typename PointT>
inline void get_cloud_cpt(const typename pcl::PointCloud<PointT>::Ptr &cloud, centerpoint_t &cp)
{
	mulls_ctx *ctx = thread_context();
	const mulls_cloud c = borrow(cloud);
	double centre[3];
	const int rc = mulls_cloud_centre(ctx, &c, centre);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_cloud_centre failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	cp.x = centre[0], cp.y = centre[1], cp.z = centre[2];
}
inline void image_2d_of_cloud(const mulls_cloud &cloud, std::vector<uint8_t> &image, double m2pix, int map_width, int map_height, int min_points_in_pix,
							  int max_points_in_pix, double min_height, double max_height, bool shift_or_not)
{
	mulls_ctx *ctx = thread_context();
	mulls_image2d_params P;
	mulls_image2d_default_params(&P);
	P.m2pix = m2pix, P.map_width = map_width, P.map_height = map_height;
	P.min_points_in_pix = min_points_in_pix, P.max_points_in_pix = max_points_in_pix;
	P.min_height = min_height, P.max_height = max_height, P.shift = shift_or_not;
	image.assign(map_width > 0 && map_height > 0 ? (size_t)map_width * (size_t)map_height : 0, 0);
	const int rc = mulls_map_image_2d(ctx, &cloud, &P, image.data(), nullptr, nullptr);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_map_image_2d failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
}
template <typename PointT>
inline void generate_2d_map(const typename pcl::PointCloud<PointT>::Ptr &cloud, std::vector<uint8_t> &image, double m2pix, int map_width, int map_height,
							int min_points_in_pix, int max_points_in_pix, double min_height, double max_height, bool shift_or_not = false)
{
	image_2d_of_cloud(borrow(cloud), image, m2pix, map_width, map_height, min_points_in_pix, max_points_in_pix, min_height, max_height, shift_or_not);
}
// the HDL-64 constants are upstream's own (:2717-2721): width and height come back as 900 and 64
template <typename PointT>
inline bool pointcloud_to_rangeimage(typename pcl::PointCloud<PointT>::Ptr &point_cloud, std::vector<uint8_t> &range_image, int &width, int &height)
{
	mulls_ctx *ctx = thread_context();
	mulls_range_image_params P;
	mulls_range_image_default_params(&P);
	const mulls_cloud c = borrow(point_cloud);
	range_image.assign((size_t)P.width * (size_t)P.height, 0);
	const int rc = mulls_range_image(ctx, &c, &P, range_image.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_range_image failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	width = P.width, height = P.height;
	return true;
}
#if OPENCV_ON
template <typename PointT>
inline cv::Mat generate_2d_map(const typename pcl::PointCloud<PointT>::Ptr &cloud, double m2pix, int map_width, int map_height, int min_points_in_pix,
							   int max_points_in_pix, double min_height, double max_height, bool shift_or_not = false)
{
	std::vector<uint8_t> image;
	generate_2d_map<PointT>(cloud, image, m2pix, map_width, map_height, min_points_in_pix, max_points_in_pix, min_height, max_height, shift_or_not);
	return cv::Mat(map_height, map_width, CV_8UC1, image.data()).clone();
}
template <typename PointT>
inline bool pointcloud_to_rangeimage(typename pcl::PointCloud<PointT>::Ptr &point_cloud, cv::Mat &range_image)
{
	std::vector<uint8_t> image;
	int width = 0, height = 0;
	pointcloud_to_rangeimage<PointT>(point_cloud, image, width, height);
	range_image = cv::Mat(height, width, CV_8UC1, image.data()).clone();
	return true;
}
#endif

// the pieces lo::hip::extract_semantic_pts and lo::hip::extract_semantic_pts_batch share
namespace detail
{
struct ExtractSetup
{
	mulls_extract_params X;
	bool scanner_stage, voxels;
};
// extract_semantic_pts' arguments as mulls_extract_params (two seeds of the feature stage's sequence are taken)
inline ExtractSetup extract_setup(float vf_downsample_resolution, float gf_grid_resolution, float gf_max_grid_height_diff,
								 float gf_neighbor_height_diff, float gf_max_ground_height, int &gf_down_rate_ground, int &gf_downsample_rate_nonground,
								 float pca_neighbor_radius, int pca_neighbor_k, float edge_thre, float planar_thre, float curvature_thre, float edge_thre_down,
								 float planar_thre_down, bool use_distance_adaptive_pca, int distance_inverse_sampling_method,
								 float standard_distance, int estimate_ground_normal_method, float normal_estimation_radius,
								 bool use_adpative_parameters, bool apply_scanner_filter, bool extract_curb_or_not,
								 int extract_vertex_points_method, int gf_grid_pt_num_thre, int gf_reliable_neighbor_grid_thre,
								 int gf_down_down_rate_ground, int pca_neighbor_k_min, int pca_down_rate, float intensity_thre,
								 float linear_vertical_sin_high_thre, float linear_vertical_sin_low_thre, float planar_vertical_sin_high_thre,
								 float planar_vertical_sin_low_thre, bool sharpen_with_nms_on, bool fixed_num_downsampling,
								 int ground_down_fixed_num, int pillar_down_fixed_num, int facade_down_fixed_num, int beam_down_fixed_num,
								 int roof_down_fixed_num, int unground_down_fixed_num, float beam_height_max, float roof_height_min,
								 float approx_scanner_height, float underground_thre, float feature_pts_ratio_guess, bool semantic_assisted,
								 bool apply_roi_filtering, float roi_min_y, float roi_max_y)
{
	(void)extract_curb_or_not, (void)apply_roi_filtering, (void)roi_min_y, (void)roi_max_y, (void)use_adpative_parameters;
	const bool scanner_stage = apply_scanner_filter && !semantic_assisted; // upstream: `if (semantic_assisted) ... else if (apply_scanner_filter) scanner_filter(...)`
	ExtractSetup S;
	mulls_extract_params &X = S.X;
	mulls_extract_default_params(&X);
	mulls_ground_params &G = X.ground;
	G.min_grid_pt_num = gf_grid_pt_num_thre;
	G.grid_resolution = gf_grid_resolution;
	G.max_height_difference = gf_max_grid_height_diff;
	G.neighbor_height_diff = gf_neighbor_height_diff;
	G.max_ground_height = gf_max_ground_height;
	G.ground_random_down_rate = gf_down_rate_ground;
	G.ground_random_down_down_rate = gf_down_down_rate_ground;
	G.nonground_random_down_rate = gf_downsample_rate_nonground;
	G.reliable_neighbor_grid_num_thre = gf_reliable_neighbor_grid_thre;
	G.estimate_ground_normal_method = estimate_ground_normal_method;
	G.normal_estimation_radius = normal_estimation_radius;
	G.distance_weight_downsampling_method = distance_inverse_sampling_method;
	G.standard_distance = standard_distance;
	G.fixed_num_downsampling = fixed_num_downsampling;
	G.down_ground_fixed_num = ground_down_fixed_num;
	G.intensity_thre = intensity_thre;
	G.apply_grid_wise_outlier_filter = apply_scanner_filter; // :2361
	G.outlier_std_scale = 3.0f;
	G.rng_seed = feature_rng_seed()++;
	mulls_classify_params &K = X.classify;
	K.neighbor_searching_radius = pca_neighbor_radius;
	K.neighbor_k = pca_neighbor_k;
	K.neigh_k_min = pca_neighbor_k_min;
	K.pca_down_rate = pca_down_rate;
	K.edge_thre = edge_thre, K.planar_thre = planar_thre, K.edge_thre_down = edge_thre_down, K.planar_thre_down = planar_thre_down;
	K.extract_vertex_points_method = extract_vertex_points_method;
	K.curvature_thre = curvature_thre;
	K.vertex_curvature_non_max_radius = 1.5 * pca_neighbor_radius; // :2365
	K.linear_vertical_sin_high_thre = linear_vertical_sin_high_thre, K.linear_vertical_sin_low_thre = linear_vertical_sin_low_thre;
	K.planar_vertical_sin_high_thre = planar_vertical_sin_high_thre, K.planar_vertical_sin_low_thre = planar_vertical_sin_low_thre;
	K.fixed_num_downsampling = fixed_num_downsampling;
	K.sharpen_with_nms = sharpen_with_nms_on;
	K.use_distance_adaptive_pca = use_distance_adaptive_pca;
	K.pillar_down_fixed_num = pillar_down_fixed_num, K.facade_down_fixed_num = facade_down_fixed_num, K.beam_down_fixed_num = beam_down_fixed_num;
	K.roof_down_fixed_num = roof_down_fixed_num, K.unground_down_fixed_num = unground_down_fixed_num;
	K.beam_height_max = beam_height_max, K.roof_height_min = roof_height_min, K.feature_pts_ratio_guess = feature_pts_ratio_guess;
	K.rng_seed = feature_rng_seed()++;
	X.apply_scanner_filter = scanner_stage;
	X.self_ring_radius = 1.75f; // :2340-2343
	X.ghost_radius = 20.0f;
	X.z_min = -approx_scanner_height - 4.0;
	X.z_min_min = -approx_scanner_height + underground_thre;
	X.vf_downsample_resolution = vf_downsample_resolution;
	S.scanner_stage = scanner_stage;
	S.voxels = !(vf_downsample_resolution < 0.001);
	return S;
}
// filter_with_dynamic_object_mask_pre(in_block->pc_raw), cfilter.hpp:2487-2504: the float comparisons as written there
template <typename PointT>
inline void extract_semantic_prefilter(cloudblock_t &blk)
{
	typename pcl::PointCloud<PointT>::Ptr kept(new pcl::PointCloud<PointT>());
	for (size_t i = 0; i < blk.pc_raw->points.size(); i++)
		if (blk.pc_raw->points[i].curvature < 250 && blk.pc_raw->points[i].curvature != 1)
			kept->points.push_back(blk.pc_raw->points[i]);
	kept->points.swap(blk.pc_raw->points);
}
// pc_sketch from pc_down: random_downsample(pc_down, pc_sketch, size / 1024 + 1) (:2351, :713-728)
inline void extract_sketch(cloudblock_t &b)
{
	const int ratio = (int)(b.pc_down->points.size() / 1024 + 1);
	if (ratio > 1)
	{
		b.pc_sketch->points.clear();
		for (size_t i = 0; i < b.pc_down->points.size(); i++)
			if ((int)i % ratio == 0)
				b.pc_sketch->points.push_back(b.pc_down->points[i]);
	}
}
// what extract_semantic_pts does on the host once the clouds are in the block: the feature count and the adaptive parameter update, with its exception
inline void extract_finish(cloudblock_t &b, bool use_adpative_parameters, int &gf_downsample_rate_nonground)
{
	b.down_feature_point_num = b.pc_ground_down->points.size() + b.pc_pillar_down->points.size() + b.pc_beam_down->points.size() + b.pc_facade_down->points.size() +
							   b.pc_roof_down->points.size() + b.pc_vertex->points.size(); // :2397-2398
	if (use_adpative_parameters)
	{
		// update_parameters_self_adaptive (:2416-2444): the one live rule lowers the non-ground down-sampling rate when few facade / pillar points came out
		const int non_ground_num_min_expected = 200;
		const int non_ground_feature_num = (int)b.pc_facade_down->points.size() + (int)b.pc_pillar_down->points.size();
		if (non_ground_feature_num < non_ground_num_min_expected)
		{
			if (non_ground_feature_num == 0)
				throw std::runtime_error("lo::hip::extract_semantic_pts: adaptive parameters with no facade / pillar point (upstream divides by zero here)");
			gf_downsample_rate_nonground = std::max(1, gf_downsample_rate_nonground - non_ground_num_min_expected / non_ground_feature_num);
		}
	}
}
} // namespace detail

// CFilter<PointT>::extract_semantic_pts (include/common/cfilter.hpp:2295-2413), verbatim signature: the whole chain in one device call
// (mulls_extract_features).  The binding is one early return at the top of the member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::extract_semantic_pts<PointT>(in_block, vf_downsample_resolution, gf_grid_resolution, ...);
//     #endif
// semantic_assisted (deprecated upstream, off in every shipped configuration; round 5): the pre-filter filter_with_dynamic_object_mask_pre (cfilter.hpp:2487-2504 —
// Semantic-KITTI labels in the curvature field: moving objects, labels >= 250, and outliers, label 1, leave pc_raw) runs here on the host, in place on pc_raw as
// upstream does, INSTEAD of the scanner filter (upstream's `else if`, :2331-2345); the post-filter filter_with_semantic_mask(in_block) is called with its default mask
// "000000" (:2396), with which it touches nothing.  apply_roi_filtering is dead code upstream ("#if 0") and ignored here too.  use_adpative_parameters runs upstream's update (:2416-2444) on the host; where upstream would divide by zero (no facade and
// no pillar point left) this throws instead.
// One side effect is not reproduced: upstream's ground filter writes (0,0,1) normals and data[3] heights into the points of pc_down (= pc_raw)
// it classifies; here pc_raw / pc_down / pc_sketch keep the scan's records (the clouds handed out carry those values).
template <typename PointT>
inline bool extract_semantic_pts(cloudblock_Ptr in_block, float vf_downsample_resolution, float gf_grid_resolution, float gf_max_grid_height_diff,
								 float gf_neighbor_height_diff, float gf_max_ground_height, int &gf_down_rate_ground, int &gf_downsample_rate_nonground,
								 float pca_neighbor_radius, int pca_neighbor_k, float edge_thre, float planar_thre, float curvature_thre, float edge_thre_down,
								 float planar_thre_down, bool use_distance_adaptive_pca = false, int distance_inverse_sampling_method = 0,
								 float standard_distance = 15.0, int estimate_ground_normal_method = 3, float normal_estimation_radius = 2.0,
								 bool use_adpative_parameters = false, bool apply_scanner_filter = false, bool extract_curb_or_not = false,
								 int extract_vertex_points_method = 2, int gf_grid_pt_num_thre = 8, int gf_reliable_neighbor_grid_thre = 0,
								 int gf_down_down_rate_ground = 2, int pca_neighbor_k_min = 8, int pca_down_rate = 1, float intensity_thre = FLT_MAX,
								 float linear_vertical_sin_high_thre = 0.94, float linear_vertical_sin_low_thre = 0.17, float planar_vertical_sin_high_thre = 0.98,
								 float planar_vertical_sin_low_thre = 0.34, bool sharpen_with_nms_on = true, bool fixed_num_downsampling = false,
								 int ground_down_fixed_num = 500, int pillar_down_fixed_num = 200, int facade_down_fixed_num = 800, int beam_down_fixed_num = 200,
								 int roof_down_fixed_num = 200, int unground_down_fixed_num = 20000, float beam_height_max = FLT_MAX, float roof_height_min = 0.0,
								 float approx_scanner_height = 2.0, float underground_thre = -7.0, float feature_pts_ratio_guess = 0.3, bool semantic_assisted = false,
								 bool apply_roi_filtering = false, float roi_min_y = 0.0, float roi_max_y = 0.0)
{
	if (semantic_assisted)
		detail::extract_semantic_prefilter<PointT>(*in_block);
	const detail::ExtractSetup S = detail::extract_setup(vf_downsample_resolution, gf_grid_resolution, gf_max_grid_height_diff, gf_neighbor_height_diff, gf_max_ground_height, gf_down_rate_ground, gf_downsample_rate_nonground, pca_neighbor_radius, pca_neighbor_k, edge_thre, planar_thre, curvature_thre, edge_thre_down, planar_thre_down, use_distance_adaptive_pca, distance_inverse_sampling_method, standard_distance, estimate_ground_normal_method, normal_estimation_radius, use_adpative_parameters, apply_scanner_filter, extract_curb_or_not, extract_vertex_points_method, gf_grid_pt_num_thre, gf_reliable_neighbor_grid_thre, gf_down_down_rate_ground, pca_neighbor_k_min, pca_down_rate, intensity_thre, linear_vertical_sin_high_thre, linear_vertical_sin_low_thre, planar_vertical_sin_high_thre, planar_vertical_sin_low_thre, sharpen_with_nms_on, fixed_num_downsampling, ground_down_fixed_num, pillar_down_fixed_num, facade_down_fixed_num, beam_down_fixed_num, roof_down_fixed_num, unground_down_fixed_num, beam_height_max, roof_height_min, approx_scanner_height, underground_thre, feature_pts_ratio_guess, semantic_assisted, apply_roi_filtering, roi_min_y, roi_max_y);
	const mulls_extract_params &X = S.X;
	const bool scanner_stage = S.scanner_stage, voxels = S.voxels;
	mulls_ctx *ctx = thread_context();

	cloudblock_t &b = *in_block;
	const mulls_cloud in = borrow(b.pc_raw);
	std::vector<unsigned char> raw[MULLS_EX_COUNT];
	void *out[MULLS_EX_COUNT];
	uint32_t cap[MULLS_EX_COUNT], n_out[MULLS_EX_COUNT];
	for (int k = 0; k < MULLS_EX_COUNT; k++)
	{
		const bool want = k == MULLS_EX_RAW ? scanner_stage : k == MULLS_EX_DOWN ? voxels : true; // without the scanner filter pc_raw stays what it is, without voxels pc_down is pc_raw
		raw[k].resize(want ? (size_t)in.n * MULLS_POINT_BYTES : 0);
		out[k] = want ? raw[k].data() : nullptr;
		cap[k] = want ? in.n : 0;
	}
	const int rc = mulls_extract_features(ctx, in.pts, in.n, in.stride, &X, out, cap, n_out);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_extract_features failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	if (scanner_stage)
		take_cloud<PointT>(b.pc_raw, raw[MULLS_EX_RAW], n_out[MULLS_EX_RAW], false); // scanner_filter works on pc_raw itself
	if (voxels)
		take_cloud<PointT>(b.pc_down, raw[MULLS_EX_DOWN], n_out[MULLS_EX_DOWN], true); // `cloud_out->push_back(...)` (:147)
	else
		b.pc_down = b.pc_raw; // voxel_downsample below 0.001 m: `cloud_out = cloud_in` (:92)
	detail::extract_sketch(b);
	take_cloud<PointT>(b.pc_ground, raw[MULLS_EX_GROUND], n_out[MULLS_EX_GROUND], true);
	take_cloud<PointT>(b.pc_ground_down, raw[MULLS_EX_GROUND_DOWN], n_out[MULLS_EX_GROUND_DOWN], true);
	take_cloud<PointT>(b.pc_unground, raw[MULLS_EX_UNGROUND], n_out[MULLS_EX_UNGROUND], false); // the filter appends to an empty cloud, the classification works on it in place
	typename pcl::PointCloud<PointT>::Ptr *dst[9] = {&b.pc_pillar, &b.pc_beam, &b.pc_facade, &b.pc_roof, &b.pc_pillar_down, &b.pc_beam_down, &b.pc_facade_down, &b.pc_roof_down, &b.pc_vertex};
	for (int k = 0; k < 9; k++)
		take_cloud<PointT>(*dst[k], raw[MULLS_EX_PILLAR + k], n_out[MULLS_EX_PILLAR + k], true);
	detail::extract_finish(b, use_adpative_parameters, gf_downsample_rate_nonground);
	return true;
}

// extract_semantic_pts for many blocks in one device call (mulls_extract_features_batch): every block's pc_raw is one scan, all scans take the same arguments
// (one pair of seeds: every scan's fixed-number selections are those of a single call with these seeds), and every block leaves as extract_semantic_pts leaves
// it — the clouds come back from the device-resident feature blocks, one download per cloud, and the host-side remainder is the single call's
// (detail::extract_sketch, detail::extract_finish: the adaptive update lowers gf_downsample_rate_nonground once per block, in order, as a loop of single calls
// would).  A scan the library refuses throws, naming it, after the others' blocks have been filled.  With the scanner filter on, pc_raw is filtered here on the
// host (cfilter.hpp:914-929, the comparisons as written there): a feature block does not keep pc_raw, and the size is checked against the device's.
template <typename PointT>
inline bool extract_semantic_pts_batch(std::vector<cloudblock_Ptr> &in_blocks, float vf_downsample_resolution, float gf_grid_resolution, float gf_max_grid_height_diff,
								 float gf_neighbor_height_diff, float gf_max_ground_height, int &gf_down_rate_ground, int &gf_downsample_rate_nonground,
								 float pca_neighbor_radius, int pca_neighbor_k, float edge_thre, float planar_thre, float curvature_thre, float edge_thre_down,
								 float planar_thre_down, bool use_distance_adaptive_pca = false, int distance_inverse_sampling_method = 0,
								 float standard_distance = 15.0, int estimate_ground_normal_method = 3, float normal_estimation_radius = 2.0,
								 bool use_adpative_parameters = false, bool apply_scanner_filter = false, bool extract_curb_or_not = false,
								 int extract_vertex_points_method = 2, int gf_grid_pt_num_thre = 8, int gf_reliable_neighbor_grid_thre = 0,
								 int gf_down_down_rate_ground = 2, int pca_neighbor_k_min = 8, int pca_down_rate = 1, float intensity_thre = FLT_MAX,
								 float linear_vertical_sin_high_thre = 0.94, float linear_vertical_sin_low_thre = 0.17, float planar_vertical_sin_high_thre = 0.98,
								 float planar_vertical_sin_low_thre = 0.34, bool sharpen_with_nms_on = true, bool fixed_num_downsampling = false,
								 int ground_down_fixed_num = 500, int pillar_down_fixed_num = 200, int facade_down_fixed_num = 800, int beam_down_fixed_num = 200,
								 int roof_down_fixed_num = 200, int unground_down_fixed_num = 20000, float beam_height_max = FLT_MAX, float roof_height_min = 0.0,
								 float approx_scanner_height = 2.0, float underground_thre = -7.0, float feature_pts_ratio_guess = 0.3, bool semantic_assisted = false,
								 bool apply_roi_filtering = false, float roi_min_y = 0.0, float roi_max_y = 0.0)
{
	static_assert(sizeof(PointT) == MULLS_POINT_BYTES, "the feature stage expects 48-byte pcl::PointXYZINormal records");
	if (semantic_assisted)
		for (cloudblock_Ptr &blk : in_blocks)
			detail::extract_semantic_prefilter<PointT>(*blk);
	const detail::ExtractSetup S = detail::extract_setup(vf_downsample_resolution, gf_grid_resolution, gf_max_grid_height_diff, gf_neighbor_height_diff, gf_max_ground_height, gf_down_rate_ground, gf_downsample_rate_nonground, pca_neighbor_radius, pca_neighbor_k, edge_thre, planar_thre, curvature_thre, edge_thre_down, planar_thre_down, use_distance_adaptive_pca, distance_inverse_sampling_method, standard_distance, estimate_ground_normal_method, normal_estimation_radius, use_adpative_parameters, apply_scanner_filter, extract_curb_or_not, extract_vertex_points_method, gf_grid_pt_num_thre, gf_reliable_neighbor_grid_thre, gf_down_down_rate_ground, pca_neighbor_k_min, pca_down_rate, intensity_thre, linear_vertical_sin_high_thre, linear_vertical_sin_low_thre, planar_vertical_sin_high_thre, planar_vertical_sin_low_thre, sharpen_with_nms_on, fixed_num_downsampling, ground_down_fixed_num, pillar_down_fixed_num, facade_down_fixed_num, beam_down_fixed_num, roof_down_fixed_num, unground_down_fixed_num, beam_height_max, roof_height_min, approx_scanner_height, underground_thre, feature_pts_ratio_guess, semantic_assisted, apply_roi_filtering, roi_min_y, roi_max_y);
	mulls_ctx *ctx = thread_context();
	const uint32_t count = static_cast<uint32_t>(in_blocks.size());
	std::vector<mulls_cloud> scans(count);
	std::vector<mulls_block *> dev(count, nullptr);
	std::vector<mulls_extract_batch_result> results(count);
	struct Release
	{
		mulls_ctx *ctx;
		std::vector<mulls_block *> &dev;
		~Release()
		{
			for (mulls_block *d : dev)
				mulls_block_destroy(ctx, d);
		}
	} release{ctx, dev};
	for (uint32_t k = 0; k < count; k++)
	{
		scans[k] = borrow(in_blocks[k]->pc_raw);
		if (mulls_block_create(ctx, &dev[k]) != MULLS_OK)
			throw std::runtime_error(std::string("mulls_block_create failed: ") + mulls_last_error(ctx));
	}
	const int rc = mulls_extract_features_batch(ctx, scans.data(), count, &S.X, dev.data(), 0, results.data(), nullptr);
	const std::string why = rc != MULLS_OK ? mulls_last_error(ctx) : "";
	std::vector<unsigned char> raw;
	for (uint32_t k = 0; k < count; k++)
	{
		if (results[k].status != MULLS_OK)
			continue;
		cloudblock_t &b = *in_blocks[k];
		const uint32_t *n_out = results[k].n_out;
		if (S.scanner_stage)
		{
			typename pcl::PointCloud<PointT>::Ptr kept(new pcl::PointCloud<PointT>());
			const float self_ring_radius = S.X.self_ring_radius, ghost_radius = S.X.ghost_radius, z_min = S.X.z_min, z_min_min = S.X.z_min_min;
			for (size_t i = 0; i < b.pc_raw->points.size(); i++)
			{
				const PointT &pt = b.pc_raw->points[i];
				const float dis_square = pt.x * pt.x + pt.y * pt.y;
				if (dis_square > self_ring_radius * self_ring_radius && pt.z > z_min_min && (dis_square > ghost_radius * ghost_radius || pt.z > z_min))
					kept->points.push_back(pt);
			}
			if (kept->points.size() != n_out[MULLS_EX_RAW])
				throw std::runtime_error("lo::hip::extract_semantic_pts_batch: the host's scanner filter kept " + std::to_string(kept->points.size()) + " points of block " +
										 std::to_string(k) + ", the device " + std::to_string(n_out[MULLS_EX_RAW]));
			kept->points.swap(b.pc_raw->points);
		}
		typename pcl::PointCloud<PointT>::Ptr *dst[MULLS_EX_COUNT] = {nullptr, &b.pc_ground, &b.pc_ground_down, &b.pc_unground, &b.pc_pillar, &b.pc_beam, &b.pc_facade, &b.pc_roof,
																	  &b.pc_pillar_down, &b.pc_beam_down, &b.pc_facade_down, &b.pc_roof_down, &b.pc_vertex, nullptr};
		if (S.voxels)
		{
			// (the single-scan path inside the call does not keep pc_down either: voxel_downsample once more, the same device code on the same records)
			b.pc_down->points.clear();
			voxel_downsample<PointT>(b.pc_raw, b.pc_down, S.X.vf_downsample_resolution);
		}
		else
			b.pc_down = b.pc_raw; // voxel_downsample below 0.001 m: `cloud_out = cloud_in` (:92)
		detail::extract_sketch(b);
		for (int c = 0; c < MULLS_EX_COUNT; c++)
		{
			if (!dst[c])
				continue;
			uint32_t got = 0;
			raw.resize((size_t)n_out[c] * MULLS_POINT_BYTES);
			const int rd = mulls_block_download(ctx, dev[k], c, raw.data(), n_out[c], &got);
			if (rd != MULLS_OK || got != n_out[c])
				throw std::runtime_error(std::string("mulls_block_download failed (") + std::to_string(rd) + "): " + mulls_last_error(ctx));
			take_cloud<PointT>(*dst[c], raw, got, c != MULLS_EX_UNGROUND); // (the filter appends to an empty pc_unground, the classification works on it in place)
		}
		detail::extract_finish(b, use_adpative_parameters, gf_downsample_rate_nonground);
	}
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_extract_features_batch failed (") + std::to_string(rc) + "): " + why);
	return true;
}

// CRegistration<PointT>::omp_ndt (include/common/cregistration.hpp:945-1021), verbatim signature and defaults: the NDT baseline that
// test/mulls_slam.cpp:633-647 and :669-684 select with --baseline_reg_method=omp_ndt, in one device call (mulls_ndt).  The binding is one early return
// at the top of the member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::omp_ndt<PointT>(registration_cons, ndt_resolution, use_direct_search, initial_guess, apply_intersection_filter, fitness_score_thre);
//     #endif
// block1->pc_down is the target, block2->pc_down the source; Trans1_2 receives the pose, the return value is upstream's process code (1 or -3).
// use_direct_search = false (the kd-tree over leaf centroids) is not built: the call throws with MULLS_E_UNSUPPORTED's message.
namespace detail
{
template <typename Constraint>
inline void ndt_fill(const Constraint &con, const Eigen::Matrix4d &initial_guess, mulls_ndt_problem &P)
{
	P.tgt = borrow(con.block1->pc_down), P.src = borrow(con.block2->pc_down);
	const bounds_t &a = con.block1->local_bound, &b = con.block2->local_bound;
	const double tb[6] = {a.min_x, a.min_y, a.min_z, a.max_x, a.max_y, a.max_z}, sb[6] = {b.min_x, b.min_y, b.min_z, b.max_x, b.max_y, b.max_z};
	for (int k = 0; k < 6; k++)
		P.tgt_bound[k] = tb[k], P.src_bound[k] = sb[k];
	for (int k = 0; k < 16; k++)
		P.init_guess[k] = initial_guess.data()[k]; // (column-major)
}
} // namespace detail
inline mulls_ndt_params ndt_params(float ndt_resolution = 1.0, bool use_direct_search = true, bool apply_intersection_filter = true, float fitness_score_thre = 10.0)
{
	mulls_ndt_params P;
	mulls_ndt_default_params(&P);
	P.resolution = ndt_resolution, P.search_method = use_direct_search ? MULLS_NDT_DIRECT7 : MULLS_NDT_KDTREE;
	P.apply_intersection_filter = apply_intersection_filter ? 1 : 0, P.fitness_score_thre = fitness_score_thre;
	return P;
}
template <typename PointT>
inline int omp_ndt(constraint_t &registration_cons, float ndt_resolution = 1.0, bool use_direct_search = true,
				   Eigen::Matrix4d initial_guess = Eigen::Matrix4d::Identity(), bool apply_intersection_filter = true, float fitness_score_thre = 10.0)
{
	mulls_ctx *ctx = thread_context();
	mulls_ndt_problem P;
	detail::ndt_fill(registration_cons, initial_guess, P);
	const mulls_ndt_params prm = ndt_params(ndt_resolution, use_direct_search, apply_intersection_filter, fitness_score_thre);
	mulls_ndt_result R;
	const int rc = mulls_ndt(ctx, &P, &prm, &R);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_ndt failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (int k = 0; k < 16; k++)
		registration_cons.Trans1_2.data()[k] = R.T[k];
	return R.code;
}
// many constraints in one call (mulls_ndt_batch): every constraint with the bits of its omp_ndt call; initial_guesses is empty (identity for all) or
// one matrix per constraint.  Returns the process codes.
template <typename PointT>
inline std::vector<int> omp_ndt_batch(std::vector<constraint_t> &registration_cons, float ndt_resolution = 1.0, bool use_direct_search = true,
									  const std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>> &initial_guesses = {},
									  bool apply_intersection_filter = true, float fitness_score_thre = 10.0)
{
	const size_t B = registration_cons.size();
	if (!initial_guesses.empty() && initial_guesses.size() != B)
		throw std::runtime_error("lo::hip::omp_ndt_batch: one initial guess per constraint, or none");
	mulls_ctx *ctx = thread_context();
	std::vector<mulls_ndt_problem> problems(B);
	for (size_t k = 0; k < B; k++)
		detail::ndt_fill(registration_cons[k], initial_guesses.empty() ? Eigen::Matrix4d(Eigen::Matrix4d::Identity()) : initial_guesses[k], problems[k]);
	const mulls_ndt_params prm = ndt_params(ndt_resolution, use_direct_search, apply_intersection_filter, fitness_score_thre);
	std::vector<mulls_ndt_result> R(B);
	const int rc = mulls_ndt_batch(ctx, problems.data(), (uint32_t)B, &prm, R.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_ndt_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	std::vector<int> codes(B);
	for (size_t k = 0; k < B; k++)
	{
		for (int e = 0; e < 16; e++)
			registration_cons[k].Trans1_2.data()[e] = R[k].T[e];
		codes[k] = R[k].code;
	}
	return codes;
}

// CRegistration<PointT>::omp_gicp (include/common/cregistration.hpp:1024-1098), verbatim signature and defaults: the GICP baseline that
// test/mulls_slam.cpp:637-639 and :674-676 select with --baseline_reg_method=gicp, in one device call (mulls_gicp).  The binding is one early return
// at the top of the member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::omp_gicp<PointT>(registration_cons, max_iter_num, dis_thre_unit, using_voxel_gicp, voxel_size, initial_guess, apply_intersection_filter, fitness_score_thre);
//     #endif
// block1->pc_down is the target, block2->pc_down the source; Trans1_2 receives the pose, the return value is upstream's process code (1 or -3).
// max_iter_num and dis_thre_unit are accepted and not read, as upstream does not read them with using_voxel_gicp = true.  using_voxel_gicp = false
// (PCL's BFGS GICP) is not built: the call throws with MULLS_E_UNSUPPORTED's message.
inline mulls_gicp_params gicp_params(bool using_voxel_gicp = true, float voxel_size = 1.0, bool apply_intersection_filter = false, float fitness_score_thre = 10.0)
{
	mulls_gicp_params P;
	mulls_gicp_default_params(&P);
	P.voxel_resolution = voxel_size, P.using_voxel_gicp = using_voxel_gicp ? 1 : 0;
	P.apply_intersection_filter = apply_intersection_filter ? 1 : 0, P.fitness_score_thre = fitness_score_thre;
	return P;
}
template <typename PointT>
inline int omp_gicp(constraint_t &registration_cons, int max_iter_num = 20, float dis_thre_unit = 1.5, bool using_voxel_gicp = true, float voxel_size = 1.0,
					Eigen::Matrix4d initial_guess = Eigen::Matrix4d::Identity(), bool apply_intersection_filter = false, float fitness_score_thre = 10.0)
{
	(void)max_iter_num, (void)dis_thre_unit;
	mulls_ctx *ctx = thread_context();
	mulls_gicp_problem P;
	detail::ndt_fill(registration_cons, initial_guess, P);
	const mulls_gicp_params prm = gicp_params(using_voxel_gicp, voxel_size, apply_intersection_filter, fitness_score_thre);
	mulls_gicp_result R;
	const int rc = mulls_gicp(ctx, &P, &prm, &R);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_gicp failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (int k = 0; k < 16; k++)
		registration_cons.Trans1_2.data()[k] = R.T[k];
	return R.code;
}
// many constraints in one call (mulls_gicp_batch): every constraint with the bits of its omp_gicp call; initial_guesses is empty (identity for all) or
// one matrix per constraint.  Returns the process codes.
template <typename PointT>
inline std::vector<int> omp_gicp_batch(std::vector<constraint_t> &registration_cons, float voxel_size = 1.0,
									   const std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>> &initial_guesses = {},
									   bool apply_intersection_filter = false, float fitness_score_thre = 10.0, bool using_voxel_gicp = true)
{
	const size_t B = registration_cons.size();
	if (!initial_guesses.empty() && initial_guesses.size() != B)
		throw std::runtime_error("lo::hip::omp_gicp_batch: one initial guess per constraint, or none");
	mulls_ctx *ctx = thread_context();
	std::vector<mulls_gicp_problem> problems(B);
	for (size_t k = 0; k < B; k++)
		detail::ndt_fill(registration_cons[k], initial_guesses.empty() ? Eigen::Matrix4d(Eigen::Matrix4d::Identity()) : initial_guesses[k], problems[k]);
	const mulls_gicp_params prm = gicp_params(using_voxel_gicp, voxel_size, apply_intersection_filter, fitness_score_thre);
	std::vector<mulls_gicp_result> R(B);
	const int rc = mulls_gicp_batch(ctx, problems.data(), (uint32_t)B, &prm, R.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_gicp_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	std::vector<int> codes(B);
	for (size_t k = 0; k < B; k++)
	{
		for (int e = 0; e < 16; e++)
			registration_cons[k].Trans1_2.data()[e] = R[k].T[e];
		codes[k] = R[k].code;
	}
	return codes;
}

// CRegistration<PointT>::pcl_icp (include/common/cregistration.hpp:882-942), verbatim signature and defaults: the classical ICP baseline that
// test/mulls_slam.cpp:195 names "pclicp", in one device call (mulls_pcl_icp).  The binding is one early return at the top of the member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::pcl_icp<PointT>(registration_cons, max_iter_num, dis_thre_unit, metrics, ce, te, use_reciprocal_correspondence,
//                                         use_trimmed_rejector, neighbor_radius, initial_guess, apply_intersection_filter, fitness_score_thre);
//     #endif
// block1->pc_down is the target, block2->pc_down the source; Trans1_2 receives the pose, the return value is upstream's process code (1 or -3).
// metrics, ce and te are upstream's DistMetricType, CorresEstimationType and TransformEstimationType (cregistration.hpp:59-75; the library's enums
// have their values), taken as template parameters because this header does not define them.  Plane2Plane, LM, NS and the trimmed rejector are not
// built: the call throws with MULLS_E_UNSUPPORTED's message.  With an identity guess upstream registers an empty source (include/mulls_hip.h);
// this call registers block2->pc_down.
inline mulls_pcl_icp_params pcl_icp_params(int max_iter_num, float dis_thre_unit, int metrics, int ce, int te, bool use_reciprocal_correspondence,
										   bool use_trimmed_rejector, float neighbor_radius = 2.0, bool apply_intersection_filter = true,
										   float fitness_score_thre = 10.0)
{
	mulls_pcl_icp_params P;
	mulls_pcl_icp_default_params(&P);
	P.max_iter_num = max_iter_num, P.dis_thre_unit = dis_thre_unit, P.metrics = metrics, P.ce = ce, P.te = te;
	P.use_reciprocal_correspondence = use_reciprocal_correspondence ? 1 : 0, P.use_trimmed_rejector = use_trimmed_rejector ? 1 : 0;
	P.neighbor_radius = neighbor_radius, P.apply_intersection_filter = apply_intersection_filter ? 1 : 0, P.fitness_score_thre = fitness_score_thre;
	return P;
}
template <typename PointT, typename Metric, typename Ce, typename Te>
inline int pcl_icp(constraint_t &registration_cons, int max_iter_num, float dis_thre_unit, Metric metrics, Ce ce, Te te, bool use_reciprocal_correspondence,
				   bool use_trimmed_rejector, float neighbor_radius = 2.0, Eigen::Matrix4d initial_guess = Eigen::Matrix4d::Identity(),
				   bool apply_intersection_filter = true, float fitness_score_thre = 10.0)
{
	mulls_ctx *ctx = thread_context();
	mulls_pcl_icp_problem P;
	detail::ndt_fill(registration_cons, initial_guess, P);
	const mulls_pcl_icp_params prm = pcl_icp_params(max_iter_num, dis_thre_unit, (int)metrics, (int)ce, (int)te, use_reciprocal_correspondence, use_trimmed_rejector,
													neighbor_radius, apply_intersection_filter, fitness_score_thre);
	mulls_pcl_icp_result R;
	const int rc = mulls_pcl_icp(ctx, &P, &prm, &R);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_pcl_icp failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (int k = 0; k < 16; k++)
		registration_cons.Trans1_2.data()[k] = R.T[k];
	return R.code;
}
// many constraints in one call (mulls_pcl_icp_batch): every constraint with the bits of its pcl_icp call; initial_guesses is empty (identity for all)
// or one matrix per constraint.  Returns the process codes.
template <typename PointT, typename Metric, typename Ce, typename Te>
inline std::vector<int> pcl_icp_batch(std::vector<constraint_t> &registration_cons, int max_iter_num, float dis_thre_unit, Metric metrics, Ce ce, Te te,
									  bool use_reciprocal_correspondence, bool use_trimmed_rejector, float neighbor_radius = 2.0,
									  const std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>> &initial_guesses = {},
									  bool apply_intersection_filter = true, float fitness_score_thre = 10.0)
{
	const size_t B = registration_cons.size();
	if (!initial_guesses.empty() && initial_guesses.size() != B)
		throw std::runtime_error("lo::hip::pcl_icp_batch: one initial guess per constraint, or none");
	mulls_ctx *ctx = thread_context();
	std::vector<mulls_pcl_icp_problem> problems(B);
	for (size_t k = 0; k < B; k++)
		detail::ndt_fill(registration_cons[k], initial_guesses.empty() ? Eigen::Matrix4d(Eigen::Matrix4d::Identity()) : initial_guesses[k], problems[k]);
	const mulls_pcl_icp_params prm = pcl_icp_params(max_iter_num, dis_thre_unit, (int)metrics, (int)ce, (int)te, use_reciprocal_correspondence, use_trimmed_rejector,
													neighbor_radius, apply_intersection_filter, fitness_score_thre);
	std::vector<mulls_pcl_icp_result> R(B);
	const int rc = mulls_pcl_icp_batch(ctx, problems.data(), (uint32_t)B, &prm, R.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_pcl_icp_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	std::vector<int> codes(B);
	for (size_t k = 0; k < B; k++)
	{
		for (int e = 0; e < 16; e++)
			registration_cons[k].Trans1_2.data()[e] = R[k].T[e];
		codes[k] = R[k].code;
	}
	return codes;
}

} // namespace hip
} // namespace lo

#endif // MULLS_CREGISTRATION_HIP_HPP
