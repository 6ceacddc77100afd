// map_internal.h — what map.cpp (a map's life, mulls_map_set, the downloads) and map_batch.cpp (mulls_map_update and mulls_map_update_batch: lock-step groups
// of maps) share: the map itself, and the host arithmetic of every phase of an update.  Nothing here is ABI.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstring>

#include "ctx.h"
#include "device_types.h"
#include "hostmath.h"
#include "map_launch.h"

struct mulls_map
{
	float4 *rec[MULLS_NC] = {}; // class clouds, 48-B records
	float4 *alt[MULLS_NC] = {}; // compaction target (ping-pong)
	size_t cap[MULLS_NC] = {}, cap_alt[MULLS_NC] = {};
	uint32_t n[MULLS_NC] = {};
	float4 *frame[MULLS_NC] = {}, *frame_alt[MULLS_NC] = {};
	size_t cap_frame[MULLS_NC] = {}, cap_frame_alt[MULLS_NC] = {};
	uint32_t frame_n[MULLS_NC] = {};
	double pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; // pose_lo, column-major
	uint32_t *counts = nullptr; // [6] device
	uint32_t *keys = nullptr;	// [12] device
	double *T12 = nullptr;		// [12] device
	uint32_t *best = nullptr;
	uint8_t *keep = nullptr;
	size_t cap_best = 0, cap_keep = 0;
	uint8_t *dmask = nullptr; // the thinning masks of a frame's update
	size_t cap_dmask = 0;
	uint32_t *seg = nullptr; // per-segment counters of the stable compactions
	size_t cap_seg = 0;
	bool has_bounds = false; // the last update's report (what a submap snapshot carries on: mulls_submaps_push_map)
	double local_bound[6] = {}, bound[6] = {};
};

namespace mulls_mapi
{
using mulls::Mat4;
const size_t REC = MULLS_POINT_BYTES;

inline void rows12_of(const Mat4 &M, double out[12])
{
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 4; c++)
			out[r * 4 + c] = M.at(r, c);
}

// step 2 and step 5: tran_target_map = last_target.pose_lo^-1 * local_map.pose_lo (map_manager.cpp:28); the frame's five *_down clouds go to the map frame by
// its inverse (:32), the map to the frame's coordinates by itself (:57-59); step 8 poses the bounds by the frame's pose_lo
struct UpdatePoses
{
	double frame_to_map[12], map_to_frame[12], frame_pose[12]; // rows of [R|t]
};
inline void update_poses(const double map_pose[16], const double frame_pose_lo[16], UpdatePoses *out)
{
	Mat4 map_T, frame_T;
	std::memcpy(map_T.v, map_pose, sizeof(map_T.v));
	std::memcpy(frame_T.v, frame_pose_lo, sizeof(frame_T.v));
	const Mat4 tran_target_map = mulls::invert4(frame_T) * map_T;
	const Mat4 inv = mulls::invert4(tran_target_map);
	rows12_of(inv, out->frame_to_map);
	rows12_of(tran_target_map, out->map_to_frame);
	rows12_of(frame_T, out->frame_pose);
}

// step 3: dynamic_dist_thre_max as map_scan_feature_pts_distance_removal uses it (:37-47)
inline float removal_dmax(const mulls_map_params *P)
{
	float dmax = P->dynamic_dist_thre_max;
	const double lo = P->dynamic_dist_thre_min + 0.1;
	dmax = (float)(((double)dmax > lo) ? (double)dmax : lo);
	return dmax;
}
// ... whether the removal runs at all (the map's feature points against max_num_pts / 5), which of the pillar, beam and facade clouds it takes (a used class with
// a tree, more than 10 frame points and a non-empty map class) and where each starts in the map's `best` / `keep` ranges (multiples of 4 words)
struct RemovalPlan
{
	bool ran;
	bool run[3];
	uint32_t first[3], total;
};
inline const int *removal_order()
{
	static const int order[3] = {MULLS_PILLAR, MULLS_BEAM, MULLS_FACADE};
	return order;
}
inline RemovalPlan removal_plan(const mulls_map *m, const mulls_map_params *P)
{
	RemovalPlan R;
	std::memset(&R, 0, sizeof(R));
	const int fpn0 = (int)(m->n[MULLS_GROUND] + m->n[MULLS_FACADE] + m->n[MULLS_ROOF] + m->n[MULLS_PILLAR] + m->n[MULLS_BEAM]);
	R.ran = P->map_based_dynamic_removal_on && fpn0 > P->max_num_pts / 5 && P->tree_mode != 0;
	if (!R.ran)
		return R;
	for (int k = 0; k < 3; k++)
	{
		const int c = removal_order()[k];
		R.run[k] = !(P->used_feature_type[c] != '1' || P->tree_used[c] != '1' || m->frame_n[c] <= 10 || m->n[c] == 0);
		R.first[k] = R.total;
		if (R.run[k])
			R.total += (m->frame_n[c] + 3u) & ~3u;
	}
	return R;
}

// step 7: random_downsample_pcl's per-class share of max_num_pts (:70-86); returns the bytes of mask the classes above their share need (0: nothing to thin)
inline size_t thinning_plan(const uint32_t n[MULLS_NC], const mulls_map_params *P, int kept[MULLS_NC])
{
	const int cur = (int)(n[MULLS_GROUND] + n[MULLS_FACADE] + n[MULLS_ROOF] + n[MULLS_PILLAR] + n[MULLS_BEAM]);
	for (int c = 0; c < 5; c++)
		kept[c] = cur > 0 ? (int)(1.0 * P->max_num_pts / cur * n[c] + 1) : 1;
	kept[MULLS_VERTEX] = P->kept_vertex_num;
	size_t mask_total = 0;
	for (int c = 0; c < MULLS_NC; c++)
		if ((long)n[c] > (long)kept[c])
			mask_total += n[c];
	return mask_total;
}

// step 8: the 12 ordered-uint keys before the launch, and what they say afterwards
inline void bound_keys_init(uint32_t keys[12])
{
	for (int k = 0; k < 12; k++)
		keys[k] = (k % 6) < 3 ? 0xffffffffu : 0u;
}
inline double key_to_double(uint32_t k, bool is_min)
{
	const bool none = is_min ? k == 0xffffffffu : k == 0u;
	if (none)
		return is_min ? 1.7976931348623157e308 : -1.7976931348623157e308;
	const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
	float f;
	std::memcpy(&f, &u, sizeof(f));
	return (double)f;
}
inline void bound_keys_decode(const uint32_t keys[12], mulls_map *m, mulls_map_report *rep)
{
	for (int k = 0; k < 6; k++)
	{
		rep->local_bound[k] = key_to_double(keys[k], k < 3);
		rep->bound[k] = key_to_double(keys[6 + k], k < 3);
	}
	std::memcpy(m->local_bound, rep->local_bound, sizeof(m->local_bound));
	std::memcpy(m->bound, rep->bound, sizeof(m->bound));
	m->has_bounds = true;
}

// step 9: update_cloud_vectors' constants (:98-118): pca_radius 1.8, pca_max_k 20, pca_min_k 6, min_linearity 0.65, pillars kept above sin 0.80, beams below 0.25
inline const int *refresh_classes()
{
	static const int cls[2] = {MULLS_PILLAR, MULLS_BEAM};
	return cls;
}
inline bool refresh_runs(const mulls_map *m, const mulls_map_params *P, int k)
{
	const int c = refresh_classes()[k];
	return P->recalculate_feature_on && P->used_feature_type[c] == '1' && m->n[c] != 0;
}
inline void refresh_args(int k, float4 *recs, uint32_t n, uint8_t *keep, MapPcaArgs *pa)
{
	static const float sin_low[2] = {0.0f, 0.25f}, sin_high[2] = {0.80f, 1.0f};
	pa->recs = recs;
	pa->n = n;
	pa->radius = 1.8f;
	pa->max_k = 20;
	pa->min_k = 6;
	pa->sin_low = sin_low[k];
	pa->sin_high = sin_high[k];
	pa->min_linearity = 0.65f;
	pa->keep = keep;
}
inline void report_sizes(const mulls_map *m, mulls_map_report *rep)
{
	for (int c = 0; c < MULLS_NC; c++)
		rep->n[c] = m->n[c];
	rep->feature_point_num = (int)(m->n[MULLS_GROUND] + m->n[MULLS_FACADE] + m->n[MULLS_ROOF] + m->n[MULLS_PILLAR] + m->n[MULLS_BEAM]);
}
} // namespace mulls_mapi
