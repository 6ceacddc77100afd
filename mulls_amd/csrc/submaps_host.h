// submaps_host.h — the host arithmetic of the submap archive (include/mulls_hip.h, "the submap archive"): Constraint_Finder's calculate_iou,
// judge_adjacent_by_id and find_overlap_registration_constraint (src/build_pose_graph.cpp:123-209, :560-590) on poses and bounds that are already on the
// host.  No device work: a few hundred boxes.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mulls_hip.h"
#include "hostmath.h"

namespace mulls
{
namespace submaps
{
// calculate_iou (:571-590), bounds as {min_x, min_y, min_z, max_x, max_y, max_z}; max_ / min_ are utility.hpp:31-32
inline double calculate_iou(const double b1[6], const double b2[6])
{
	auto max_ = [](double a, double b) { return a > b ? a : b; };
	auto min_ = [](double a, double b) { return a < b ? a : b; };
	const double area1 = (b1[3] - b1[0]) * (b1[4] - b1[1]);
	const double area2 = (b2[3] - b2[0]) * (b2[4] - b2[1]);
	const double x1 = max_(b1[0], b2[0]);
	const double y1 = max_(b1[1], b2[1]);
	const double x2 = min_(b1[3], b2[3]);
	const double y2 = min_(b1[4], b2[4]);
	const double w = max_(0.0, x2 - x1);
	const double h = max_(0.0, y2 - y1);
	const double area1i2 = w * h;
	return area1i2 / (area1 + area2 - area1i2);
}

// judge_adjacent_by_id (:560-569)
inline bool adjacent_by_id(int64_t id_1, int64_t id_2, int64_t diff) { return id_1 <= id_2 + diff && id_1 >= id_2 - diff; }

// find_overlap_registration_constraint for blocks = infos[0 .. cur]; the edges in output order
inline std::vector<mulls_submap_edge> find_overlap(const mulls_submap_info *infos, uint32_t cur, const mulls_overlap_params &P)
{
	std::vector<mulls_submap_edge> edges;
	if ((uint64_t)cur + 1u < (uint64_t)P.adjacent_id_thre + 2u)
		return edges;
	struct Nb
	{
		float d2;
		uint32_t id;
	};
	std::vector<Nb> nb;
	const int dims = P.search_2d ? 2 : 3;
	const float r2 = (float)((double)P.neighbor_search_dist * (double)P.neighbor_search_dist);
	for (uint32_t i = 0; i < cur; i++)
	{
		float d2 = 0.0f;
		for (int k = 0; k < dims; k++)
		{
			const float d = (float)infos[cur].pose_lo[12 + k] - (float)infos[i].pose_lo[12 + k];
			d2 += d * d;
		}
		if (d2 < r2)
			nb.push_back({d2, i});
	}
	std::stable_sort(nb.begin(), nb.end(), [](const Nb &a, const Nb &b) { return a.d2 < b.d2; }); // (ids ascend within equal distances)
	if (P.max_neighbor > 0 && nb.size() > (size_t)P.max_neighbor)
		nb.resize((size_t)P.max_neighbor);
	for (const Nb &q : nb)
	{
		const double iou = calculate_iou(infos[cur].bound, infos[q.id].bound);
		if (adjacent_by_id(infos[cur].id_in_strip, infos[q.id].id_in_strip, P.adjacent_id_thre) || !(iou > (double)P.min_iou_thre))
			continue;
		mulls_submap_edge e;
		std::memset(&e, 0, sizeof(e));
		e.tgt_id = (int32_t)q.id, e.src_id = (int32_t)cur;
		e.overlapping_ratio = iou;
		Mat4 tgt, src;
		std::memcpy(tgt.v, infos[q.id].pose_lo, sizeof(tgt.v));
		std::memcpy(src.v, infos[cur].pose_lo, sizeof(src.v));
		const Mat4 T = invert4(tgt) * src;
		std::memcpy(e.Trans1_2, T.v, sizeof(T.v));
		edges.push_back(e);
	}
	std::stable_sort(edges.begin(), edges.end(), [](const mulls_submap_edge &a, const mulls_submap_edge &b) { return a.overlapping_ratio > b.overlapping_ratio; });
	return edges;
}
} // namespace submaps
} // namespace mulls
