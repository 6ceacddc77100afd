// Test harness of the key-point non-maximum suppression, built for the CPU: CFilter::non_max_suppress as upstream runs it (cfilter.hpp:1183-1240) — a
// std::sort of real 48-byte records with upstream's comparator, then the sequential walk over a std::set of unvisited indices — with a brute-force radius
// query in FLANN's float arithmetic in place of the kd-tree.  It shares nothing with mulls_amd/csrc/nms.cpp except, in nh_pair_order, the sort header
// nms_host.h, so that tests/test_nms.py can hold that header's (key, index) sort against the record sort here.
// Build with -ffp-contract=off.
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <set>
#include <vector>

#include "../mulls_amd/csrc/nms_host.h"

namespace
{
struct alignas(16) Rec // pcl::PointXYZINormal's layout
{
	float x, y, z, pad;
	float normal[4];
	float intensity, curvature, tail[2];
};
static_assert(sizeof(Rec) == 48, "48-byte records");

// the records, sorted as upstream sorts them; tag[i] = where the i-th record of the result stood in the input
void record_sort(const unsigned char *recs, uint32_t n, uint32_t stride, std::vector<Rec> &pts, std::vector<int32_t> &tag)
{
	pts.resize(n);
	std::vector<float> saved(n);
	for (uint32_t i = 0; i < n; i++)
	{
		std::memcpy(&pts[i], recs + (size_t)i * stride, 48);
		saved[i] = pts[i].pad; // the index rides in the record's padding float while std::sort moves the record
		std::memcpy(&pts[i].pad, &i, 4);
	}
	std::sort(pts.begin(), pts.end(), [](const Rec &a, const Rec &b) { return a.normal[3] > b.normal[3]; });
	tag.resize(n);
	for (uint32_t i = 0; i < n; i++)
	{
		uint32_t from;
		std::memcpy(&from, &pts[i].pad, 4);
		tag[i] = (int32_t)from;
		pts[i].pad = saved[from];
	}
}
} // namespace

extern "C"
{
	// order[i] = the input index of the record std::sort leaves at position i
	void nh_record_order(const unsigned char *recs, uint32_t n, uint32_t stride, int32_t *order)
	{
		std::vector<Rec> pts;
		std::vector<int32_t> tag;
		record_sort(recs, n, stride, pts, tag);
		std::memcpy(order, tag.data(), (size_t)n * 4u);
	}
	// the same from the library's shared (key, index) sort
	void nh_pair_order(const float *keys, uint32_t n, int32_t *order) { nms_visiting_order(keys, n, reinterpret_cast<uint32_t *>(order)); }

	// the whole call: returns the kept count, or -1 under the gate (nothing written).  out: n records, kept_idx / order: n ints
	int nh_suppress(const unsigned char *recs, uint32_t n, uint32_t stride, float non_max_radius, unsigned char *out, int32_t *kept_idx, int32_t *order)
	{
		const int pt_count_before = (int)n;
		if (pt_count_before < 10)
			return -1;
		std::vector<Rec> pts;
		std::vector<int32_t> tag;
		record_sort(recs, n, stride, pts, tag);
		std::memcpy(order, tag.data(), (size_t)n * 4u);
		const float r2 = (float)((double)non_max_radius * (double)non_max_radius);
		std::set<int> unvisited;
		for (int i = 0; i < pt_count_before; ++i)
			unvisited.insert(i);
		int kept = 0;
		std::vector<int> found;
		do
		{
			const int id = *unvisited.begin();
			std::memcpy(out + (size_t)kept * 48u, &pts[id], 48);
			kept_idx[kept++] = tag[id];
			unvisited.erase(id);
			found.clear();
			for (int j = 0; j < pt_count_before; j++) // the radius query
			{
				const float dx = pts[j].x - pts[id].x, dy = pts[j].y - pts[id].y, dz = pts[j].z - pts[id].z;
				if ((dx * dx + dy * dy) + dz * dz < r2)
					found.push_back(j);
			}
			for (size_t i = 0; i < found.size(); i++)
				unvisited.erase(found[i]);
		} while (!unvisited.empty());
		return kept;
	}
}
