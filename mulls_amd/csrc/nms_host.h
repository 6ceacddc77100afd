// nms_host.h — the one step of CFilter::non_max_suppress that upstream hands to the toolchain: the visiting order, std::sort by normal[3] descending
// (cfilter.hpp:1193, :1255).  Equal keys fall as this toolchain's std::sort leaves them, and std::sort is not stable: the order among them is whatever its
// introsort does, which depends on the comparisons' outcomes and on the count only, not on what else an element carries.  So (key, index) pairs are sorted
// with upstream's comparator and the indices are the permutation upstream's record sort applies.  classify.cpp (the class clouds) and nms.cpp (the key
// points) both run these lines; tests/nms_harness.cpp holds them against a std::sort of whole 48-byte records.  Plain C++, no device headers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

struct NmsKeyIdx
{
	float key;
	uint32_t idx;
};
// perm[i] = the index of the point visited i-th.  A NaN key makes the comparator no strict weak order: callers refuse such input before they come here.
inline void nms_visiting_order(const float *keys, uint32_t n, uint32_t *perm)
{
	std::vector<NmsKeyIdx> ki(n);
	for (uint32_t i = 0; i < n; i++)
		ki[i] = NmsKeyIdx{keys[i], i};
	// the comparator of cfilter.hpp:1193 / :1255
	std::sort(ki.begin(), ki.end(), [](const NmsKeyIdx &a, const NmsKeyIdx &b) { return a.key > b.key; });
	for (uint32_t i = 0; i < n; i++)
		perm[i] = ki[i].idx;
}
