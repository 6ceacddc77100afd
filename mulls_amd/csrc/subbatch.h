// subbatch.h — what the planners of the batch entry points share: the 256-byte rounding of every arena offset, and the rule that cuts a batch into
// sub-batches.  Host code without HIP, so that the harnesses under tests/ can hold it on the CPU.
#pragma once
#include <stdint.h>

#include <vector>

inline uint64_t up256(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }

// Consecutive cuts: cuts[k] .. cuts[k + 1] is sub-batch k.  A sub-batch starts at head_bytes and takes problems while its bytes stay at or below the
// limit; it holds one problem at least (a problem larger than the limit runs alone) and max_count at most.  wgs, when given, is a second budget counted the
// same way: wgs[b] of problem b, at most max_wgs per sub-batch.
inline void sub_batch_cuts(const uint64_t *bytes, uint32_t count, uint64_t limit, uint32_t max_count, std::vector<uint32_t> *cuts, uint64_t head_bytes = 0,
						   const uint64_t *wgs = nullptr, uint64_t max_wgs = 0)
{
	cuts->assign(1, 0u);
	uint64_t held = head_bytes, grid = 0;
	for (uint32_t b = 0; b < count; b++)
	{
		const uint64_t w = wgs ? wgs[b] : 0u;
		if (b > cuts->back() && (held + bytes[b] > limit || (wgs && grid + w > max_wgs) || b - cuts->back() >= max_count))
			cuts->push_back(b), held = head_bytes, grid = 0;
		held += bytes[b];
		grid += w;
	}
	if (count)
		cuts->push_back(count);
}
