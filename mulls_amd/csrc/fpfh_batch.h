// fpfh_batch.h — the planner of mulls_coarse_reg_fpfhsac_batch and mulls_compute_fpfh_batch: the arena bytes a cloud and a problem are counted with when
// a call is cut into sub-batches, and the cut of a sub-batch's flat list of hypotheses into the stretches whose nearest-target distances are held at a
// time.  Host code without HIP, so that tests/fpfh_batch_harness.cpp can hold it on the CPU.  include/mulls_hip.h states the same formulas.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "subbatch.h"

namespace fpfh_batch
{
constexpr uint32_t MAX_SLOTS = 1024u;			  // MULLS_FPFH_HYP_CHUNK: slots of a stretch, and problems of a sub-batch
constexpr uint64_t SLOT_BYTES = 2048u;			  // counted per slot of a stretch: its NdtDesc and NdtRec (fpfh.cpp asserts that they fit)
constexpr uint64_t HEAD_BYTES = MAX_SLOTS * SLOT_BYTES; // of every sub-batch: the stretch's slots
constexpr uint64_t CLOUD_TABLE_BYTES = 1024u;	  // counted per cloud: its FpfhDesc, RegTab[MULLS_REG_TABS] and RegHead (asserted likewise)
constexpr uint64_t PROBLEM_TABLE_BYTES = 4096u;	  // counted per problem: its table entry, FpfhSacOut, winner's frame, NdtDesc and NdtRec (asserted likewise)
constexpr uint64_t MAX_POOL_BYTES = 256ull << 20; // what the single call allows its distances
constexpr uint32_t MAX_CLOUDS = 4096u;			  // clouds of one launch set of the descriptors (a grid dimension)

// the slots of a cloud's cell table: a power of two >= max(2 n, 1024) (reg_table.h)
inline uint64_t table_slots(uint64_t n)
{
	uint64_t slots = 1024u;
	while (slots < 2 * n)
		slots <<= 1;
	return slots;
}
// a cloud of n points in the arena: coordinates and normals as given and in cell order (4 x 12 n), SPFH and FPFH (2 x 132 n), the neighbourhood sizes, the
// points' slots and the lists (3 x 4 n), each rounded up to 256 bytes, 20 bytes a slot, and its table entries
inline uint64_t cloud_bytes(uint64_t n) { return 4 * up256(12 * n) + 2 * up256(132 * n) + 3 * up256(4 * n) + 20 * table_slots(n) + CLOUD_TABLE_BYTES; }
// a problem: both clouds (a cloud shared with another problem is counted for each), samples, ranks, correspondences, frames and errors of `iters`
// hypotheses (140 bytes each, and the five arrays' rounding), the winner's distances, one hypothesis of the distance pool, and its table entries
inline uint64_t problem_bytes(uint64_t n_src, uint64_t n_tgt, uint64_t iters)
{
	return cloud_bytes(n_src) + cloud_bytes(n_tgt) + 140 * iters + 1280 + 2 * up256(4 * n_src) + PROBLEM_TABLE_BYTES;
}
// The distance pool of a sub-batch whose problems were counted with `counted` bytes (HEAD_BYTES included): what the limit leaves beside the one
// hypothesis every problem was counted with, at most MAX_POOL_BYTES and at most what all hypotheses need; at least one hypothesis of the largest source.
inline uint64_t pool_bytes(const uint32_t *n_src, uint32_t P, uint32_t iters, uint64_t counted, uint64_t limit)
{
	uint64_t one = 0, least = 0, all = 0;
	for (uint32_t b = 0; b < P; b++)
		one += up256(4ull * n_src[b]), least = std::max<uint64_t>(least, 4ull * n_src[b]), all += 4ull * n_src[b] * iters;
	const uint64_t left = limit > counted - one ? limit - (counted - one) : 0;
	return std::max(least, std::min({left, MAX_POOL_BYTES, all}));
}

// hypotheses [h0, h0 + n) of the flat list (problem b's are b iters .. (b + 1) iters - 1); slot j's distances lie at byte d(h0 + j) - d0 of the pool,
// d(h) = the distance bytes of all hypotheses before h
struct Stretch
{
	uint32_t h0, n;
	uint64_t d0, bytes;
	uint32_t n_src_max; // over the problems it touches
};
// d(first hypothesis of problem b), P + 1 entries
inline std::vector<uint64_t> dist_prefix(const uint32_t *n_src, uint32_t P, uint32_t iters)
{
	std::vector<uint64_t> d(P + 1, 0);
	for (uint32_t b = 0; b < P; b++)
		d[b + 1] = d[b] + 4ull * n_src[b] * iters;
	return d;
}
// Consecutive stretches over all P iters hypotheses, in order: each takes hypotheses while it has fewer than MAX_SLOTS and its distances fit the pool.
// A stretch may begin and end inside a problem.  pool >= 4 max(n_src) (else a hypothesis that does not fit still runs alone: nothing is skipped).
inline void stretches(const uint32_t *n_src, uint32_t P, uint32_t iters, uint64_t pool, std::vector<Stretch> *out)
{
	out->clear();
	Stretch S{0, 0, 0, 0, 0};
	uint64_t d = 0;
	for (uint32_t b = 0; b < P; b++)
	{
		const uint64_t one = 4ull * n_src[b];
		for (uint32_t left = iters; left;)
		{
			const uint64_t room = pool > S.bytes ? (pool - S.bytes) / one : 0;
			uint32_t take = (uint32_t)std::min<uint64_t>({left, MAX_SLOTS - S.n, room});
			if (!take && !S.n)
				take = 1;
			if (!take)
			{
				out->push_back(S);
				S = Stretch{S.h0 + S.n, 0, d, 0, 0};
				continue;
			}
			S.n += take, S.bytes += one * take, S.n_src_max = std::max(S.n_src_max, n_src[b]);
			d += one * take, left -= take;
		}
	}
	if (S.n)
		out->push_back(S);
}
} // namespace fpfh_batch
