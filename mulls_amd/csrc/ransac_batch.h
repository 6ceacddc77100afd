// ransac_batch.h — the planner of mulls_coarse_reg_ransac_batch (include/mulls_hip.h; DESIGN.md section 7.1, addendum): host code without HIP, so that
// tests/ransac_batch_harness.cpp can hold it on the CPU.  A batch is cut into consecutive sub-batches whose device arena stays at or below the limit; a
// problem larger than the limit runs alone.  The descriptor table (one RansacBatchDesc per problem) is what the k_rb_* kernels of k_ransac.hip read.
#pragma once
#include <stdint.h>

#include <vector>

#include "pair_gather.h"
#include "subbatch.h"

#define MULLS_RANSAC_MODEL_BYTES 48u // sizeof(RansacModel), sizeof(RansacRound): ransac.cpp asserts both (ransac_launch.h needs HIP's headers)
#define MULLS_RANSAC_ROUND_BYTES 64u
#define MULLS_RANSAC_BATCH_MAX_PROBLEMS 16384u // problems of one sub-batch: a grid axis

// one problem of a sub-batch, as the device sees it: byte offsets into the arena, all multiples of 256
struct RansacBatchDesc
{
	uint64_t src, tgt; // n float4 each: the pairs' points
	uint64_t idx;	   // 2 n int32: the index lists of an indexed problem with a device-resident cloud (target's, then source's)
	uint64_t tri;	   // 3 n_hyp int32: the samples
	uint64_t models;   // n_hyp RansacModel
	uint64_t counts;   // n_hyp uint32
	uint64_t mask;	   // three masks of n bytes, mask_stride apart: [0] the winner's inliers, kept; [1], [2] the refinement rounds' sets in turn
	uint64_t d2;	   // n float
	uint64_t round;	   // one RansacRound
	uint32_t n, n_hyp; // pairs; hypotheses that have a sample (0: a pass-through problem, no kernel touches it)
	int32_t best;	   // the winning hypothesis, once the host has applied the sequential rule
	uint32_t mask_stride;
};

// a gather job of a sub-batch is the solvers' shared one (pair_gather.h); the planner's name for it, which tests/ransac_batch_harness.cpp sizes the table with
using RansacBatchGather = PairGather;

// one workgroup of a refinement round: the problem, the buffers of its previous and next inlier set, its squared threshold
struct RansacBatchJob
{
	uint32_t problem, prev, next, pad;
	double thresh;
};

struct RansacBatchLayout
{
	std::vector<RansacBatchDesc> desc;
	// device arena: the tables (descriptors, winner records, two gather jobs, one refinement job: per problem), then one region per array kind
	uint64_t o_desc = 0, o_win = 0, o_gather = 0, o_jobs = 0, o_pts = 0, o_idx = 0, o_tri = 0, o_models = 0, o_counts = 0, o_mask = 0, o_d2 = 0, o_round = 0;
	uint64_t dev_bytes = 0;
	// pinned mirror of the regions that travel; an array lies at the same offset inside its region as on the device
	uint64_t p_desc = 0, p_win = 0, p_gather = 0, p_jobs = 0, p_pts = 0, p_idx = 0, p_tri = 0, p_counts = 0, p_mask = 0, p_round = 0;
	uint64_t pin_bytes = 0;
	uint64_t pts_bytes = 0, idx_bytes = 0, tri_bytes = 0, counts_bytes = 0, mask_bytes = 0, round_bytes = 0; // the regions that move whole
};

// hypotheses of a problem at most: iteration max_iter_num is still evaluated
inline uint32_t ransac_batch_hypotheses(int32_t max_iter_num) { return (uint32_t)(max_iter_num > 0 ? max_iter_num : 0) + 1u; }

// the arena bytes of one problem (its share of the tables is counted as 512)
inline uint64_t ransac_batch_problem_bytes(uint32_t n, int32_t max_iter_num)
{
	const uint64_t H = ransac_batch_hypotheses(max_iter_num);
	return 2u * up256((uint64_t)n * 16u) + up256((uint64_t)n * 8u) + up256(H * 12u) +
		   up256(H * MULLS_RANSAC_MODEL_BYTES) + up256(H * 4u) + 3u * up256(n) + up256((uint64_t)n * 4u) +
		   up256(MULLS_RANSAC_ROUND_BYTES) + 512u;
}

// the cut rule of subbatch.h with this batch's constant
inline void ransac_batch_cuts(const uint64_t *bytes, uint32_t count, uint64_t limit, std::vector<uint32_t> *cuts) { sub_batch_cuts(bytes, count, limit, MULLS_RANSAC_BATCH_MAX_PROBLEMS, cuts); }

// the arena of the problems n[0 .. count), each with room for the hypotheses of max_iter_num
inline void ransac_batch_layout(const uint32_t *n, uint32_t count, int32_t max_iter_num, RansacBatchLayout *L)
{
	const uint64_t H = ransac_batch_hypotheses(max_iter_num);
	L->desc.assign(count, RansacBatchDesc());
	uint64_t off = 0;
	auto table = [&](uint64_t entry) { // (every entry size is a multiple of 8: the tables are 8-byte aligned)
		const uint64_t at = off;
		off += entry * count;
		return at;
	};
	L->o_desc = table(sizeof(RansacBatchDesc)), L->o_win = table(MULLS_RANSAC_ROUND_BYTES), L->o_gather = table(2u * sizeof(RansacBatchGather));
	L->o_jobs = table(sizeof(RansacBatchJob));
	off = up256(off); // (at most 512 bytes per problem)
	auto region = [&](uint64_t RansacBatchDesc::*field, uint64_t per_pair, uint64_t fixed, uint64_t *bytes) {
		const uint64_t at = off;
		for (uint32_t b = 0; b < count; b++)
		{
			L->desc[b].*field = off;
			off += up256(fixed ? fixed : (uint64_t)n[b] * per_pair);
		}
		if (bytes)
			*bytes = off - at;
		return at;
	};
	L->o_pts = off;
	for (uint32_t b = 0; b < count; b++) // a problem's source and target points lie side by side
	{
		L->desc[b].n = n[b], L->desc[b].n_hyp = 0, L->desc[b].best = -1;
		L->desc[b].src = off, off += up256((uint64_t)n[b] * 16u);
		L->desc[b].tgt = off, off += up256((uint64_t)n[b] * 16u);
	}
	L->pts_bytes = off - L->o_pts;
	L->o_idx = region(&RansacBatchDesc::idx, 8, 0, &L->idx_bytes);
	L->o_tri = region(&RansacBatchDesc::tri, 0, H * 12u, &L->tri_bytes);
	L->o_models = region(&RansacBatchDesc::models, 0, H * MULLS_RANSAC_MODEL_BYTES, nullptr);
	L->o_counts = region(&RansacBatchDesc::counts, 0, H * 4u, &L->counts_bytes);
	L->o_mask = off;
	for (uint32_t b = 0; b < count; b++) // a problem's three masks lie side by side
	{
		L->desc[b].mask = off, L->desc[b].mask_stride = (uint32_t)up256(n[b]);
		off += 3u * up256(n[b]);
	}
	L->mask_bytes = off - L->o_mask;
	L->o_d2 = region(&RansacBatchDesc::d2, 4, 0, nullptr);
	L->o_round = region(&RansacBatchDesc::round, 0, MULLS_RANSAC_ROUND_BYTES, &L->round_bytes);
	L->dev_bytes = off;
	uint64_t p = 0;
	auto mirror = [&](uint64_t bytes) {
		const uint64_t at = p;
		p += up256(bytes);
		return at;
	};
	L->p_desc = mirror(sizeof(RansacBatchDesc) * count), L->p_win = mirror((uint64_t)MULLS_RANSAC_ROUND_BYTES * count);
	L->p_gather = mirror(2u * sizeof(RansacBatchGather) * count), L->p_jobs = mirror(sizeof(RansacBatchJob) * count);
	L->p_pts = mirror(L->pts_bytes), L->p_idx = mirror(L->idx_bytes), L->p_tri = mirror(L->tri_bytes), L->p_counts = mirror(L->counts_bytes);
	L->p_mask = mirror(L->mask_bytes), L->p_round = mirror(L->round_bytes);
	L->pin_bytes = p;
}
