// teaser_batch.h — the planner of mulls_coarse_reg_teaser_batch (include/mulls_hip.h): host code without HIP, so that
// tests/teaser_batch_harness.cpp can hold it on the CPU.  A batch is cut into consecutive sub-batches twice, by two resources planned separately:
//   graph phase  every per-problem array but the weights, in one device arena (teaser_batch_problem_bytes(n) each; the two bit matrices, 2 n ceil(n / 64) 8
//                bytes, are nearly all of it at large n) — the arena of a sub-batch stays at or below the limit;
//   GNC phase    the weights, C (C - 1) / 2 doubles per problem, known only after the clique search — the problems of one graph sub-batch are cut
//                again so that the weights of the problems that run the loop in lock-step stay at or below the limit.
// A problem larger than the limit runs alone.  The descriptor table (one TeaserBatchDesc per problem) is what the k_tb_* kernels of k_teaser.hip read.
#pragma once
#include <stdint.h>

#include <vector>

#include "pair_gather.h"
#include "subbatch.h"
#include "teaser_math.h"

// one problem of a sub-batch, as the device sees it: byte offsets into the arena (weights: into the weights arena), all multiples of 256
struct TeaserBatchDesc
{
	uint64_t src, tgt;	  // n float4 each: the pairs' points
	uint64_t idx;		  // 2 n int32: the index lists of a device-resident indexed problem (target's, then source's)
	uint64_t adj, sub;	  // n x W words; m x Wm words (sub: packed once m is known)
	uint64_t deg, core;	  // n uint32; 2 n uint32 (core numbers, then greedy clique sizes)
	uint64_t keep;		  // n int32: the kept vertices, later the clique
	uint64_t cs, ct;	  // C float4 each (packed once C is known)
	uint64_t part;		  // 9 x MULLS_TEASER_PARTIALS doubles
	uint64_t weights;	  // M doubles
	uint64_t M;			  // C (C - 1) / 2
	uint32_t n, W, m, Wm; // pairs, words per row; kept vertices, words per row of sub
	uint32_t C, pad;	  // clique size (below 2: the problem never enters the GNC loop)
};

#define MULLS_TEASER_BATCH_MAX_PROBLEMS 16384u // problems of one sub-batch: a grid axis

struct TeaserBatchLayout
{
	std::vector<TeaserBatchDesc> desc;
	// device arena: the tables (descriptors, TeaserGnc records, degree sums, frozen words, two gather jobs: per problem), then one region per array kind
	uint64_t o_desc = 0, o_gnc = 0, o_sum = 0, o_frozen = 0, o_jobs = 0, o_pts = 0, o_idx = 0, o_adj = 0, o_sub = 0, o_deg = 0, o_core = 0, o_keep = 0, o_cpts = 0, o_part = 0;
	uint64_t dev_bytes = 0;
	// pinned mirror of the regions that travel; an array lies at the same offset inside its region as on the device
	uint64_t p_desc = 0, p_gnc = 0, p_sum = 0, p_jobs = 0, p_pts = 0, p_idx = 0, p_sub = 0, p_core = 0, p_keep = 0, p_cpts = 0;
	uint64_t pin_bytes = 0;
	uint64_t pts_bytes = 0, idx_bytes = 0, core_bytes = 0, keep_bytes = 0; // the regions that move whole
};

// the arena bytes of one problem (its share of the tables is counted as 512)
inline uint64_t teaser_batch_problem_bytes(uint32_t n)
{
	const uint64_t W = (n + 63u) / 64u, mat = up256((uint64_t)n * W * 8u), p16 = up256((uint64_t)n * 16u);
	return 4u * p16 + 2u * up256((uint64_t)n * 8u) + 2u * mat + 2u * up256((uint64_t)n * 4u) +
		   up256((uint64_t)9u * MULLS_TEASER_PARTIALS * 8u) + 512u;
}

// the weights of a clique of C
inline uint64_t teaser_batch_weight_bytes(uint32_t C) { return C < 2u ? 0u : up256((uint64_t)C * (C - 1u) / 2u * 8u); }

// the cut rule of subbatch.h with this batch's constant
inline void teaser_batch_cuts(const uint64_t *bytes, uint32_t count, uint64_t limit, std::vector<uint32_t> *cuts) { sub_batch_cuts(bytes, count, limit, MULLS_TEASER_BATCH_MAX_PROBLEMS, cuts); }

// the arena of the problems n[0 .. count): every offset but sub, cs, ct and weights
inline void teaser_batch_layout(const uint32_t *n, uint32_t count, TeaserBatchLayout *L)
{
	L->desc.assign(count, TeaserBatchDesc());
	uint64_t off = 0;
	auto table = [&](uint64_t entry) { // (every entry size but the last is a multiple of 8: the tables are 8-byte aligned)
		const uint64_t at = off;
		off += entry * count;
		return at;
	};
	L->o_desc = table(sizeof(TeaserBatchDesc)), L->o_gnc = table(sizeof(TeaserGnc)), L->o_sum = table(8);
	L->o_jobs = table(2u * sizeof(PairGather)), L->o_frozen = table(4);
	off = up256(off); // (at most 512 bytes per problem)
	auto region = [&](uint64_t TeaserBatchDesc::*field, uint64_t per_point, bool matrix, bool fixed) {
		const uint64_t at = off;
		for (uint32_t b = 0; b < count; b++)
		{
			const uint64_t W = (n[b] + 63u) / 64u;
			L->desc[b].*field = off;
			off += up256(fixed ? per_point : (matrix ? (uint64_t)n[b] * W * 8u : (uint64_t)n[b] * per_point));
		}
		return at;
	};
	L->o_pts = off;
	for (uint32_t b = 0; b < count; b++) // a problem's source and target points lie side by side
	{
		L->desc[b].n = n[b], L->desc[b].W = (n[b] + 63u) / 64u;
		L->desc[b].src = off, off += up256((uint64_t)n[b] * 16u);
		L->desc[b].tgt = off, off += up256((uint64_t)n[b] * 16u);
	}
	L->pts_bytes = off - L->o_pts;
	L->o_idx = region(&TeaserBatchDesc::idx, 8, false, false), L->idx_bytes = off - L->o_idx;
	L->o_adj = region(&TeaserBatchDesc::adj, 0, true, false);
	L->o_sub = region(&TeaserBatchDesc::sub, 0, true, false);
	L->o_deg = region(&TeaserBatchDesc::deg, 4, false, false);
	L->o_core = region(&TeaserBatchDesc::core, 8, false, false), L->core_bytes = off - L->o_core;
	L->o_keep = region(&TeaserBatchDesc::keep, 4, false, false), L->keep_bytes = off - L->o_keep;
	L->o_cpts = off;
	for (uint32_t b = 0; b < count; b++)
	{
		L->desc[b].cs = off, off += up256((uint64_t)n[b] * 16u);
		L->desc[b].ct = off, off += up256((uint64_t)n[b] * 16u);
	}
	L->o_part = region(&TeaserBatchDesc::part, (uint64_t)9u * MULLS_TEASER_PARTIALS * 8u, false, true);
	L->dev_bytes = off;
	uint64_t p = 0;
	auto mirror = [&](uint64_t bytes) {
		const uint64_t at = p;
		p += up256(bytes);
		return at;
	};
	L->p_desc = mirror(sizeof(TeaserBatchDesc) * count), L->p_gnc = mirror(sizeof(TeaserGnc) * count), L->p_sum = mirror((uint64_t)8u * count);
	L->p_jobs = mirror(2u * sizeof(PairGather) * count);
	L->p_pts = mirror(L->pts_bytes), L->p_idx = mirror(L->idx_bytes), L->p_sub = mirror(L->o_deg - L->o_sub), L->p_core = mirror(L->core_bytes);
	L->p_keep = mirror(L->keep_bytes), L->p_cpts = mirror(L->o_part - L->o_cpts);
	L->pin_bytes = p;
}

// m[b] kept vertices (0: no search): the sub-matrices packed from the region's start, so that they come down in one copy.  Returns the packed bytes.
inline uint64_t teaser_batch_pack_sub(TeaserBatchLayout *L, const uint32_t *m)
{
	uint64_t off = L->o_sub;
	for (size_t b = 0; b < L->desc.size(); b++)
	{
		TeaserBatchDesc &D = L->desc[b];
		D.m = m[b], D.Wm = (m[b] + 63u) / 64u, D.sub = off; // (m <= n: the packed matrices end inside the region)
		off += up256((uint64_t)D.m * D.Wm * 8u);
	}
	return off - L->o_sub;
}

// C[b] clique sizes: the clique's source and target points packed from the region's start.  Returns the packed bytes.
inline uint64_t teaser_batch_pack_clique(TeaserBatchLayout *L, const uint32_t *C)
{
	uint64_t off = L->o_cpts;
	for (size_t b = 0; b < L->desc.size(); b++)
	{
		TeaserBatchDesc &D = L->desc[b];
		D.C = C[b], D.M = C[b] < 2u ? 0u : (uint64_t)C[b] * (C[b] - 1u) / 2u;
		D.cs = off, off += up256((uint64_t)C[b] * 16u);
		D.ct = off, off += up256((uint64_t)C[b] * 16u);
	}
	return off - L->o_cpts;
}

// the weights of the problems first .. last of the layout, from the start of the weights arena.  Returns their bytes.
inline uint64_t teaser_batch_place_weights(TeaserBatchLayout *L, uint32_t first, uint32_t last)
{
	uint64_t off = 0;
	for (uint32_t b = first; b < last; b++)
		L->desc[b].weights = off, off += teaser_batch_weight_bytes(L->desc[b].C);
	return off;
}
