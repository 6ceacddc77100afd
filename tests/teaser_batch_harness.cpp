// Test harness: C entry points around mulls_amd/csrc/teaser_batch.h, the planner of mulls_coarse_reg_teaser_batch (sub-batch cuts of both phases, the arena
// layout, the descriptor table), built for the CPU so that tests/test_teaser_batch.py can check it without a device.
#include <cstring>

#include "../mulls_amd/csrc/teaser_batch.h"

extern "C"
{
	uint64_t tb_problem_bytes(uint32_t n) { return teaser_batch_problem_bytes(n); }
	uint64_t tb_weight_bytes(uint32_t C) { return teaser_batch_weight_bytes(C); }
	uint32_t tb_desc_bytes(void) { return (uint32_t)sizeof(TeaserBatchDesc); }
	uint32_t tb_max_problems(void) { return MULLS_TEASER_BATCH_MAX_PROBLEMS; }

	// cuts: count + 1 entries at most; returns the number written (sub-batches + 1, or 1 for an empty batch)
	uint32_t tb_cuts(const uint64_t *bytes, uint32_t count, uint64_t limit, uint32_t *cuts)
	{
		std::vector<uint32_t> c;
		teaser_batch_cuts(bytes, count, limit, &c);
		std::memcpy(cuts, c.data(), c.size() * 4u);
		return (uint32_t)c.size();
	}

	// the layout of the problems n[0 .. count); with m: the sub-matrices packed; with C: the cliques' points packed and the weights of [w_first, w_last) placed.
	// desc: 18 words per problem (src tgt idx adj sub deg core keep cs ct part weights M n W m Wm C); info: dev_bytes pin_bytes o_pts pts_bytes o_sub o_cpts
	// packed_sub packed_cpts weight_bytes o_desc o_gnc o_sum o_jobs o_frozen o_adj
	void tb_layout(const uint32_t *n, uint32_t count, const uint32_t *m, const uint32_t *C, uint32_t w_first, uint32_t w_last, uint64_t *desc, uint64_t *info)
	{
		TeaserBatchLayout L;
		teaser_batch_layout(n, count, &L);
		uint64_t packed_sub = 0, packed_cpts = 0, weights = 0;
		if (m)
			packed_sub = teaser_batch_pack_sub(&L, m);
		if (C)
		{
			packed_cpts = teaser_batch_pack_clique(&L, C);
			weights = teaser_batch_place_weights(&L, w_first, w_last);
		}
		for (uint32_t b = 0; b < count; b++)
		{
			const TeaserBatchDesc &D = L.desc[b];
			const uint64_t row[18] = {D.src, D.tgt, D.idx, D.adj, D.sub, D.deg, D.core, D.keep, D.cs, D.ct, D.part, D.weights, D.M, D.n, D.W, D.m, D.Wm, D.C};
			std::memcpy(desc + (size_t)18u * b, row, sizeof(row));
		}
		const uint64_t out[15] = {L.dev_bytes, L.pin_bytes, L.o_pts, L.pts_bytes, L.o_sub, L.o_cpts, packed_sub, packed_cpts, weights, L.o_desc,
								  L.o_gnc,	   L.o_sum,	   L.o_jobs, L.o_frozen, L.o_adj};
		std::memcpy(info, out, sizeof(out));
	}
}
