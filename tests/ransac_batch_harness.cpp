// Test harness: C entry points around mulls_amd/csrc/ransac_batch.h, the planner of mulls_coarse_reg_ransac_batch (sub-batch cuts, the arena layout, the
// descriptor table), and around the resumable refinement control of ransac_host.h next to refine_control, built for the CPU so that
// tests/test_ransac_batch.py can check them without a device.
#include <cstring>

#include "../mulls_amd/csrc/ransac_batch.h"
#include "../mulls_amd/csrc/ransac_host.h"

extern "C"
{
	uint64_t rb_problem_bytes(uint32_t n, int32_t max_iter_num) { return ransac_batch_problem_bytes(n, max_iter_num); }
	uint32_t rb_desc_bytes(void) { return (uint32_t)sizeof(RansacBatchDesc); }
	uint32_t rb_gather_bytes(void) { return (uint32_t)sizeof(RansacBatchGather); }
	uint32_t rb_job_bytes(void) { return (uint32_t)sizeof(RansacBatchJob); }
	uint32_t rb_max_problems(void) { return MULLS_RANSAC_BATCH_MAX_PROBLEMS; }

	// cuts: count + 1 entries at most; returns the number written (sub-batches + 1, or 1 for an empty batch)
	uint32_t rb_cuts(const uint64_t *bytes, uint32_t count, uint64_t limit, uint32_t *cuts)
	{
		std::vector<uint32_t> c;
		ransac_batch_cuts(bytes, count, limit, &c);
		std::memcpy(cuts, c.data(), c.size() * 4u);
		return (uint32_t)c.size();
	}

	// the layout of the problems n[0 .. count).  desc: 13 words per problem (src tgt idx tri models counts mask d2 round n n_hyp best mask_stride);
	// info: dev_bytes pin_bytes o_desc o_win o_gather o_jobs o_pts pts_bytes o_tri tri_bytes o_counts counts_bytes o_mask mask_bytes o_round round_bytes
	void rb_layout(const uint32_t *n, uint32_t count, int32_t max_iter_num, uint64_t *desc, uint64_t *info)
	{
		RansacBatchLayout L;
		ransac_batch_layout(n, count, max_iter_num, &L);
		for (uint32_t b = 0; b < count; b++)
		{
			const RansacBatchDesc &D = L.desc[b];
			const uint64_t row[13] = {D.src, D.tgt, D.idx, D.tri, D.models, D.counts, D.mask, D.d2, D.round, D.n, D.n_hyp, (uint64_t)(int64_t)D.best, D.mask_stride};
			std::memcpy(desc + (size_t)13u * b, row, sizeof(row));
		}
		const uint64_t out[16] = {L.dev_bytes, L.pin_bytes,	 L.o_desc,	 L.o_win,		 L.o_gather, L.o_jobs,	   L.o_pts,	  L.pts_bytes,
								  L.o_tri,	   L.tri_bytes,	 L.o_counts, L.counts_bytes, L.o_mask,	 L.mask_bytes, L.o_round, L.round_bytes};
		std::memcpy(info, out, sizeof(out));
	}

	// The refinement control over a script of rounds: n_new / changed / median per round (the last entry repeats when the script runs out), by the loop
	// (refine_control, resumable = 0) or by the state fed one round at a time (refine_begin / refine_threshold / refine_feed, resumable = 1).
	// out: rounds, failed, oscillating, final_mask, n_inliers; log[2 r ..]: prev, next of round r; thresholds[r]: its squared threshold
	void rb_refine(int resumable, double noise_bound, uint32_t n_in, const uint32_t *n_new, const int32_t *changed, const float *median, int n_script, int out[5],
				   int *log, double *thresholds, int log_cap)
	{
		RefineOutcome o;
		int r = 0;
		auto round = [&](int prev, int next, double thresh, RefineStep &s) -> int {
			const int k = r < n_script ? r : n_script - 1;
			s.n_new = n_new[k], s.changed = changed[k] != 0, s.median = median[k];
			if (r < log_cap)
				log[2 * r] = prev, log[2 * r + 1] = next, thresholds[r] = thresh;
			r++;
			return 0;
		};
		if (resumable)
		{
			RefineState s;
			refine_begin(s, noise_bound, n_in);
			for (;;)
			{
				RefineStep step;
				round(s.prev, s.next, refine_threshold(s), step);
				if (!refine_feed(s, step))
					break;
			}
			o = s.o;
		}
		else
			refine_control(noise_bound, n_in, o, round);
		out[0] = o.rounds, out[1] = o.failed, out[2] = o.oscillating, out[3] = o.final_mask, out[4] = (int)o.n_inliers;
	}
}
