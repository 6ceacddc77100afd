// ransac.cpp — mulls_coarse_reg_ransac: CRegistration<PointT>::coarse_reg_ransac (cregistration.hpp:605-661), the solver between the key-point matcher
// (ncc.cpp) and mulls_icp, on the device (k_ransac.hip).  Host side: argument checks, staging (pair_stage.h), PCL's sample sequence (sequential and cheap: a
// Mersenne twister and three swaps per hypothesis), PCL's sequential "first best wins, stop at k" rule applied to the counts the device returns for every
// hypothesis, and the control flow of refineModel around one launch per round.  include/mulls_hip.h has the definition this file follows.
// mulls_coarse_reg_ransac_batch runs the same steps for many problems in lock step: ransac_batch.h plans a sub-batch's arena, the k_rb_* kernels of
// k_ransac.hip run each step for all its problems in one launch, and the refinement keeps one resumable control state (ransac_host.h) per problem.  The
// three entry points share one argument checker, the staging, pass_through and finish_inliers.
// WHY THE HOST SEQUENCE IS WRITTEN TWICE (ransac_run, ransac_sub_batch): the single calls run as a sub-batch of one were built and measured against ransac_run
// on one MI355X and were 1.4 to 5 % slower (6 to 32 us) on 15 of 33 rows, outside the parent's spread (profiles/ransac_single_as_batch.txt).  The kernel
// trace there shows the solver's kernels level and 3.4 more runtime dispatches per call: the 64-byte winner record is zeroed by three fill kernels where the
// single call's 4-byte count takes one, and the descriptor and job uploads run as copy kernels.  So ransac_run keeps its kernels with launch arguments; the two share the __device__ steps of k_ransac.hip and everything named above.
#include "pair_stage.h"
#include "ransac_host.h"
#include "ransac_launch.h"

// a context's scratch of this entry point: one device arena and one pinned host buffer, grow-only, reused between calls
struct mulls_ransac_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr;
	size_t dev_cap = 0, pin_cap = 0;
};

void mulls_ransac_release(mulls_ctx *ctx)
{
	if (!ctx->ransac)
		return;
	staggered_free(ctx->ransac->dev);
	if (ctx->ransac->pin)
		(void)hipHostFree(ctx->ransac->pin);
	delete ctx->ransac;
	ctx->ransac = nullptr;
}

namespace
{
static_assert(sizeof(RansacModel) == MULLS_RANSAC_MODEL_BYTES && sizeof(RansacRound) == MULLS_RANSAC_ROUND_BYTES, "ransac_batch.h plans with these sizes");

void reset_result(mulls_ransac_result *result)
{
	std::memset(result, 0, sizeof(*result));
	result->status = -1;
	result->best_iteration = -1;
	identity16(result->T);
}

// every correspondence passes, T = identity: PCL's outcome when no model is found, or when the model has fewer than three inliers
void pass_through(uint32_t n, int min_in, mulls_ransac_result *result, int32_t *inliers, uint32_t cap)
{
	result->n_inliers = n;
	for (uint32_t i = 0; i < std::min(n, cap); i++)
		inliers[i] = (int32_t)i;
	identity16(result->T);
	result->status = (long)n >= 2 * (long)min_in ? 1 : ((long)n >= (long)min_in ? 0 : -1);
}

// the final mask, down: the inlier list, the status and the model
void finish_inliers(const uint8_t *hm, uint32_t n, int min_in, const RansacModel &best_model, mulls_ransac_result *result, int32_t *inliers, uint32_t cap)
{
	uint32_t w = 0;
	for (uint32_t i = 0; i < n; i++)
		if (hm[i])
		{
			if (w < cap)
				inliers[w] = (int32_t)i;
			w++;
		}
	result->n_inliers = w;
	result->status = (long)w >= 2 * (long)min_in ? 1 : ((long)w >= (long)min_in ? 0 : -1);
	if (result->status >= 0)
	{
		for (int r = 0; r < 3; r++)
			for (int c = 0; c < 4; c++)
				result->T[c * 4 + r] = (double)best_model.m[r * 4 + c];
	}
}

// A problem as it was handed in, before the device is touched, in the single call's order: the refusals, or its number of pairs; *runs = false below three
// pairs (getSamples: "Can not select 3 unique points out of n"), the pass-through outcome.  indexed: the batch ABI infers it from the lists and wants both or
// none; the indexed single call says so itself and reads no list when n_corr = 0.
int check_pairs(const Refusal &refuse, const mulls_ransac_problem &P, bool indexed, const mulls_ransac_params *params, BatchProblem *A, bool *runs)
{
	*runs = false;
	const mulls_cloud &T = P.tgt, &S = P.src;
	if ((T.n && !T.pts) || (S.n && !S.pts) || (P.inlier_cap && !P.inliers))
		return refuse.quiet(MULLS_E_INVALID, "a NULL cloud or inlier buffer");
	if (!std::isfinite(params->noise_bound))
		return refuse(MULLS_E_INVALID, "noise_bound is not finite");
	A->indexed = indexed, A->n = indexed ? P.n_corr : T.n;
	if (indexed)
	{
		if ((!P.tgt_idx || !P.src_idx) && (refuse.problem >= 0 || P.n_corr))
			return refuse.quiet(MULLS_E_INVALID, "one index list without the other");
	}
	else if (T.n != S.n)
		return refuse(MULLS_E_INVALID, "the clouds' sizes differ (correspondence i pairs point i of each)");
	if (A->n > MULLS_RANSAC_MAX_POINTS || params->max_iter_num > MULLS_RANSAC_MAX_ITER)
		return refuse(MULLS_E_UNSUPPORTED, "at most 65536 pairs and max_iter_num <= 2^20");
	if (indexed)
		for (uint32_t i = 0; i < A->n; i++)
			if (P.tgt_idx[i] < 0 || (uint32_t)P.tgt_idx[i] >= T.n || P.src_idx[i] < 0 || (uint32_t)P.src_idx[i] >= S.n)
				return refuse(MULLS_E_INVALID, "an index lies outside its cloud");
	*runs = A->n >= 3u;
	return MULLS_OK;
}

int ransac_run(mulls_ctx *ctx, const mulls_cloud *tgt_in, const mulls_cloud *src_in, const int32_t *tgt_idx, const int32_t *src_idx, uint32_t n_corr,
			   bool indexed, const mulls_ransac_params *params, mulls_ransac_result *result, int32_t *inliers, uint32_t cap)
{
	const char *who = indexed ? "mulls_coarse_reg_ransac_indexed" : "mulls_coarse_reg_ransac";
	if (!ctx || !tgt_in || !src_in || !params || !result || (cap && !inliers))
		return MULLS_E_INVALID;
	reset_result(result);
	const Refusal refuse{ctx, who, -1};
	mulls_ransac_problem P;
	P.tgt = *tgt_in, P.src = *src_in;
	P.tgt_idx = tgt_idx, P.src_idx = src_idx, P.n_corr = n_corr;
	P.inliers = inliers, P.inlier_cap = cap;
	BatchProblem A;
	bool runs;
	if (int rc = check_pairs(refuse, P, indexed, params, &A, &runs))
		return rc;
	const uint32_t n = A.n;
	const int min_in = params->min_inlier_num;
	if (!runs)
	{
		pass_through(n, min_in, result, inliers, cap);
		return MULLS_OK;
	}

	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (int rc = check_strides(refuse, P.tgt, P.src, &A))
		return rc;
	if (!ctx->ransac)
		ctx->ransac = new mulls_ransac_scratch();
	mulls_ransac_scratch &sc = *ctx->ransac;
	const uint32_t n_hyp_max = ransac_batch_hypotheses(params->max_iter_num); // iteration max_iter_num is still evaluated: the loop ends on ++iterations > max
	size_t off = 0;
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return at;
	};
	const size_t o_src = take((size_t)n * 16u), o_tgt = take((size_t)n * 16u);
	const size_t o_idx = take((size_t)n * 8u), o_jobs = take(2u * sizeof(PairGather));
	const size_t o_tri = take((size_t)n_hyp_max * 12u), o_models = take((size_t)n_hyp_max * sizeof(RansacModel)), o_counts = take((size_t)n_hyp_max * 4u);
	const size_t o_mask0 = take(n), o_mask1 = take(n), o_mask2 = take(n), o_d2 = take((size_t)n * 4u), o_round = take(sizeof(RansacRound)), o_cnt = take(4);
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
		return rc;
	size_t poff = 0;
	auto ptake = [&](size_t bytes) {
		const size_t at = poff;
		poff += up256(bytes);
		return at;
	};
	const size_t p_src = ptake(2u * up256((size_t)n * 16u)), p_idx = ptake((size_t)n * 8u), p_jobs = ptake(2u * sizeof(PairGather)), p_tri = ptake((size_t)n_hyp_max * 12u);
	const size_t p_counts = ptake((size_t)n_hyp_max * 4u), p_mask = ptake(n), p_round = ptake(sizeof(RansacRound)), p_model = ptake(sizeof(RansacModel)), p_cnt = ptake(4);
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, poff, hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	float4 *src4 = reinterpret_cast<float4 *>(d + o_src), *tgt4 = reinterpret_cast<float4 *>(d + o_tgt);
	float *h_src = reinterpret_cast<float *>(h + p_src);

	// staging: a list of one (the source's and the target's points lie side by side in the arena and in its mirror); with a device-resident source the
	// points come down again, for the draws
	const PairStageItem item{&P.tgt, &P.src, tgt_idx, src_idx, n, indexed, A.t_dev, A.s_dev, o_src, o_tgt, o_idx};
	if (int rc = stage_pairs(ctx, st, d, h, PairStagePlaces{o_src, o_idx - o_src, o_idx, o_jobs - o_idx, o_jobs, p_src, p_idx, p_jobs}, &item, 1))
		return rc;
	if (A.s_dev)
	{
		HIPCHK(ctx, hipMemcpyAsync(h_src, src4, (size_t)n * 16u, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}

	// the samples of every iteration the sequential loop can reach
	std::vector<int32_t> triples;
	draw_triples(h_src, n, n_hyp_max, triples);
	const uint32_t n_hyp = (uint32_t)(triples.size() / 3u);
	if (!n_hyp) // no good sample for the first iteration: computeModel fails
	{
		pass_through(n, min_in, result, inliers, cap);
		return MULLS_OK;
	}
	const double nb = (double)params->noise_bound, thr_sqr = nb * nb;
	std::memcpy(h + p_tri, triples.data(), triples.size() * 4u);
	HIPCHK(ctx, hipMemcpyAsync(d + o_tri, h + p_tri, triples.size() * 4u, hipMemcpyHostToDevice, st));
	RansacModel *models = reinterpret_cast<RansacModel *>(d + o_models);
	uint32_t *counts = reinterpret_cast<uint32_t *>(d + o_counts);
	HIPCHK(ctx, launch_ransac_models(st, src4, tgt4, reinterpret_cast<const int32_t *>(d + o_tri), n_hyp, models));
	HIPCHK(ctx, launch_ransac_score(st, src4, tgt4, n, models, n_hyp, thr_sqr, counts));
	HIPCHK(ctx, hipMemcpyAsync(h + p_counts, counts, (size_t)n_hyp * 4u, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));

	// RandomSampleConsensus::computeModel's loop over the counts (ransac.hpp): std::log / std::pow as PCL calls them
	const uint32_t *hc = reinterpret_cast<const uint32_t *>(h + p_counts);
	int iterations = 0, best_it = -1;
	ransac_sequential_rule(hc, n_hyp, n, params->max_iter_num, &iterations, &best_it);
	result->iterations = iterations;
	result->best_iteration = best_it;

	// the winner's inliers
	uint8_t *mask[3] = {d + o_mask0, d + o_mask1, d + o_mask2}; // [0]: the winner's inliers, kept; [1], [2]: the rounds' sets in turn
	uint32_t *d_cnt = reinterpret_cast<uint32_t *>(d + o_cnt);
	RansacModel best_model;
	HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 4, st));
	HIPCHK(ctx, launch_ransac_select(st, src4, tgt4, n, models + best_it, thr_sqr, mask[0], d_cnt));
	HIPCHK(ctx, hipMemcpyAsync(h + p_model, models + best_it, sizeof(RansacModel), hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipMemcpyAsync(h + p_cnt, d_cnt, 4, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::memcpy(&best_model, h + p_model, sizeof(best_model));
	uint32_t n_in = *reinterpret_cast<const uint32_t *>(h + p_cnt);
	int final_mask = 0;

	if (params->refine)
	{
		// RandomSampleConsensus::refineModel(3.0, 1000) (sac.h): its control flow is refine_control (ransac_host.h), one launch per round
		RansacRound R;
		RefineOutcome ro;
		const int rc = refine_control(nb, n_in, ro, [&](int prev, int next, double thresh, RefineStep &step) -> int {
			HIPCHK(ctx, launch_ransac_refine(st, src4, tgt4, n, mask[prev], mask[next], reinterpret_cast<float *>(d + o_d2), thresh, reinterpret_cast<RansacRound *>(d + o_round)));
			HIPCHK(ctx, hipMemcpyAsync(h + p_round, d + o_round, sizeof(RansacRound), hipMemcpyDeviceToHost, st));
			HIPCHK(ctx, hipStreamSynchronize(st));
			std::memcpy(&R, h + p_round, sizeof(R));
			step.n_new = R.n_new, step.changed = R.changed != 0, step.median = R.median;
			return MULLS_OK;
		});
		if (rc != MULLS_OK)
			return rc;
		result->refine_iterations = ro.rounds;
		if (ro.failed)
		{
			// "Refinement failed": getRemainingCorrespondences returns with nothing
			result->n_inliers = 0;
			result->status = -1;
			return MULLS_OK;
		}
		if (!ro.oscillating) // (an oscillation returns true without installing anything: the unrefined model and its inliers stay)
		{
			best_model = R.T;
			n_in = ro.n_inliers;
			final_mask = ro.final_mask;
		}
	}
	if (n_in < 3u)
	{
		pass_through(n, min_in, result, inliers, cap);
		return MULLS_OK;
	}
	HIPCHK(ctx, hipMemcpyAsync(h + p_mask, mask[final_mask], n, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	finish_inliers(h + p_mask, n, min_in, best_model, result, inliers, cap);
	return MULLS_OK;
}

// ---- mulls_coarse_reg_ransac_batch
// one sub-batch: `count` problems of three pairs or more whose arena fits the limit (or one that does not).  The host steps are ransac_run's, each for all
// problems at once: one upload, one launch, one download and one wait where the single call makes its own.
int ransac_sub_batch(mulls_ctx *ctx, const mulls_ransac_problem *problems, const BatchProblem *act, uint32_t count, const mulls_ransac_params *params,
					 mulls_ransac_result *results)
{
	mulls_ransac_scratch &sc = *ctx->ransac;
	std::vector<uint32_t> sizes(count);
	uint32_t n_max = 0;
	bool any_s_dev = false;
	for (uint32_t k = 0; k < count; k++)
		sizes[k] = act[k].n, n_max = std::max(n_max, act[k].n), any_s_dev = any_s_dev || act[k].s_dev;
	RansacBatchLayout L;
	ransac_batch_layout(sizes.data(), count, params->max_iter_num, &L);
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, (size_t)L.dev_bytes))
		return rc;
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, (size_t)L.pin_bytes, hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	const RansacBatchDesc *d_desc = reinterpret_cast<const RansacBatchDesc *>(d + L.o_desc);
	auto put_desc = [&]() { // (the pinned copy is rewritten only behind a synchronisation)
		std::memcpy(h + L.p_desc, L.desc.data(), sizeof(RansacBatchDesc) * count);
		return hipMemcpyAsync(d + L.o_desc, h + L.p_desc, sizeof(RansacBatchDesc) * count, hipMemcpyHostToDevice, st);
	};
	const int min_in = params->min_inlier_num;

	// staging; with a device-resident source the points come down again in one copy, for the draws
	std::vector<PairStageItem> items(count);
	for (uint32_t k = 0; k < count; k++)
	{
		const mulls_ransac_problem &P = problems[act[k].index];
		const RansacBatchDesc &D = L.desc[k];
		items[k] = PairStageItem{&P.tgt, &P.src, P.tgt_idx, P.src_idx, D.n, act[k].indexed, act[k].t_dev, act[k].s_dev, D.src, D.tgt, D.idx};
	}
	if (int rc = stage_pairs(ctx, st, d, h, PairStagePlaces{L.o_pts, L.pts_bytes, L.o_idx, L.idx_bytes, L.o_gather, L.p_pts, L.p_idx, L.p_gather}, items.data(), count))
		return rc;
	if (any_s_dev)
	{
		HIPCHK(ctx, hipMemcpyAsync(h + L.p_pts, d + L.o_pts, L.pts_bytes, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}

	// the samples of every iteration the sequential loops can reach: the problems side by side, each draw sequential inside
	const uint32_t n_hyp_cap = ransac_batch_hypotheses(params->max_iter_num);
	std::vector<std::vector<int32_t>> triples(count);
	auto draw = [&](long k) {
		draw_triples(reinterpret_cast<const float *>(h + L.p_pts + (L.desc[k].src - L.o_pts)), L.desc[k].n, n_hyp_cap, triples[k]);
		if (!triples[k].empty())
			std::memcpy(h + L.p_tri + (L.desc[k].tri - L.o_tri), triples[k].data(), triples[k].size() * 4u);
	};
	if (count > 1u)
		shared_host_pool().parallel_for(0, (long)count, 1, draw);
	else
		draw(0);
	uint32_t n_hyp_max = 0;
	for (uint32_t k = 0; k < count; k++)
	{
		L.desc[k].n_hyp = (uint32_t)(triples[k].size() / 3u);
		n_hyp_max = std::max(n_hyp_max, L.desc[k].n_hyp);
		if (!L.desc[k].n_hyp) // no good sample for the first iteration: computeModel fails
		{
			const mulls_ransac_problem &P = problems[act[k].index];
			pass_through(L.desc[k].n, min_in, &results[act[k].index], P.inliers, P.inlier_cap);
		}
	}
	if (!n_hyp_max)
		return MULLS_OK; // every problem passes through: nothing to launch
	triples.clear();

	// models and counts of every hypothesis of every problem, then PCL's sequential rule per problem
	const double nb = (double)params->noise_bound, thr_sqr = nb * nb;
	HIPCHK(ctx, hipMemcpyAsync(d + L.o_tri, h + L.p_tri, L.tri_bytes, hipMemcpyHostToDevice, st));
	HIPCHK(ctx, put_desc());
	HIPCHK(ctx, launch_ransac_batch_models(st, d_desc, count, n_hyp_max, d));
	HIPCHK(ctx, launch_ransac_batch_score(st, d_desc, count, n_hyp_max, d, thr_sqr));
	HIPCHK(ctx, hipMemcpyAsync(h + L.p_counts, d + L.o_counts, L.counts_bytes, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	for (uint32_t k = 0; k < count; k++)
	{
		RansacBatchDesc &D = L.desc[k];
		if (!D.n_hyp)
			continue;
		mulls_ransac_result *result = &results[act[k].index];
		int iterations = 0, best_it = -1;
		ransac_sequential_rule(reinterpret_cast<const uint32_t *>(h + L.p_counts + (D.counts - L.o_counts)), D.n_hyp, D.n, params->max_iter_num, &iterations, &best_it);
		result->iterations = iterations;
		result->best_iteration = best_it;
		D.best = best_it;
	}

	// the winners' inliers
	RansacRound *d_win = reinterpret_cast<RansacRound *>(d + L.o_win);
	HIPCHK(ctx, put_desc());
	HIPCHK(ctx, hipMemsetAsync(d_win, 0, sizeof(RansacRound) * count, st));
	HIPCHK(ctx, launch_ransac_batch_select(st, d_desc, count, n_max, d, thr_sqr, d_win));
	HIPCHK(ctx, hipMemcpyAsync(h + L.p_win, d_win, sizeof(RansacRound) * count, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::vector<RansacModel> best_model(count);
	std::vector<uint32_t> n_in(count, 0u);
	std::vector<int> final_mask(count, 0);
	std::vector<char> live(count); // the problem still has a model: no pass-through, no failed refinement
	for (uint32_t k = 0; k < count; k++)
	{
		RansacRound W;
		std::memcpy(&W, h + L.p_win + sizeof(RansacRound) * k, sizeof(W));
		best_model[k] = W.T, n_in[k] = W.n_new, live[k] = L.desc[k].n_hyp != 0u;
	}

	if (params->refine)
	{
		// RandomSampleConsensus::refineModel(3.0, 1000) (sac.h) in lock step: one RefineState (ransac_host.h) per problem, one launch per round with one
		// workgroup per problem that still refines.  A problem that has ended has no job any more: its masks and its round record stay as they are.
		std::vector<RefineState> state(count);
		std::vector<uint32_t> active;
		for (uint32_t k = 0; k < count; k++)
			if (live[k])
			{
				refine_begin(state[k], nb, n_in[k]);
				active.push_back(k);
			}
		RansacBatchJob *jobs = reinterpret_cast<RansacBatchJob *>(h + L.p_jobs);
		while (!active.empty())
		{
			for (size_t j = 0; j < active.size(); j++)
			{
				const RefineState &s = state[active[j]];
				jobs[j] = RansacBatchJob{active[j], (uint32_t)s.prev, (uint32_t)s.next, 0u, refine_threshold(s)};
			}
			HIPCHK(ctx, hipMemcpyAsync(d + L.o_jobs, jobs, sizeof(RansacBatchJob) * active.size(), hipMemcpyHostToDevice, st));
			HIPCHK(ctx, launch_ransac_batch_refine(st, d_desc, reinterpret_cast<const RansacBatchJob *>(d + L.o_jobs), (uint32_t)active.size(), d));
			HIPCHK(ctx, hipMemcpyAsync(h + L.p_round, d + L.o_round, L.round_bytes, hipMemcpyDeviceToHost, st));
			HIPCHK(ctx, hipStreamSynchronize(st));
			size_t kept = 0;
			for (size_t j = 0; j < active.size(); j++)
			{
				const uint32_t k = active[j];
				RansacRound R;
				std::memcpy(&R, h + L.p_round + (L.desc[k].round - L.o_round), sizeof(R));
				RefineStep step;
				step.n_new = R.n_new, step.changed = R.changed != 0, step.median = R.median;
				if (refine_feed(state[k], step))
				{
					active[kept++] = k;
					continue;
				}
				const RefineOutcome &ro = state[k].o;
				mulls_ransac_result *result = &results[act[k].index];
				result->refine_iterations = ro.rounds;
				if (ro.failed)
				{
					// "Refinement failed": getRemainingCorrespondences returns with nothing
					result->n_inliers = 0;
					result->status = -1;
					live[k] = 0;
				}
				else if (!ro.oscillating) // (an oscillation returns true without installing anything: the unrefined model and its inliers stay)
				{
					best_model[k] = R.T;
					n_in[k] = ro.n_inliers;
					final_mask[k] = ro.final_mask;
				}
			}
			active.resize(kept);
		}
	}

	// the final masks, down in one copy, compacted into the callers' lists
	bool any_mask = false;
	for (uint32_t k = 0; k < count; k++)
		if (live[k])
		{
			if (n_in[k] < 3u)
			{
				const mulls_ransac_problem &P = problems[act[k].index];
				pass_through(L.desc[k].n, min_in, &results[act[k].index], P.inliers, P.inlier_cap);
				live[k] = 0;
			}
			else
				any_mask = true;
		}
	if (!any_mask)
		return MULLS_OK;
	HIPCHK(ctx, hipMemcpyAsync(h + L.p_mask, d + L.o_mask, L.mask_bytes, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	for (uint32_t k = 0; k < count; k++)
		if (live[k])
		{
			const RansacBatchDesc &D = L.desc[k];
			const mulls_ransac_problem &P = problems[act[k].index];
			finish_inliers(h + L.p_mask + (D.mask - L.o_mask) + (size_t)final_mask[k] * D.mask_stride, D.n, min_in, best_model[k], &results[act[k].index], P.inliers,
						   P.inlier_cap);
		}
	return MULLS_OK;
}

int ransac_batch_run(mulls_ctx *ctx, const mulls_ransac_problem *problems, uint32_t n_problems, const mulls_ransac_params *params, uint64_t limit,
					 mulls_ransac_result *results)
{
	if (!ctx || !params || (n_problems && (!problems || !results)))
		return MULLS_E_INVALID;
	for (uint32_t b = 0; b < n_problems; b++)
		reset_result(&results[b]);
	if (!n_problems)
		return MULLS_OK;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	// every problem is checked before any device work and before any result is written: the first refusal found ends the call
	std::vector<BatchProblem> act;
	std::vector<BatchProblem> few; // below three pairs: pass-through
	for (uint32_t b = 0; b < n_problems; b++)
	{
		const mulls_ransac_problem &P = problems[b];
		const Refusal refuse{ctx, "mulls_coarse_reg_ransac_batch", b};
		BatchProblem A;
		bool runs;
		A.index = b;
		if (int rc = check_pairs(refuse, P, P.tgt_idx || P.src_idx, params, &A, &runs))
			return rc;
		if (!runs)
		{
			few.push_back(A);
			continue;
		}
		if (int rc = check_strides(refuse, P.tgt, P.src, &A))
			return rc;
		act.push_back(A);
	}
	for (const BatchProblem &A : few)
		pass_through(A.n, params->min_inlier_num, &results[A.index], problems[A.index].inliers, problems[A.index].inlier_cap);
	if (act.empty())
		return MULLS_OK;
	if (!ctx->ransac)
		ctx->ransac = new mulls_ransac_scratch();
	if (!limit)
		limit = MULLS_RANSAC_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<uint64_t> bytes(act.size());
	for (size_t k = 0; k < act.size(); k++)
		bytes[k] = ransac_batch_problem_bytes(act[k].n, params->max_iter_num);
	std::vector<uint32_t> cuts;
	ransac_batch_cuts(bytes.data(), (uint32_t)act.size(), limit, &cuts);
	for (size_t c = 0; c + 1 < cuts.size(); c++)
		if (int rc = ransac_sub_batch(ctx, problems, &act[cuts[c]], cuts[c + 1] - cuts[c], params, results))
		{
			for (uint32_t b = 0; b < n_problems; b++)
				reset_result(&results[b]);
			return rc;
		}
	return MULLS_OK;
}

} // namespace

extern "C"
{
	void mulls_ransac_default_params(mulls_ransac_params *p)
	{
		if (!p)
			return;
		p->noise_bound = 0.2f; // cregistration.hpp:607
		p->min_inlier_num = 8;
		p->max_iter_num = 20000;
		p->refine = 1; // :618
	}

	int mulls_coarse_reg_ransac(mulls_ctx *ctx, const mulls_cloud *tgt_pts, const mulls_cloud *src_pts, const mulls_ransac_params *params,
								mulls_ransac_result *result, int32_t *inliers, uint32_t cap)
	try
	{
		return ransac_run(ctx, tgt_pts, src_pts, nullptr, nullptr, 0, false, params, result, inliers, cap);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_coarse_reg_ransac_indexed(mulls_ctx *ctx, const mulls_cloud *tgt_kpts, const mulls_cloud *src_kpts, const int32_t *tgt_idx, const int32_t *src_idx,
										uint32_t n_corr, const mulls_ransac_params *params, mulls_ransac_result *result, int32_t *inliers, uint32_t cap)
	try
	{
		return ransac_run(ctx, tgt_kpts, src_kpts, tgt_idx, src_idx, n_corr, true, params, result, inliers, cap);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	int mulls_coarse_reg_ransac_batch(mulls_ctx *ctx, const mulls_ransac_problem *problems, uint32_t n_problems, const mulls_ransac_params *params,
									  uint64_t scratch_limit_bytes, mulls_ransac_result *results)
	try
	{
		return ransac_batch_run(ctx, problems, n_problems, params, scratch_limit_bytes, results);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}
}
