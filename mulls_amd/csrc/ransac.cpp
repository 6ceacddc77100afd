// ransac.cpp — mulls_coarse_reg_ransac: CRegistration<PointT>::coarse_reg_ransac (cregistration.hpp:605-661), the solver between the key-point matcher
// (ncc.cpp) and mulls_icp, on the device (k_ransac.hip).  Host side: argument checks, staging, PCL's sample sequence (sequential and cheap: a Mersenne
// twister and three swaps per hypothesis), PCL's sequential "first best wins, stop at k" rule applied to the counts the device returns for every
// hypothesis, and the control flow of refineModel around one launch per round.  include/mulls_hip.h has the definition this file follows.
// mulls_coarse_reg_ransac_batch runs the same steps for many problems in lock step: ransac_batch.h plans a sub-batch's arena, the k_rb_* kernels of
// k_ransac.hip run each step for all its problems in one launch, and the refinement keeps one resumable control state (ransac_host.h) per problem.  The
// three entry points share one argument checker, pass_through and finish_inliers.
#include "ctx.h"
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
bool cloud_on_device(mulls_ctx *ctx, const mulls_cloud &c)
{
	if (mulls_is_map_memory(ctx, c.pts, (size_t)c.n * MULLS_POINT_BYTES))
		return true;
	hipPointerAttribute_t at;
	std::memset(&at, 0, sizeof(at));
	if (hipPointerGetAttributes(&at, c.pts) == hipSuccess)
		return at.type == hipMemoryTypeDevice;
	(void)hipGetLastError(); // (an ordinary host pointer: the query reports an error on some runtimes — cleared)
	return false;
}

// x, y, z, data[3] of the n pairs' points out of a host cloud
void pack_xyzw(const mulls_cloud &c, const int32_t *idx, uint32_t n, float *out)
{
	const unsigned char *p = static_cast<const unsigned char *>(c.pts);
	for (uint32_t i = 0; i < n; i++, out += 4)
		std::memcpy(out, p + (size_t)(idx ? (uint32_t)idx[i] : i) * c.stride, 16);
}

void identity16(double T[16])
{
	for (int k = 0; k < 16; k++)
		T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

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

struct BatchProblem // a problem that reaches the device
{
	uint32_t index, n;
	bool indexed, t_dev, s_dev;
};

// who refuses: the entry point's name and, in a batch, the problem's index — mulls_last_error reads "<entry point>: [problem <b>: ]<why>"
struct Refusal
{
	mulls_ctx *ctx;
	const char *who;
	int64_t problem; // -1: a single call

	int operator()(int code, const char *why) const
	{
		ctx->err = std::string(who) + (problem >= 0 ? ": problem " + std::to_string(problem) : std::string()) + ": " + why;
		return code;
	}
	// a refusal the single calls make without a message
	int quiet(int code, const char *why) const { return problem >= 0 ? (*this)(code, why) : code; }
};

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

// ... and once the device is set, for a problem that runs: where its clouds lie, and their strides
int check_strides(const Refusal &refuse, const mulls_ransac_problem &P, BatchProblem *A)
{
	const mulls_cloud &T = P.tgt, &S = P.src;
	A->t_dev = cloud_on_device(refuse.ctx, T), A->s_dev = cloud_on_device(refuse.ctx, S);
	if ((A->t_dev && T.stride != MULLS_POINT_BYTES) || (A->s_dev && S.stride != MULLS_POINT_BYTES) || (!A->t_dev && (T.stride < 16u || T.stride % 4u)) ||
		(!A->s_dev && (S.stride < 16u || S.stride % 4u)))
		return refuse(MULLS_E_INVALID, "stride (device clouds: 48; host clouds: a multiple of 4, at least 16)");
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
	const mulls_cloud &T = P.tgt, &S = P.src;
	const uint32_t n = A.n;
	const int min_in = params->min_inlier_num;
	if (!runs)
	{
		pass_through(n, min_in, result, inliers, cap);
		return MULLS_OK;
	}

	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (int rc = check_strides(refuse, P, &A))
		return rc;
	const bool t_dev = A.t_dev, s_dev = A.s_dev;
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
	const size_t o_idx = take((size_t)n * 8u);
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
	const size_t p_src = ptake((size_t)n * 16u), p_tgt = ptake((size_t)n * 16u), p_idx = ptake((size_t)n * 8u), p_tri = ptake((size_t)n_hyp_max * 12u);
	const size_t p_counts = ptake((size_t)n_hyp_max * 4u), p_mask = ptake(n), p_round = ptake(sizeof(RansacRound)), p_model = ptake(sizeof(RansacModel)), p_cnt = ptake(4);
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, poff, hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	float4 *src4 = reinterpret_cast<float4 *>(d + o_src), *tgt4 = reinterpret_cast<float4 *>(d + o_tgt);
	float *h_src = reinterpret_cast<float *>(h + p_src);

	// staging: host clouds are packed (and gathered) on the host and go up; device clouds are gathered on the device, the source's floats come down for the draws
	if (indexed && (t_dev || s_dev))
	{
		std::memcpy(h + p_idx, tgt_idx, (size_t)n * 4u);
		std::memcpy(h + p_idx + (size_t)n * 4u, src_idx, (size_t)n * 4u);
		HIPCHK(ctx, hipMemcpyAsync(d + o_idx, h + p_idx, (size_t)n * 8u, hipMemcpyHostToDevice, st));
	}
	const int32_t *d_tidx = indexed ? reinterpret_cast<const int32_t *>(d + o_idx) : nullptr, *d_sidx = indexed ? d_tidx + n : nullptr;
	if (t_dev)
		HIPCHK(ctx, launch_ransac_gather(st, T.pts, d_tidx, n, tgt4));
	else
	{
		pack_xyzw(T, indexed ? tgt_idx : nullptr, n, reinterpret_cast<float *>(h + p_tgt));
		HIPCHK(ctx, hipMemcpyAsync(tgt4, h + p_tgt, (size_t)n * 16u, hipMemcpyHostToDevice, st));
	}
	if (s_dev)
	{
		HIPCHK(ctx, launch_ransac_gather(st, S.pts, d_sidx, n, src4));
		HIPCHK(ctx, hipMemcpyAsync(h_src, src4, (size_t)n * 16u, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	else
	{
		pack_xyzw(S, indexed ? src_idx : nullptr, n, h_src);
		HIPCHK(ctx, hipMemcpyAsync(src4, h_src, (size_t)n * 16u, hipMemcpyHostToDevice, st));
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
const char *const BATCH = "mulls_coarse_reg_ransac_batch";

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

	// staging: the host clouds packed into the pinned mirror of the points and up in one copy; device clouds gathered by one launch; with a device-resident
	// source the points come down again in one copy, for the draws
	RansacBatchGather *gathers = reinterpret_cast<RansacBatchGather *>(h + L.p_gather);
	uint32_t n_gathers = 0;
	bool any_host = false, any_idx = false;
	for (uint32_t k = 0; k < count; k++)
	{
		const mulls_ransac_problem &P = problems[act[k].index];
		const RansacBatchDesc &D = L.desc[k];
		const uint32_t n = D.n;
		int32_t *h_idx = reinterpret_cast<int32_t *>(h + L.p_idx + (D.idx - L.o_idx));
		if (act[k].indexed && (act[k].t_dev || act[k].s_dev))
		{
			std::memcpy(h_idx, P.tgt_idx, (size_t)n * 4u);
			std::memcpy(h_idx + n, P.src_idx, (size_t)n * 4u);
			any_idx = true;
		}
		if (act[k].t_dev)
			gathers[n_gathers++] = RansacBatchGather{static_cast<const unsigned char *>(P.tgt.pts), D.idx, D.tgt, n, act[k].indexed ? 1u : 0u};
		else
			pack_xyzw(P.tgt, act[k].indexed ? P.tgt_idx : nullptr, n, reinterpret_cast<float *>(h + L.p_pts + (D.tgt - L.o_pts))), any_host = true;
		if (act[k].s_dev)
			gathers[n_gathers++] = RansacBatchGather{static_cast<const unsigned char *>(P.src.pts), D.idx + (uint64_t)n * 4u, D.src, n, act[k].indexed ? 1u : 0u};
		else
			pack_xyzw(P.src, act[k].indexed ? P.src_idx : nullptr, n, reinterpret_cast<float *>(h + L.p_pts + (D.src - L.o_pts))), any_host = true;
	}
	if (any_host) // (the places of device-resident clouds go up as they are and are gathered over below)
		HIPCHK(ctx, hipMemcpyAsync(d + L.o_pts, h + L.p_pts, L.pts_bytes, hipMemcpyHostToDevice, st));
	if (any_idx)
		HIPCHK(ctx, hipMemcpyAsync(d + L.o_idx, h + L.p_idx, L.idx_bytes, hipMemcpyHostToDevice, st));
	if (n_gathers)
	{
		HIPCHK(ctx, hipMemcpyAsync(d + L.o_gather, gathers, sizeof(RansacBatchGather) * n_gathers, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, launch_ransac_batch_gather(st, reinterpret_cast<const RansacBatchGather *>(d + L.o_gather), n_gathers, n_max, d));
	}
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
		const Refusal refuse{ctx, BATCH, b};
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
		if (int rc = check_strides(refuse, P, &A))
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
