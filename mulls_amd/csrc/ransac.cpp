// ransac.cpp — mulls_coarse_reg_ransac: CRegistration<PointT>::coarse_reg_ransac (cregistration.hpp:605-661), the solver between the key-point matcher
// (ncc.cpp) and mulls_icp, on the device (k_ransac.hip).  Host side: argument checks, staging, PCL's sample sequence (sequential and cheap: a Mersenne
// twister and three swaps per hypothesis), PCL's sequential "first best wins, stop at k" rule applied to the counts the device returns for every
// hypothesis, and the control flow of refineModel around one launch per round.  include/mulls_hip.h has the definition this file follows.
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
size_t up256(size_t v) { return (v + 255u) & ~(size_t)255u; }

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

int ransac_run(mulls_ctx *ctx, const mulls_cloud *tgt_in, const mulls_cloud *src_in, const int32_t *tgt_idx, const int32_t *src_idx, uint32_t n_corr,
			   bool indexed, const mulls_ransac_params *params, mulls_ransac_result *result, int32_t *inliers, uint32_t cap)
{
	const char *who = indexed ? "mulls_coarse_reg_ransac_indexed" : "mulls_coarse_reg_ransac";
	if (!ctx || !tgt_in || !src_in || !params || !result || (cap && !inliers))
		return MULLS_E_INVALID;
	std::memset(result, 0, sizeof(*result));
	result->status = -1;
	result->best_iteration = -1;
	identity16(result->T);
	const mulls_cloud T = *tgt_in, S = *src_in;
	if ((T.n && !T.pts) || (S.n && !S.pts))
		return MULLS_E_INVALID;
	if (!std::isfinite(params->noise_bound))
	{
		ctx->err = std::string(who) + ": noise_bound is not finite";
		return MULLS_E_INVALID;
	}
	uint32_t n = T.n;
	if (indexed)
	{
		if (n_corr && (!tgt_idx || !src_idx))
			return MULLS_E_INVALID;
		n = n_corr;
	}
	else if (T.n != S.n)
	{
		ctx->err = std::string(who) + ": the clouds' sizes differ (correspondence i pairs point i of each)";
		return MULLS_E_INVALID;
	}
	if (n > MULLS_RANSAC_MAX_POINTS || params->max_iter_num > MULLS_RANSAC_MAX_ITER)
	{
		ctx->err = std::string(who) + ": at most 65536 pairs and max_iter_num <= 2^20";
		return MULLS_E_UNSUPPORTED;
	}
	if (indexed)
		for (uint32_t i = 0; i < n; i++)
			if (tgt_idx[i] < 0 || (uint32_t)tgt_idx[i] >= T.n || src_idx[i] < 0 || (uint32_t)src_idx[i] >= S.n)
			{
				ctx->err = std::string(who) + ": an index lies outside its cloud";
				return MULLS_E_INVALID;
			}
	const int min_in = params->min_inlier_num;
	// every correspondence passes, T = identity: PCL's outcome when no model is found, or when the model has fewer than three inliers
	auto pass_through = [&]() {
		result->n_inliers = n;
		for (uint32_t i = 0; i < std::min(n, cap); i++)
			inliers[i] = (int32_t)i;
		identity16(result->T);
		result->status = (long)n >= 2 * (long)min_in ? 1 : ((long)n >= (long)min_in ? 0 : -1);
		return MULLS_OK;
	};
	if (n < 3u) // getSamples: "Can not select 3 unique points out of n"
		return pass_through();

	HIPCHK(ctx, hipSetDevice(ctx->device));
	const bool t_dev = cloud_on_device(ctx, T), s_dev = cloud_on_device(ctx, S);
	if ((t_dev && T.stride != MULLS_POINT_BYTES) || (s_dev && S.stride != MULLS_POINT_BYTES) || (!t_dev && (T.stride < 16u || T.stride % 4u)) ||
		(!s_dev && (S.stride < 16u || S.stride % 4u)))
	{
		ctx->err = std::string(who) + ": stride (device clouds: 48; host clouds: a multiple of 4, at least 16)";
		return MULLS_E_INVALID;
	}
	if (!ctx->ransac)
		ctx->ransac = new mulls_ransac_scratch();
	mulls_ransac_scratch &sc = *ctx->ransac;
	const uint32_t n_hyp_max = (uint32_t)std::max(params->max_iter_num, 0) + 1u; // iteration max_iter_num is still evaluated: the loop ends on ++iterations > max

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
		return pass_through();
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
		return pass_through();
	HIPCHK(ctx, hipMemcpyAsync(h + p_mask, mask[final_mask], n, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	const uint8_t *hm = h + p_mask;
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
}
