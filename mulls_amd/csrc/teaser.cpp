// teaser.cpp — mulls_coarse_reg_teaser: CRegistration<PointT>::coarse_reg_teaser (cregistration.hpp:664-759), the solver every shipped configuration
// selects between the key-point matcher (ncc.cpp) and mulls_icp.  Host side: argument checks (one checker for the three entry points), staging, the order of
// the device steps (k_teaser.hip: graph, core numbers, greedy lower bound, compaction, GNC-TLS rotation), the exact clique search — on the one sub-matrix that
// comes down (teaser_host.h) or, with MULLS_OPT_TEASER_DEVICE_SEARCH, as a chain of bounded launches on the sub-matrix where it lies (teaser_search.h,
// k_teaser_clique.hip) — and the serial TLS translation estimate on the clique's points.  include/mulls_hip.h has the definition this file follows.
// mulls_coarse_reg_teaser_batch runs the same steps for many problems: the device steps per sub-batch (teaser_batch.h plans them, the k_tb_* kernels of
// k_teaser.hip run them, the GNC loop in lock-step), the search and the translation per problem with the code of the single call.
// WHY THE HOST SEQUENCE IS WRITTEN TWICE (teaser_run, teaser_sub_batch): a single call run as a batch of one was built and measured against teaser_run on one
// MI355X and was 1.2 to 2.1 % slower on every launch-bound row (profiles/teaser_kernel_stats.txt, section 5).  The cause was not isolated.  Supposed: the kernels of a
// sub-batch read their pointers and sizes from a descriptor in device memory before their own data, in a GNC loop of 22 to 42 iterations of five launches;
// the batch path's descriptor uploads, its memset and its planner vectors may have a share.
// So teaser_run keeps launch arguments; what the two share is one kernel text (the __device__ steps of k_teaser.hip), the argument checker, the staging of
// the pairs (pair_stage.h, shared with ransac.cpp: teaser_run stages a list of one), the searches and teaser_finish.
#include <chrono>

#include "pair_stage.h"
#include "teaser_host.h"
#include "teaser_launch.h"

// a context's scratch of this entry point: a device arena, the GNC weights (up to C (C - 1) / 2 doubles), a pinned host buffer and the device clique
// search's workers (states, cliques so far, stacks: sized once the kept vertices and the largest core number are known), grow-only
struct mulls_teaser_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr, *search = nullptr;
	double *weights = nullptr;
	size_t dev_cap = 0, pin_cap = 0, weights_cap = 0, search_cap = 0;
};

void mulls_teaser_release(mulls_ctx *ctx)
{
	if (!ctx->teaser)
		return;
	staggered_free(ctx->teaser->dev);
	staggered_free(ctx->teaser->weights);
	staggered_free(ctx->teaser->search);
	if (ctx->teaser->pin)
		(void)hipHostFree(ctx->teaser->pin);
	delete ctx->teaser;
	ctx->teaser = nullptr;
}

namespace
{
// The executor of teaser_search_control on the device: one k_teaser_clique launch and one readback of the shared words per step.  Every word a phase reads
// is written at its beginning (the shared words and the workers' states; stacks and cliques are written before they are read), so nothing of an earlier
// call or phase is seen.
struct DeviceSearch
{
	mulls_ctx *ctx;
	hipStream_t st;
	TeaserSearchArgs A;
	TeaserSearchCtl *h_ctl;			   // pinned: [0] goes up, [1] comes down
	TeaserWorkerState *h_init, *h_back; // pinned, A.workers each
	uint32_t *h_list, *d_list;		   // m + 1 words each
	uint32_t witness_at;

	int begin(int phase, uint32_t bound)
	{
		A.phase = (uint32_t)phase, A.omega = bound;
		std::memset(&h_ctl[0], 0, sizeof(TeaserSearchCtl));
		h_ctl[0].bound = bound, h_ctl[0].best_rank = MULLS_TEASER_NO_RANK;
		HIPCHK(ctx, hipMemcpyAsync(A.ctl, &h_ctl[0], sizeof(TeaserSearchCtl), hipMemcpyHostToDevice, st));
		HIPCHK(ctx, hipMemcpyAsync(A.state, h_init, (size_t)A.workers * sizeof(TeaserWorkerState), hipMemcpyHostToDevice, st));
		return MULLS_OK;
	}
	int launch(TeaserSearchCtl *out)
	{
		HIPCHK(ctx, launch_teaser_clique(st, A));
		HIPCHK(ctx, hipMemcpyAsync(&h_ctl[1], A.ctl, sizeof(TeaserSearchCtl), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		*out = h_ctl[1];
		return MULLS_OK;
	}
	int clique(uint32_t rank, std::vector<uint32_t> *out)
	{
		HIPCHK(ctx, hipMemcpyAsync(h_back, A.state, (size_t)A.workers * sizeof(TeaserWorkerState), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		for (uint32_t w = 0; w < A.workers; w++)
			if (h_back[w].found == rank)
			{
				HIPCHK(ctx, hipMemcpyAsync(h_list, A.cur + (size_t)w * A.levels, (size_t)A.omega * 4u, hipMemcpyDeviceToHost, st)); // (omega < levels)
				HIPCHK(ctx, hipStreamSynchronize(st));
				out->assign(h_list, h_list + A.omega);
				return MULLS_OK;
			}
		return MULLS_TEASER_SEARCH_FAILED;
	}
	int witness(std::vector<uint32_t> *out)
	{
		HIPCHK(ctx, launch_teaser_witness(st, A.sub, A.m, witness_at, d_list));
		HIPCHK(ctx, hipMemcpyAsync(h_list, d_list, ((size_t)A.m + 1u) * 4u, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		if (!h_list[0] || h_list[0] > A.m)
			return MULLS_TEASER_SEARCH_FAILED;
		out->assign(h_list + 1, h_list + 1 + h_list[0]);
		std::sort(out->begin(), out->end());
		return MULLS_OK;
	}
};

// what the device clique search uses besides the workers' scratch: words per kept vertex and the control records, on the device and pinned
struct DeviceSearchBuffers
{
	uint32_t *later, *first; // m and m + 1 words
	TeaserSearchCtl *ctl;
	uint32_t *list; // m + 1 words
	uint32_t *h_later; // m + 1 words
	TeaserSearchCtl *h_ctl; // two
	uint32_t *h_list;
	TeaserWorkerState *h_init, *h_back; // MULLS_TEASER_SEARCH_WORKERS each
};

// the exact search on the device, on the m x ceil(m / 64) sub-matrix where it lies; clique: original vertex numbers (h_keep maps the kept ones back)
int device_clique_search(mulls_ctx *ctx, mulls_teaser_scratch &sc, hipStream_t st, const char *who, const uint64_t *sub, uint32_t m, uint32_t lb, uint32_t max_core,
						 uint32_t witness_at, uint64_t node_budget, const DeviceSearchBuffers &B, const int32_t *h_keep, mulls_teaser_result *result,
						 std::vector<uint32_t> *clique_out)
{
	std::vector<uint32_t> &clique = *clique_out;
	const uint32_t Wm = (m + 63u) / 64u;
	// the sub-matrix stays where it is: the plan needs one count per kept vertex, the control a few words per launch
	const auto tic = std::chrono::steady_clock::now();
	uint32_t *later = B.later, *h_later = B.h_later;
	HIPCHK(ctx, launch_teaser_later(st, sub, m, later));
	HIPCHK(ctx, hipMemcpyAsync(h_later, later, (size_t)m * 4u, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	TeaserPlan plan;
	teaser_plan(h_later, m, lb, max_core, plan);
	DeviceSearch ex;
	ex.ctx = ctx, ex.st = st, ex.witness_at = witness_at;
	TeaserSearchArgs &A = ex.A;
	A.sub = sub, A.first = B.first;
	A.m = m, A.W = Wm, A.n_tasks = plan.n_tasks, A.levels = plan.levels;
	A.phase = 0, A.omega = lb, A.quota = MULLS_TEASER_SEARCH_QUOTA, A.workers = teaser_plan_workers(plan);
	size_t soff = 0;
	auto stake = [&](size_t bytes) {
		const size_t at = soff;
		soff += up256(bytes);
		return at;
	};
	const size_t s_state = stake((size_t)A.workers * sizeof(TeaserWorkerState)), s_cur = stake((size_t)A.workers * A.levels * 4u);
	const size_t s_slab = stake((size_t)A.workers * A.levels * Wm * 8u);
	if (int rc = grow(ctx, &sc.search, &sc.search_cap, soff))
		return rc;
	A.ctl = B.ctl;
	A.state = reinterpret_cast<TeaserWorkerState *>(sc.search + s_state);
	A.cur = reinterpret_cast<uint32_t *>(sc.search + s_cur), A.slab = reinterpret_cast<uint64_t *>(sc.search + s_slab);
	ex.h_ctl = B.h_ctl;
	ex.h_init = B.h_init, ex.h_back = B.h_back;
	ex.h_list = B.h_list, ex.d_list = B.list;
	for (uint32_t w = 0; w < A.workers; w++)
		ex.h_init[w] = TeaserWorkerState{0, 0, 0, 0, MULLS_TEASER_NO_RANK, {0, 0, 0}};
	std::memcpy(h_later, plan.first.data(), ((size_t)m + 1u) * 4u); // (the counts are in the plan now)
	HIPCHK(ctx, hipMemcpyAsync(B.first, h_later, ((size_t)m + 1u) * 4u, hipMemcpyHostToDevice, st));
	TeaserSearchOutcome found;
	if (int rc = teaser_search_control(ex, plan, max_core, node_budget, found))
	{
		if (rc != MULLS_TEASER_SEARCH_FAILED)
			return rc;
		ctx->err = std::string(who) + ": the device clique search left the states its plan allows";
		return MULLS_E_HIP;
	}
	result->search_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tic).count();
	result->clique_nodes = found.nodes;
	result->clique_exact = found.exact ? 1 : 0;
	if (found.clique.size() != (found.exact ? found.omega : lb))
	{
		ctx->err = std::string(who) + ": the device clique search's list does not have the size it proved";
		return MULLS_E_HIP;
	}
	for (uint32_t v : found.clique)
		clique.push_back((uint32_t)h_keep[v]);
	return MULLS_OK;
}

// the exact search on the host, on the downloaded sub-matrix
int host_clique_search(mulls_ctx *ctx, const char *who, const uint64_t *h_sub, uint32_t m, uint32_t lb, uint32_t witness_at, uint64_t node_budget,
					   const int32_t *h_keep, mulls_teaser_result *result, std::vector<uint32_t> *clique_out)
{
	std::vector<uint32_t> &clique = *clique_out;
	const uint32_t Wm = (m + 63u) / 64u;
	TeaserBits G;
	G.m = m, G.W = Wm, G.rows = h_sub;
	const auto tic = std::chrono::steady_clock::now();
	std::vector<uint32_t> witness;
	teaser_greedy_clique(G, witness_at, witness);
	if (witness.size() != lb)
	{
		ctx->err = std::string(who) + ": the greedy clique's witness does not have the size the device counted";
		return MULLS_E_HIP;
	}
	TeaserSearch search;
	search.run(G, lb, witness, node_budget);
	result->search_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tic).count();
	result->clique_nodes = search.nodes;
	result->clique_exact = search.aborted ? 0 : 1;
	for (uint32_t v : search.best_clique)
		clique.push_back((uint32_t)h_keep[v]);
	return MULLS_OK;
}

// what follows the GNC loop: the counts, the serial TLS translation on the clique's points (already down) and R, the outcome
void teaser_finish(const TeaserGnc &G, int iters, const float *h_cs, const float *h_ct, uint32_t C, double nb, const mulls_teaser_params *params,
				   mulls_teaser_result *result)
{
	const uint64_t M = (uint64_t)C * (C - 1u) / 2u;
	result->gnc_iterations = iters;
	result->cost = G.cost;
	const uint64_t n_rot = G.stop == 1u ? M : (uint64_t)G.n_inlier;
	result->n_rotation_inliers = (int32_t)n_rot;

	// the translation: serial, on the clique's points (already down) and R
	double that[3];
	result->n_translation_inliers = (int32_t)teaser_translation(h_cs, h_ct, C, G.R, nb, that);
	const long long min_in = params->min_inlier_num;
	result->status = (long long)n_rot >= 2 * min_in ? 1 : ((long long)n_rot >= min_in ? 0 : -1);
	if (result->status >= 0)
		for (int r = 0; r < 3; r++)
		{
			for (int c = 0; c < 3; c++)
				result->T[c * 4 + r] = G.R[r * 3 + c];
			result->T[12 + r] = that[r];
		}
}

void reset_result(mulls_teaser_result *result)
{
	std::memset(result, 0, sizeof(*result));
	result->status = -1;
	identity16(result->T);
}

// one mulls_teaser_params for a call
int check_params(const Refusal &refuse, const mulls_teaser_params *params)
{
	if (std::isfinite(params->noise_bound) && params->noise_bound >= 0.0f)
		return MULLS_OK;
	return refuse(MULLS_E_INVALID, "noise_bound is not finite or negative");
}

// A problem as it was handed in, before the device is touched: the refusals, upstream's early returns (*runs = false: the result stays at status -1), or
// its number of pairs.  indexed: the batch ABI infers it from the lists and wants both or none; the indexed single call says so itself and reads no list
// when n_corr = 0.
int check_pairs(const Refusal &refuse, const mulls_teaser_problem &P, bool indexed, BatchProblem *A, bool *runs)
{
	*runs = false;
	const mulls_cloud &T = P.tgt, &S = P.src;
	const bool list_missing = indexed && (!P.tgt_idx || !P.src_idx) && (refuse.problem >= 0 || P.n_corr);
	if ((T.n && !T.pts) || (S.n && !S.pts) || (P.clique_cap && !P.clique) || list_missing)
		return refuse(MULLS_E_INVALID, "a NULL cloud, clique buffer or index list");
	A->indexed = indexed, A->n = indexed ? P.n_corr : T.n;
	if (!indexed && T.n != S.n)
		return MULLS_OK; // upstream: "source points number != target points number", -1
	if (A->n <= 3u)
		return MULLS_OK; // upstream: "too few correspondences", -1
	if (A->n > MULLS_TEASER_MAX_POINTS)
		return refuse(MULLS_E_UNSUPPORTED, "at most 8192 pairs");
	if (indexed)
		for (uint32_t i = 0; i < A->n; i++)
			if (P.tgt_idx[i] < 0 || (uint32_t)P.tgt_idx[i] >= T.n || P.src_idx[i] < 0 || (uint32_t)P.src_idx[i] >= S.n)
				return refuse(MULLS_E_INVALID, "an index lies outside its cloud");
	*runs = true;
	return MULLS_OK;
}

// the device clique search's words behind an arena: taken once per call or sub-batch for its largest problem of n pairs (nothing when the host searches)
struct SearchPlaces
{
	size_t o_later, o_first, o_ctl, o_list, p_later, p_ctl, p_list, p_init, p_back;

	SearchPlaces(bool device_search, uint32_t n, size_t &off, size_t &poff) // off, poff: the arenas' ends so far, moved on
	{
		auto take = [&](size_t bytes) {
			const size_t at = off;
			off += up256(bytes);
			return at;
		};
		auto ptake = [&](size_t bytes) {
			const size_t at = poff;
			poff += up256(bytes);
			return at;
		};
		const size_t words = device_search ? ((size_t)n + 1u) * 4u : 0u, states = device_search ? MULLS_TEASER_SEARCH_WORKERS * sizeof(TeaserWorkerState) : 0u;
		o_later = take(device_search ? (size_t)n * 4u : 0u), o_first = take(words), o_ctl = take(sizeof(TeaserSearchCtl)), o_list = take(words);
		p_later = ptake(words), p_ctl = ptake(2u * sizeof(TeaserSearchCtl)), p_list = ptake(words), p_init = ptake(states), p_back = ptake(states);
	}
	DeviceSearchBuffers at(unsigned char *d, unsigned char *h) const
	{
		DeviceSearchBuffers B;
		B.later = reinterpret_cast<uint32_t *>(d + o_later), B.first = reinterpret_cast<uint32_t *>(d + o_first);
		B.ctl = reinterpret_cast<TeaserSearchCtl *>(d + o_ctl), B.list = reinterpret_cast<uint32_t *>(d + o_list);
		B.h_later = reinterpret_cast<uint32_t *>(h + p_later), B.h_ctl = reinterpret_cast<TeaserSearchCtl *>(h + p_ctl);
		B.h_list = reinterpret_cast<uint32_t *>(h + p_list);
		B.h_init = reinterpret_cast<TeaserWorkerState *>(h + p_init), B.h_back = reinterpret_cast<TeaserWorkerState *>(h + p_back);
		return B;
	}
};

int teaser_run(mulls_ctx *ctx, const char *who, bool indexed_call, const mulls_cloud *tgt_in, const mulls_cloud *src_in, const int32_t *tgt_idx,
			   const int32_t *src_idx, uint32_t n_corr, const mulls_teaser_params *params, mulls_teaser_result *result, int32_t *clique_out, uint32_t cap)
{
	if (!ctx || !tgt_in || !src_in || !params || !result || (cap && !clique_out))
		return MULLS_E_INVALID;
	reset_result(result);
	if ((tgt_in->n && !tgt_in->pts) || (src_in->n && !src_in->pts))
		return MULLS_E_INVALID;
	const Refusal refuse{ctx, who, -1};
	if (int rc = check_params(refuse, params))
		return rc;
	mulls_teaser_problem P;
	P.tgt = *tgt_in, P.src = *src_in;
	P.tgt_idx = tgt_idx, P.src_idx = src_idx, P.n_corr = n_corr;
	P.clique = clique_out, P.clique_cap = cap;
	BatchProblem A;
	bool runs;
	if (int rc = check_pairs(refuse, P, indexed_call, &A, &runs))
		return rc;
	if (!runs)
		return MULLS_OK; // upstream's early returns: -1
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (int rc = check_strides(refuse, P.tgt, P.src, &A))
		return rc;
	const uint32_t n = A.n;
	if (!ctx->teaser)
		ctx->teaser = new mulls_teaser_scratch();
	mulls_teaser_scratch &sc = *ctx->teaser;
	const uint32_t W = (n + 63u) / 64u;
	const size_t mat = (size_t)n * W * 8u;

	size_t off = 0;
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return at;
	};
	const size_t o_src = take((size_t)n * 16u), o_tgt = take((size_t)n * 16u), o_idx = take((size_t)n * 8u), o_jobs = take(2u * sizeof(PairGather)), o_adj = take(mat), o_sub = take(mat);
	const size_t o_deg = take((size_t)n * 4u), o_cg = take((size_t)n * 8u), o_sum = take(8), o_keep = take((size_t)n * 4u);
	const size_t o_cs = take((size_t)n * 16u), o_ct = take((size_t)n * 16u), o_part = take((size_t)9u * MULLS_TEASER_PARTIALS * 8u), o_S = take(sizeof(TeaserGnc));
	size_t poff = 0;
	auto ptake = [&](size_t bytes) {
		const size_t at = poff;
		poff += up256(bytes);
		return at;
	};
	const size_t p_pts = ptake(2u * up256((size_t)n * 16u)), p_idx = ptake((size_t)n * 8u), p_jobs = ptake(2u * sizeof(PairGather)), p_sub = ptake(mat);
	const size_t p_cg = ptake((size_t)n * 8u);
	const size_t p_sum = ptake(8), p_keep = ptake((size_t)n * 4u), p_cs = ptake((size_t)n * 32u), p_S = ptake(sizeof(TeaserGnc));
	const bool device_search = ctx->opt[MULLS_OPT_TEASER_DEVICE_SEARCH] != 0.0;
	const SearchPlaces search(device_search, n, off, poff);
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
		return rc;
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, poff, hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	float4 *src4 = reinterpret_cast<float4 *>(d + o_src), *tgt4 = reinterpret_cast<float4 *>(d + o_tgt);

	// staging: a list of one (the source's and the target's points lie side by side in the arena and in its mirror)
	const PairStageItem item{&P.tgt, &P.src, tgt_idx, src_idx, n, A.indexed, A.t_dev, A.s_dev, o_src, o_tgt, o_idx};
	if (int rc = stage_pairs(ctx, st, d, h, PairStagePlaces{o_src, o_idx - o_src, o_idx, o_jobs - o_idx, o_jobs, p_pts, p_idx, p_jobs}, &item, 1))
		return rc;

	// the graph, its core numbers and the greedy clique sizes
	const double nb = (double)params->noise_bound, beta = (2.0 * nb) * sqrt(1.0);
	uint64_t *adj = reinterpret_cast<uint64_t *>(d + o_adj), *sub = reinterpret_cast<uint64_t *>(d + o_sub);
	uint32_t *deg = reinterpret_cast<uint32_t *>(d + o_deg), *core = reinterpret_cast<uint32_t *>(d + o_cg), *greedy = core + n;
	HIPCHK(ctx, hipMemsetAsync(d + o_sum, 0, 8, st));
	HIPCHK(ctx, launch_teaser_graph(st, src4, tgt4, n, beta, adj));
	HIPCHK(ctx, launch_teaser_degrees(st, adj, n, deg, reinterpret_cast<unsigned long long *>(d + o_sum)));
	HIPCHK(ctx, launch_teaser_cores(st, adj, n, deg, core));
	HIPCHK(ctx, launch_teaser_greedy(st, adj, n, greedy));
	HIPCHK(ctx, hipMemcpyAsync(h + p_cg, core, (size_t)n * 8u, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipMemcpyAsync(h + p_sum, d + o_sum, 8, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	const uint32_t *h_core = reinterpret_cast<const uint32_t *>(h + p_cg), *h_greedy = h_core + n;
	unsigned long long deg_sum;
	std::memcpy(&deg_sum, h + p_sum, 8);
	result->n_edges = deg_sum / 2u;
	uint32_t max_core = 0, lb = 0, lb_v = 0;
	for (uint32_t i = 0; i < n; i++)
	{
		max_core = std::max(max_core, h_core[i]);
		if (h_greedy[i] > lb)
			lb = h_greedy[i], lb_v = i;
	}
	result->max_core = (int32_t)max_core;
	std::vector<uint32_t> clique; // original vertex numbers, ascending
	result->clique_exact = 1;
	if (lb <= 1u) // no edge: the smallest maximum clique is the vertex 0
		clique.assign(1, 0u);
	else
	{
		// the vertices a clique of lb or more can hold, in ascending order: the one sub-matrix the search needs
		int32_t *h_keep = reinterpret_cast<int32_t *>(h + p_keep);
		uint32_t m = 0, witness_at = 0;
		for (uint32_t i = 0; i < n; i++)
			if (h_core[i] + 1u >= lb)
			{
				if (i == lb_v)
					witness_at = m;
				h_keep[m++] = (int32_t)i;
			}
		const uint32_t Wm = (m + 63u) / 64u;
		HIPCHK(ctx, hipMemcpyAsync(d + o_keep, h_keep, (size_t)m * 4u, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, launch_teaser_compact(st, adj, n, reinterpret_cast<const int32_t *>(d + o_keep), m, sub));
		if (device_search)
		{
			if (int rc = device_clique_search(ctx, sc, st, who, sub, m, lb, max_core, witness_at, params->clique_node_budget, search.at(d, h), h_keep, result, &clique))
				return rc;
		}
		else
		{
			HIPCHK(ctx, hipMemcpyAsync(h + p_sub, sub, (size_t)m * Wm * 8u, hipMemcpyDeviceToHost, st));
			HIPCHK(ctx, hipStreamSynchronize(st));
			if (int rc = host_clique_search(ctx, who, reinterpret_cast<const uint64_t *>(h + p_sub), m, lb, witness_at, params->clique_node_budget, h_keep, result,
											&clique))
				return rc;
		}
	}
	const uint32_t C = (uint32_t)clique.size();
	result->clique_size = (int32_t)C;
	for (uint32_t k = 0; k < std::min(C, cap); k++)
		clique_out[k] = (int32_t)clique[k];
	if (C <= 1u)
		return MULLS_OK;

	// the rotation: GNC-TLS over the clique's pairwise measurements, one launch set and one small readback per iteration
	const uint64_t M = (uint64_t)C * (C - 1u) / 2u;
	if (int rc = grow(ctx, &sc.weights, &sc.weights_cap, (size_t)M))
		return rc;
	int32_t *h_keep = reinterpret_cast<int32_t *>(h + p_keep);
	for (uint32_t k = 0; k < C; k++)
		h_keep[k] = (int32_t)clique[k];
	float4 *cs = reinterpret_cast<float4 *>(d + o_cs), *ct = reinterpret_cast<float4 *>(d + o_ct);
	HIPCHK(ctx, hipMemcpyAsync(d + o_keep, h_keep, (size_t)C * 4u, hipMemcpyHostToDevice, st));
	HIPCHK(ctx, launch_teaser_pick(st, src4, tgt4, reinterpret_cast<const int32_t *>(d + o_keep), C, cs, ct));
	HIPCHK(ctx, hipMemcpyAsync(h + p_cs, cs, (size_t)C * 16u, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipMemcpyAsync(h + p_cs + (size_t)n * 16u, ct, (size_t)C * 16u, hipMemcpyDeviceToHost, st));
	double nb2 = nb * nb;
	if (nb2 < 1e-16)
		nb2 = 1e-2;
	TeaserGnc G;
	TeaserGnc *dS = reinterpret_cast<TeaserGnc *>(d + o_S);
	int iters = 0;
	for (int it = 0; it < MULLS_TEASER_GNC_MAX_ITER; it++)
	{
		HIPCHK(ctx, launch_teaser_gnc_iteration(st, cs, ct, C, it, nb2, sc.weights, reinterpret_cast<double *>(d + o_part), dS));
		HIPCHK(ctx, hipMemcpyAsync(h + p_S, dS, sizeof(TeaserGnc), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		std::memcpy(&G, h + p_S, sizeof(G));
		iters = it + 1;
		if (G.stop)
			break;
	}
	teaser_finish(G, iters, reinterpret_cast<const float *>(h + p_cs), reinterpret_cast<const float *>(h + p_cs + (size_t)n * 16u), C, nb, params, result);
	return MULLS_OK;
}
// ---- mulls_coarse_reg_teaser_batch
const char *const BATCH = "mulls_coarse_reg_teaser_batch";

// one graph-phase sub-batch: `count` problems whose arena fits the limit (or one that does not)
int teaser_sub_batch(mulls_ctx *ctx, const mulls_teaser_problem *problems, const BatchProblem *act, uint32_t count, const mulls_teaser_params *params,
					 uint64_t limit, mulls_teaser_result *results)
{
	mulls_teaser_scratch &sc = *ctx->teaser;
	const bool device_search = ctx->opt[MULLS_OPT_TEASER_DEVICE_SEARCH] != 0.0;
	std::vector<uint32_t> sizes(count);
	uint32_t n_max = 0;
	for (uint32_t k = 0; k < count; k++)
		sizes[k] = act[k].n, n_max = std::max(n_max, act[k].n);
	TeaserBatchLayout L;
	teaser_batch_layout(sizes.data(), count, &L);
	// behind the arena: what the device search needs besides its workers, once for the sub-batch (the problems are searched one after another)
	size_t off = L.dev_bytes, poff = L.pin_bytes;
	const SearchPlaces search(device_search, n_max, off, poff);
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
		return rc;
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, poff, hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	const TeaserBatchDesc *d_desc = reinterpret_cast<const TeaserBatchDesc *>(d + L.o_desc);
	auto put_desc = [&]() { // (the pinned copy is rewritten only behind a synchronisation)
		std::memcpy(h + L.p_desc, L.desc.data(), sizeof(TeaserBatchDesc) * count);
		return hipMemcpyAsync(d + L.o_desc, h + L.p_desc, sizeof(TeaserBatchDesc) * count, hipMemcpyHostToDevice, st);
	};

	// staging
	std::vector<PairStageItem> items(count);
	for (uint32_t k = 0; k < count; k++)
	{
		const mulls_teaser_problem &P = problems[act[k].index];
		const TeaserBatchDesc &D = L.desc[k];
		items[k] = PairStageItem{&P.tgt, &P.src, P.tgt_idx, P.src_idx, D.n, act[k].indexed, act[k].t_dev, act[k].s_dev, D.src, D.tgt, D.idx};
	}
	if (int rc = stage_pairs(ctx, st, d, h, PairStagePlaces{L.o_pts, L.pts_bytes, L.o_idx, L.idx_bytes, L.o_jobs, L.p_pts, L.p_idx, L.p_jobs}, items.data(), count))
		return rc;

	// the graphs, their core numbers and the greedy clique sizes
	const double nb = (double)params->noise_bound, beta = (2.0 * nb) * sqrt(1.0);
	HIPCHK(ctx, put_desc());
	HIPCHK(ctx, hipMemsetAsync(d + L.o_sum, 0, (size_t)8u * count, st));
	HIPCHK(ctx, launch_teaser_batch_graph(st, d_desc, count, n_max, d, beta, reinterpret_cast<unsigned long long *>(d + L.o_sum)));
	HIPCHK(ctx, hipMemcpyAsync(h + L.p_core, d + L.o_core, L.core_bytes, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipMemcpyAsync(h + L.p_sum, d + L.o_sum, (size_t)8u * count, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::vector<uint32_t> m(count, 0u), lbs(count), cores(count), witness_at(count, 0u), Cs(count, 0u);
	uint64_t words_max = 0;
	for (uint32_t k = 0; k < count; k++)
	{
		const TeaserBatchDesc &D = L.desc[k];
		mulls_teaser_result *result = &results[act[k].index];
		const uint32_t n = D.n;
		const uint32_t *h_core = reinterpret_cast<const uint32_t *>(h + L.p_core + (D.core - L.o_core)), *h_greedy = h_core + n;
		unsigned long long deg_sum;
		std::memcpy(&deg_sum, h + L.p_sum + (size_t)8u * k, 8);
		result->n_edges = deg_sum / 2u;
		uint32_t max_core = 0, lb = 0, lb_v = 0;
		for (uint32_t i = 0; i < n; i++)
		{
			max_core = std::max(max_core, h_core[i]);
			if (h_greedy[i] > lb)
				lb = h_greedy[i], lb_v = i;
		}
		result->max_core = (int32_t)max_core;
		result->clique_exact = 1;
		lbs[k] = lb, cores[k] = max_core;
		if (lb <= 1u)
			continue; // no edge: nothing to search
		int32_t *h_keep = reinterpret_cast<int32_t *>(h + L.p_keep + (D.keep - L.o_keep));
		for (uint32_t i = 0; i < n; i++)
			if (h_core[i] + 1u >= lb)
			{
				if (i == lb_v)
					witness_at[k] = m[k];
				h_keep[m[k]++] = (int32_t)i;
			}
		words_max = std::max<uint64_t>(words_max, (uint64_t)m[k] * ((m[k] + 63u) / 64u));
	}
	const uint64_t sub_bytes = teaser_batch_pack_sub(&L, m.data());
	HIPCHK(ctx, put_desc());
	HIPCHK(ctx, hipMemcpyAsync(d + L.o_keep, h + L.p_keep, L.keep_bytes, hipMemcpyHostToDevice, st));
	HIPCHK(ctx, launch_teaser_batch_compact(st, d_desc, count, words_max, d));
	if (!device_search && sub_bytes)
		HIPCHK(ctx, hipMemcpyAsync(h + L.p_sub, d + L.o_sub, sub_bytes, hipMemcpyDeviceToHost, st)); // every sub-matrix in one copy
	HIPCHK(ctx, hipStreamSynchronize(st));

	// the cliques: per problem, in index order, by the single call's searches
	uint32_t C_max = 0;
	for (uint32_t k = 0; k < count; k++)
	{
		const TeaserBatchDesc &D = L.desc[k];
		const mulls_teaser_problem &P = problems[act[k].index];
		mulls_teaser_result *result = &results[act[k].index];
		int32_t *h_keep = reinterpret_cast<int32_t *>(h + L.p_keep + (D.keep - L.o_keep));
		std::vector<uint32_t> clique; // original vertex numbers, ascending
		if (lbs[k] <= 1u)
			clique.assign(1, 0u);
		else if (device_search)
		{
			if (int rc = device_clique_search(ctx, sc, st, BATCH, reinterpret_cast<const uint64_t *>(d + D.sub), m[k], lbs[k], cores[k], witness_at[k],
											  params->clique_node_budget, search.at(d, h), h_keep, result, &clique))
				return rc;
		}
		else if (int rc = host_clique_search(ctx, BATCH, reinterpret_cast<const uint64_t *>(h + L.p_sub + (D.sub - L.o_sub)), m[k], lbs[k], witness_at[k],
											 params->clique_node_budget, h_keep, result, &clique))
			return rc;
		const uint32_t C = (uint32_t)clique.size();
		result->clique_size = (int32_t)C;
		for (uint32_t i = 0; i < std::min(C, P.clique_cap); i++)
			P.clique[i] = (int32_t)clique[i];
		for (uint32_t i = 0; i < C; i++) // (the kept vertices are not needed any more: the list goes up in their place)
			h_keep[i] = (int32_t)clique[i];
		Cs[k] = C, C_max = std::max(C_max, C);
	}
	if (C_max <= 1u)
		return MULLS_OK;

	// the cliques' points, down in one copy; the weights planned now that every C is known
	const uint64_t cpts_bytes = teaser_batch_pack_clique(&L, Cs.data());
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the device search's last copies)
	HIPCHK(ctx, put_desc());
	HIPCHK(ctx, hipMemcpyAsync(d + L.o_keep, h + L.p_keep, L.keep_bytes, hipMemcpyHostToDevice, st));
	HIPCHK(ctx, launch_teaser_batch_pick(st, d_desc, count, C_max, d));
	HIPCHK(ctx, hipMemcpyAsync(h + L.p_cpts, d + L.o_cpts, cpts_bytes, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::vector<uint64_t> wbytes(count);
	for (uint32_t k = 0; k < count; k++)
		wbytes[k] = teaser_batch_weight_bytes(Cs[k]);
	std::vector<uint32_t> cuts;
	teaser_batch_cuts(wbytes.data(), count, limit, &cuts);
	double nb2 = nb * nb;
	if (nb2 < 1e-16)
		nb2 = 1e-2;
	TeaserGnc *d_gnc = reinterpret_cast<TeaserGnc *>(d + L.o_gnc);
	uint32_t *d_frozen = reinterpret_cast<uint32_t *>(d + L.o_frozen);
	std::vector<int> iters(count, 0);
	std::vector<char> stopped(count);
	for (size_t c = 0; c + 1 < cuts.size(); c++)
	{
		// the rotations of the problems g0 .. g1: GNC-TLS in lock-step, one launch set and one readback of the records per iteration
		const uint32_t g0 = cuts[c], g1 = cuts[c + 1];
		const uint64_t w_total = teaser_batch_place_weights(&L, g0, g1);
		uint32_t running = 0;
		uint64_t M_max = 0;
		for (uint32_t k = g0; k < g1; k++)
		{
			stopped[k] = Cs[k] < 2u;
			running += Cs[k] >= 2u;
			M_max = std::max(M_max, L.desc[k].M);
		}
		if (!running)
			continue;
		if (int rc = grow(ctx, &sc.weights, &sc.weights_cap, (size_t)(w_total / 8u)))
			return rc;
		HIPCHK(ctx, put_desc());
		HIPCHK(ctx, hipMemsetAsync(d_frozen, 0, (size_t)4u * count, st));
		const TeaserGnc *h_gnc = reinterpret_cast<const TeaserGnc *>(h + L.p_gnc);
		for (int it = 0; it < MULLS_TEASER_GNC_MAX_ITER && running; it++)
		{
			HIPCHK(ctx, launch_teaser_batch_gnc_iteration(st, d_desc, g0, g1 - g0, M_max, it, nb2, d, reinterpret_cast<unsigned char *>(sc.weights), d_gnc, d_frozen));
			HIPCHK(ctx, hipMemcpyAsync(h + L.p_gnc + sizeof(TeaserGnc) * g0, d_gnc + g0, sizeof(TeaserGnc) * (g1 - g0), hipMemcpyDeviceToHost, st));
			HIPCHK(ctx, hipStreamSynchronize(st));
			for (uint32_t k = g0; k < g1; k++)
				if (!stopped[k])
				{
					iters[k] = it + 1;
					if (h_gnc[k].stop)
						stopped[k] = 1, running--;
				}
		}
		// the translations: serial, on the cliques' points (already down) and R (a stopped problem's record is as its last iteration left it)
		for (uint32_t k = g0; k < g1; k++)
			if (Cs[k] >= 2u)
			{
				TeaserGnc G;
				std::memcpy(&G, &h_gnc[k], sizeof(G));
				const TeaserBatchDesc &D = L.desc[k];
				teaser_finish(G, iters[k], reinterpret_cast<const float *>(h + L.p_cpts + (D.cs - L.o_cpts)),
							  reinterpret_cast<const float *>(h + L.p_cpts + (D.ct - L.o_cpts)), Cs[k], nb, params, &results[act[k].index]);
			}
	}
	return MULLS_OK;
}

int teaser_batch_run(mulls_ctx *ctx, const mulls_teaser_problem *problems, uint32_t n_problems, const mulls_teaser_params *params, uint64_t limit,
					 mulls_teaser_result *results)
{
	if (!ctx || !params || (n_problems && (!problems || !results)))
		return MULLS_E_INVALID;
	for (uint32_t b = 0; b < n_problems; b++)
		reset_result(&results[b]);
	if (!n_problems)
		return MULLS_OK;
	if (int rc = check_params(Refusal{ctx, BATCH, -1}, params))
		return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	// every problem is checked before any device work: the first refusal found ends the call
	std::vector<BatchProblem> act;
	for (uint32_t b = 0; b < n_problems; b++)
	{
		const mulls_teaser_problem &P = problems[b];
		const Refusal refuse{ctx, BATCH, b};
		BatchProblem A;
		bool runs;
		A.index = b;
		if (int rc = check_pairs(refuse, P, P.tgt_idx || P.src_idx, &A, &runs))
			return rc;
		if (!runs)
			continue;
		if (int rc = check_strides(refuse, P.tgt, P.src, &A))
			return rc;
		act.push_back(A);
	}
	if (act.empty())
		return MULLS_OK;
	if (!ctx->teaser)
		ctx->teaser = new mulls_teaser_scratch();
	if (!limit)
		limit = MULLS_TEASER_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<uint64_t> bytes(act.size());
	for (size_t k = 0; k < act.size(); k++)
		bytes[k] = teaser_batch_problem_bytes(act[k].n);
	std::vector<uint32_t> cuts;
	teaser_batch_cuts(bytes.data(), (uint32_t)act.size(), limit, &cuts);
	for (size_t c = 0; c + 1 < cuts.size(); c++)
		if (int rc = teaser_sub_batch(ctx, problems, &act[cuts[c]], cuts[c + 1] - cuts[c], params, limit, results))
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
	void mulls_teaser_default_params(mulls_teaser_params *p)
	{
		if (!p)
			return;
		p->noise_bound = 0.2f; // cregistration.hpp:666
		p->min_inlier_num = 8;
		p->clique_node_budget = MULLS_TEASER_DEFAULT_NODE_BUDGET;
	}

	int mulls_coarse_reg_teaser(mulls_ctx *ctx, const mulls_cloud *tgt_pts, const mulls_cloud *src_pts, const mulls_teaser_params *params,
								mulls_teaser_result *result, int32_t *clique, uint32_t cap)
	try
	{
		return teaser_run(ctx, "mulls_coarse_reg_teaser", false, tgt_pts, src_pts, nullptr, nullptr, 0, params, result, clique, cap);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_coarse_reg_teaser_indexed(mulls_ctx *ctx, const mulls_cloud *tgt_kpts, const mulls_cloud *src_kpts, const int32_t *tgt_idx, const int32_t *src_idx,
										uint32_t n_corr, const mulls_teaser_params *params, mulls_teaser_result *result, int32_t *clique, uint32_t cap)
	try
	{
		return teaser_run(ctx, "mulls_coarse_reg_teaser_indexed", true, tgt_kpts, src_kpts, tgt_idx, src_idx, n_corr, params, result, clique, cap);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	int mulls_coarse_reg_teaser_batch(mulls_ctx *ctx, const mulls_teaser_problem *problems, uint32_t n_problems, const mulls_teaser_params *params,
									  uint64_t scratch_limit_bytes, mulls_teaser_result *results)
	try
	{
		return teaser_batch_run(ctx, problems, n_problems, params, scratch_limit_bytes, results);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}
}
