// gicp.cpp — mulls_gicp / mulls_gicp_batch: CRegistration::omp_gicp (cregistration.hpp:1024-1098) with using_voxel_gicp = true and what it calls.  Host
// side: argument checks of every problem before any device work, the identity test of the guess, the arena of a sub-batch, the uploads, the setup launch
// set, the lock-step tick loop (k_gicp.hip) and the output pose.  The pre-steps, the crop and the fitness pass are mulls_ndt's (ndt_host.h,
// ndt_launch.h).  include/mulls_hip.h has the definition this file follows.
#include <cfloat>
#include <cmath>

#include "ctx.h"
#include "gicp_launch.h"
#include "ndt_host.h"
#include "subbatch.h"

// a context's scratch of this entry point: one device arena, one pinned host buffer; grow-only
struct mulls_gicp_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr;
	size_t dev_cap = 0, pin_cap = 0;
};

void mulls_gicp_release(mulls_ctx *ctx)
{
	if (!ctx->gicp)
		return;
	staggered_free(ctx->gicp->dev);
	if (ctx->gicp->pin)
		(void)hipHostFree(ctx->gicp->pin);
	delete ctx->gicp;
	ctx->gicp = nullptr;
}

namespace
{
constexpr uint32_t MAX_SUB_BATCH = 4096u; // problems of one sub-batch (three tables each in one grid dimension of the per-point launches)

struct Plan
{
	bool apply_guess = false;
	size_t bytes = 0;
	NdtDesc N{};
	GicpDesc D{};
};

const char *check_params(const mulls_gicp_params &p)
{
	if (!(p.voxel_resolution > 0.f) || !std::isfinite(p.voxel_resolution))
		return "voxel_resolution is not a positive number";
	if (p.k_correspondences < 3 || p.k_correspondences > 32)
		return "k_correspondences outside 3 .. 32";
	if (p.max_iterations < 1 || p.max_iterations > 1000)
		return "max_iterations outside 1 .. 1000";
	if (!(p.rotation_epsilon > 0.0) || !std::isfinite(p.rotation_epsilon) || !(p.transformation_epsilon > 0.0) || !std::isfinite(p.transformation_epsilon))
		return "rotation_epsilon or transformation_epsilon is not a positive number";
	if (!(p.fitness_score_thre >= 0.f) || !std::isfinite(p.fitness_score_thre))
		return "a negative or non-finite fitness_score_thre";
	for (float v : p.start_rotvec)
		if (!std::isfinite(v) || !(std::fabs(v) <= 1.0f))
			return "start_rotvec is not finite or beyond 1 rad";
	return nullptr;
}

void lay_out(Plan &L, const mulls_gicp_problem &P, size_t &off)
{
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return (uint64_t)at;
	};
	NdtDesc &N = L.N;
	GicpDesc &D = L.D;
	const size_t n[2] = {P.src.n, P.tgt.n};
	N.n_src_in = P.src.n, N.n_tgt_in = P.tgt.n;
	N.o_src_in = take(12 * n[0]), N.o_tgt_in = take(12 * n[1]), N.o_src = take(12 * n[0]), N.o_tgt = take(12 * n[1]);
	N.o_dist = take(4 * n[0]);
	for (int tb = 0; tb < GICP_TABS; tb++)
	{
		GicpTab &T = D.tab[tb];
		const int c = tb == GICP_TAB_KNN_SRC ? 0 : 1;
		uint32_t slots = MULLS_GICP_SEG, lg = 10;
		while ((size_t)slots < 2 * n[c])
			slots <<= 1, lg++;
		T.n_cap = (uint32_t)n[c], T.slots = slots, T.shift = 64u - lg, T.pad = 0;
		T.o_pts = c ? N.o_tgt : N.o_src;
		T.o_cell = take(4 * n[c]), T.o_list = take(4 * n[c]);
		T.o_keys = take(8ull * slots);
		T.o_count = take(4ull * slots), T.o_start = take(4ull * slots), T.o_fill = take(4ull * slots); // (contiguous: cleared together)
	}
	for (int c = 0; c < 2; c++)
		D.o_cov[c] = take(48 * n[c]), D.o_left[c] = take(4 * n[c]);
	D.o_vox = take(72 * n[1]);
	D.o_partial = take(8ull * 28u * MULLS_NDT_TREE), D.o_hits = take(4ull * MULLS_NDT_TREE);
}

void fill_result_idle(const mulls_gicp_problem &P, const Plan &L, mulls_gicp_result &res)
{
	for (int k = 0; k < 16; k++)
		res.T[k] = L.apply_guess ? P.init_guess[k] : (k % 5 == 0 ? 1.0 : 0.0);
	res.fitness = DBL_MAX;
	res.code = -3;
}

// one sub-batch: problems idx[0 .. B) of the call
int run_sub_batch(mulls_ctx *ctx, const mulls_gicp_problem *problems, std::vector<Plan> &plans, const uint32_t *idx, uint32_t B, const mulls_gicp_params &prm,
				  const GicpOpts &opt, mulls_gicp_result *results, const std::string &who, bool single)
{
	mulls_gicp_scratch &sc = *ctx->gicp;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	const uint32_t max_ticks = (uint32_t)prm.max_iterations;
	size_t off = 0;
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return at;
	};
	const size_t o_ndesc = take(sizeof(NdtDesc) * (size_t)B), o_desc = take(sizeof(GicpDesc) * (size_t)B);
	const size_t o_nrec = take(sizeof(NdtRec) * (size_t)B), o_rec = take(sizeof(GicpRec) * (size_t)B);
	const size_t o_frames = take(96ull * B), o_cnt = take(4ull * (max_ticks + 2u));
	uint32_t ns_max = 0, n_max = 0, slots_max = 0;
	size_t pin_need = std::max(up256(sizeof(NdtDesc) * (size_t)B) + up256(sizeof(GicpDesc) * (size_t)B), up256(sizeof(NdtRec) * (size_t)B) + up256(sizeof(GicpRec) * (size_t)B));
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_gicp_problem &P = problems[idx[k]];
		Plan &L = plans[idx[k]];
		lay_out(L, P, off);
		ns_max = std::max(ns_max, P.src.n), n_max = std::max(n_max, std::max(P.src.n, P.tgt.n));
		slots_max = std::max(slots_max, L.D.tab[GICP_TAB_VOXEL].slots);
		pin_need = std::max<size_t>(pin_need, 12ull * std::max(P.src.n, P.tgt.n));
	}
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
		return rc;
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, pin_need, hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin;
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_gicp_problem &P = problems[idx[k]];
		const Plan &L = plans[idx[k]];
		if (int rc = ndt_host::upload_cloud(ctx, P.src, d + L.N.o_src_in, h))
			return rc;
		if (int rc = ndt_host::upload_cloud(ctx, P.tgt, d + L.N.o_tgt_in, h))
			return rc;
		for (int tb = 0; tb < GICP_TABS; tb++)
		{
			const GicpTab &T = L.D.tab[tb];
			HIPCHK(ctx, hipMemsetAsync(d + T.o_keys, 0xff, 8ull * T.slots, st));
			HIPCHK(ctx, hipMemsetAsync(d + T.o_count, 0, 3 * up256(4ull * T.slots), st)); // count, start, fill
		}
	}
	{
		NdtDesc *hn = reinterpret_cast<NdtDesc *>(h);
		GicpDesc *hd = reinterpret_cast<GicpDesc *>(h + up256(sizeof(NdtDesc) * (size_t)B));
		for (uint32_t k = 0; k < B; k++)
			hn[k] = plans[idx[k]].N, hd[k] = plans[idx[k]].D;
		HIPCHK(ctx, hipMemcpyAsync(d + o_ndesc, hn, sizeof(NdtDesc) * (size_t)B, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, hipMemcpyAsync(d + o_desc, hd, sizeof(GicpDesc) * (size_t)B, hipMemcpyHostToDevice, st));
	}
	HIPCHK(ctx, hipMemsetAsync(d + o_nrec, 0, sizeof(NdtRec) * (size_t)B, st));
	HIPCHK(ctx, hipMemsetAsync(d + o_rec, 0, sizeof(GicpRec) * (size_t)B, st));
	HIPCHK(ctx, hipMemsetAsync(d + o_cnt, 0, 4ull * (max_ticks + 2u), st));
	const NdtDesc *ndesc = reinterpret_cast<const NdtDesc *>(d + o_ndesc);
	const GicpDesc *desc = reinterpret_cast<const GicpDesc *>(d + o_desc);
	NdtRec *nrec = reinterpret_cast<NdtRec *>(d + o_nrec);
	GicpRec *rec = reinterpret_cast<GicpRec *>(d + o_rec);
	double *frames = reinterpret_cast<double *>(d + o_frames);
	uint32_t *cnt = reinterpret_cast<uint32_t *>(d + o_cnt); // [0]: the largest leftover count; [1 + tick]: the problems still running
	// the setup's launch set: the crop (no NDT grid: a zero inverse resolution puts every point into cell 0), the tables, the covariances, the voxels
	NdtOpts nopt{};
	HIPCHK(ctx, launch_ndt_crop(st, ndesc, B, d, nopt, nrec));
	HIPCHK(ctx, launch_gicp_begin(st, B, nrec, rec, frames, opt));
	HIPCHK(ctx, launch_gicp_tables(st, desc, B, n_max, d, opt, rec));
	HIPCHK(ctx, launch_gicp_knn(st, desc, B, n_max, d, opt, rec, cnt));
	uint32_t *h_word = reinterpret_cast<uint32_t *>(h);
	HIPCHK(ctx, hipMemcpyAsync(h_word, cnt, 4, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the descriptors have left the pinned buffer)
	HIPCHK(ctx, launch_gicp_brute(st, desc, B, std::min(*h_word, n_max), d, opt, rec));
	HIPCHK(ctx, launch_gicp_voxels(st, desc, B, slots_max, d, rec));
	for (uint32_t tick = 0; tick < max_ticks; tick++)
	{
		HIPCHK(ctx, launch_gicp_eval(st, desc, B, d, opt, rec));
		HIPCHK(ctx, launch_gicp_decide(st, desc, B, d, opt, rec, frames, cnt + 1 + tick));
		HIPCHK(ctx, hipMemcpyAsync(h_word, cnt + 1 + tick, 4, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		if (*h_word == 0)
			break;
	}
	HIPCHK(ctx, launch_ndt_fitness(st, ndesc, B, ns_max, d, nrec, frames));
	std::vector<NdtRec> nrecs(B);
	std::vector<GicpRec> recs(B);
	unsigned char *h2 = h + up256(sizeof(NdtRec) * (size_t)B);
	HIPCHK(ctx, hipMemcpyAsync(h, nrec, sizeof(NdtRec) * (size_t)B, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipMemcpyAsync(h2, rec, sizeof(GicpRec) * (size_t)B, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::memcpy(nrecs.data(), h, sizeof(NdtRec) * (size_t)B);
	std::memcpy(recs.data(), h2, sizeof(GicpRec) * (size_t)B);
	for (uint32_t k = 0; k < B; k++)
	{
		const bool range = recs[k].status == GICP_ST_OK && recs[k].range;
		if (recs[k].status == GICP_ST_NONFINITE || range)
		{
			ctx->err = who + (single ? std::string() : "problem " + std::to_string(idx[k]) + ": ") +
					   (range ? "a coordinate lies beyond 2^20 voxels" : "a coordinate is not finite");
			return range ? MULLS_E_UNSUPPORTED : MULLS_E_INVALID;
		}
	}
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_gicp_problem &P = problems[idx[k]];
		const Plan &L = plans[idx[k]];
		const GicpRec &R = recs[k];
		mulls_gicp_result &res = results[idx[k]];
		std::memset(&res, 0, sizeof(res));
		res.n_src = R.n[0], res.n_tgt = R.n[1];
		if (R.status == GICP_ST_FEW)
		{
			fill_result_idle(P, L, res);
			continue;
		}
		res.n_voxels = R.n_voxels, res.n_corr = R.S.n_corr, res.loss = R.S.loss;
		res.iterations = R.S.iterations, res.converged = R.S.converged, res.stop = R.S.stop;
		res.fitness = nrecs[k].fitness;
		res.code = res.fitness > (double)prm.fitness_score_thre ? -3 : 1;
		// T = (exp(r), t) guess
		double Tn[16] = {0};
		for (int r = 0; r < 3; r++)
		{
			for (int c = 0; c < 3; c++)
				Tn[r + 4 * c] = R.S.R[3 * r + c];
			Tn[r + 12] = R.S.t[r];
		}
		Tn[15] = 1.0;
		ndt_host::pose_times_guess(Tn, L.apply_guess ? P.init_guess : nullptr, res.T);
	}
	return MULLS_OK;
}

int gicp_run(mulls_ctx *ctx, const mulls_gicp_problem *problems, uint32_t n_problems, const mulls_gicp_params *params, mulls_gicp_result *results,
			 const char *name, bool single)
{
	if (!ctx || !params || (n_problems && (!problems || !results)))
		return MULLS_E_INVALID;
	const std::string who = std::string(name) + ": ";
	if (const char *bad = check_params(*params))
	{
		ctx->err = who + bad;
		return MULLS_E_INVALID;
	}
	if (!params->using_voxel_gicp)
	{
		ctx->err = who + "plain GICP (using_voxel_gicp = false, PCL's BFGS GeneralizedIterativeClosestPoint) is not built";
		return MULLS_E_UNSUPPORTED;
	}
	std::vector<Plan> plans(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
	{
		std::string msg;
		if (int rc = ndt_host::check_problem(problems[b], msg))
		{
			ctx->err = who + (single ? std::string() : "problem " + std::to_string(b) + ": ") + msg;
			return rc;
		}
	}
	if (!n_problems)
		return MULLS_OK;
	GicpOpts opt{};
	opt.resolution = params->voxel_resolution;
	opt.knn_edge = (double)params->voxel_resolution, opt.knn_inv_edge = 1.0 / opt.knn_edge;
	opt.rotation_epsilon = params->rotation_epsilon, opt.transformation_epsilon = params->transformation_epsilon;
	opt.k = params->k_correspondences, opt.max_iterations = params->max_iterations;
	for (int k = 0; k < 3; k++)
		opt.start_rotvec[k] = params->start_rotvec[k];
	for (uint32_t b = 0; b < n_problems; b++)
	{
		const mulls_gicp_problem &P = problems[b];
		Plan &L = plans[b];
		NdtDesc &N = L.N;
		L.apply_guess = !ndt_host::is_identity(P.init_guess, 1e-6);
		N.apply_guess = L.apply_guess ? 1 : 0, N.crop = params->apply_intersection_filter ? 1 : 0;
		for (int r = 0; r < 3; r++)
		{
			for (int c = 0; c < 3; c++)
				N.G[3 * r + c] = P.init_guess[r + 4 * c];
			N.G[9 + r] = P.init_guess[12 + r];
		}
		std::memcpy(N.tgt_bound, P.tgt_bound, sizeof(N.tgt_bound)), std::memcpy(N.src_bound, P.src_bound, sizeof(N.src_bound));
		size_t off = 0;
		Plan t = L;
		lay_out(t, P, off);
		L.bytes = off;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (!ctx->gicp)
		ctx->gicp = new mulls_gicp_scratch();
	const size_t limit = params->scratch_limit_bytes ? (size_t)params->scratch_limit_bytes : (size_t)MULLS_GICP_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<mulls_gicp_result> out(n_problems); // (results are written only when the whole call succeeds)
	std::vector<uint32_t> work(n_problems), cuts;
	std::vector<uint64_t> bytes(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
		work[b] = b, bytes[b] = plans[b].bytes;
	sub_batch_cuts(bytes.data(), n_problems, limit, MAX_SUB_BATCH, &cuts);
	for (size_t c = 0; c + 1 < cuts.size(); c++)
		if (int rc = run_sub_batch(ctx, problems, plans, work.data() + cuts[c], cuts[c + 1] - cuts[c], *params, opt, out.data(), who, single))
			return rc;
	std::memcpy(results, out.data(), sizeof(mulls_gicp_result) * (size_t)n_problems);
	return MULLS_OK;
}
} // namespace

extern "C"
{
	void mulls_gicp_default_params(mulls_gicp_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->voxel_resolution = 1.0f;
		p->k_correspondences = 20;
		p->max_iterations = 64;
		p->apply_intersection_filter = 0;
		p->rotation_epsilon = 2e-3;
		p->transformation_epsilon = 5e-4;
		p->fitness_score_thre = 10.0f;
		p->using_voxel_gicp = 1;
		p->start_rotvec[0] = p->start_rotvec[1] = p->start_rotvec[2] = 0.005773503f;
	}

	int mulls_gicp(mulls_ctx *ctx, const mulls_gicp_problem *problem, const mulls_gicp_params *params, mulls_gicp_result *result)
	try
	{
		if (!problem || !result)
			return MULLS_E_INVALID;
		return gicp_run(ctx, problem, 1, params, result, "mulls_gicp", true);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	int mulls_gicp_batch(mulls_ctx *ctx, const mulls_gicp_problem *problems, uint32_t n_problems, const mulls_gicp_params *params, mulls_gicp_result *results)
	try
	{
		return gicp_run(ctx, problems, n_problems, params, results, "mulls_gicp_batch", false);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}
}
