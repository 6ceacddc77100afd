// gicp.cpp — mulls_gicp / mulls_gicp_batch: CRegistration::omp_gicp (cregistration.hpp:1024-1098) with using_voxel_gicp = true and what it calls.  Host
// side: argument checks of every problem before any device work, the arena of a sub-batch, the uploads, the setup launch set (the cell tables:
// reg_launch.h), the lock-step tick loop (k_gicp.hip) and the results.  The crop and the fitness pass are mulls_ndt's (ndt_launch.h); what a call and a
// sub-batch have in common with mulls_ndt's and mulls_pcl_icp's is reg_host.h's.  include/mulls_hip.h has the definition this file follows.
#include <cfloat>
#include <cmath>

#include "ctx.h"
#include "gicp_launch.h"
#include "reg_host.h"

namespace
{
struct Plan
{
	bool apply_guess = false;
	NdtDesc N{};
	GicpDesc D{};
	RegTab tab[MULLS_REG_TABS]{};
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

void lay_out(Plan &L, const mulls_gicp_problem &P, const GicpOpts &opt, reg_host::Arena &take)
{
	NdtDesc &N = L.N;
	GicpDesc &D = L.D;
	const size_t n[2] = {P.src.n, P.tgt.n};
	N.n_src_in = P.src.n, N.n_tgt_in = P.tgt.n;
	N.o_src_in = take(12 * n[0]), N.o_tgt_in = take(12 * n[1]), N.o_src = take(12 * n[0]), N.o_tgt = take(12 * n[1]);
	N.o_dist = take(4 * n[0]);
	for (int tb = 0; tb < GICP_TABS; tb++)
	{
		RegTab &T = L.tab[tb];
		T = RegTab{};
		T.cloud = tb == GICP_TAB_KNN_SRC ? 0 : 1, T.refuses = 1;
		T.rule = tb == GICP_TAB_VOXEL ? REG_COORD_VOXEL : REG_COORD_CELL;
		T.resolution = opt.resolution, T.inv_edge = 1.0 / opt.knn_edge;
		reg_table_lay_out(T, n[T.cloud], T.cloud ? N.o_tgt : N.o_src, false, take);
	}
	for (int c = 0; c < 2; c++)
		D.o_cov[c] = take(48 * n[c]), D.o_left[c] = take(4 * n[c]);
	D.o_vox = take(72 * n[1]);
	D.o_partial = take(8ull * 28u * MULLS_NDT_TREE), D.o_hits = take(4ull * MULLS_NDT_TREE);
}

// one sub-batch: problems idx[0 .. B) of the call
int run_sub_batch(mulls_ctx *ctx, const mulls_gicp_problem *problems, std::vector<Plan> &plans, const uint32_t *idx, uint32_t B, const mulls_gicp_params &prm,
				  const GicpOpts &opt, mulls_gicp_result *results, const std::string &who, bool single)
{
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	reg_host::Arena take;
	const size_t ndesc_bytes = sizeof(NdtDesc) * (size_t)B, desc_bytes = sizeof(GicpDesc) * (size_t)B, tab_bytes = sizeof(RegTab) * MULLS_REG_TABS * (size_t)B;
	const size_t nrec_bytes = sizeof(NdtRec) * (size_t)B, rec_bytes = sizeof(GicpRec) * (size_t)B, head_bytes = sizeof(RegHead) * (size_t)B;
	const size_t o_ndesc = take(ndesc_bytes), o_desc = take(desc_bytes), o_tabs = take(tab_bytes);
	const size_t o_nrec = take(nrec_bytes), o_rec = take(rec_bytes), o_head = take(head_bytes);
	const size_t o_frames = take(96ull * B), o_cnt = take(12);
	uint32_t ns_max = 0, n_max = 0, slots_max = 0;
	std::vector<NdtDesc> ndescs(B);
	std::vector<GicpDesc> descs(B);
	std::vector<RegTab> tabs_h(MULLS_REG_TABS * (size_t)B);
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_gicp_problem &P = problems[idx[k]];
		Plan &L = plans[idx[k]];
		lay_out(L, P, opt, take);
		ndescs[k] = L.N, descs[k] = L.D;
		for (int tb = 0; tb < GICP_TABS; tb++)
			tabs_h[MULLS_REG_TABS * (size_t)k + tb] = L.tab[tb], slots_max = std::max(slots_max, L.tab[tb].slots);
		ns_max = std::max(ns_max, P.src.n), n_max = std::max(n_max, std::max(P.src.n, P.tgt.n));
	}
	const size_t pin_need =
		std::max<size_t>({reg_host::pinned_bytes({ndesc_bytes, desc_bytes, tab_bytes}), reg_host::pinned_bytes({nrec_bytes, rec_bytes, head_bytes}), (size_t)12 * n_max});
	unsigned char *d, *h;
	if (int rc = reg_host::reserve(ctx, take.off, pin_need, &d, &h))
		return rc;
	for (uint32_t k = 0; k < B; k++)
		if (int rc = reg_host::upload_problem(ctx, problems[idx[k]], ndescs[k], d, h))
			return rc;
	if (int rc = reg_host::stage(ctx, h, {{d + o_ndesc, ndescs.data(), ndesc_bytes}, {d + o_desc, descs.data(), desc_bytes}, {d + o_tabs, tabs_h.data(), tab_bytes}}))
		return rc;
	HIPCHK(ctx, hipMemsetAsync(d + o_nrec, 0, nrec_bytes, st));
	HIPCHK(ctx, hipMemsetAsync(d + o_cnt, 0, 12, st));
	const NdtDesc *ndesc = reinterpret_cast<const NdtDesc *>(d + o_ndesc);
	const GicpDesc *desc = reinterpret_cast<const GicpDesc *>(d + o_desc);
	const RegTab *tabs = reinterpret_cast<const RegTab *>(d + o_tabs);
	NdtRec *nrec = reinterpret_cast<NdtRec *>(d + o_nrec);
	GicpRec *rec = reinterpret_cast<GicpRec *>(d + o_rec); // (written whole by k_gicp_begin, as the heads are)
	RegHead *head = reinterpret_cast<RegHead *>(d + o_head);
	double *frames = reinterpret_cast<double *>(d + o_frames);
	uint32_t *cnt = reinterpret_cast<uint32_t *>(d + o_cnt); // [0], [1]: the problems still running after an even, an odd tick; [2]: the largest leftover count
	// the setup's launch set: the crop (no NDT grid: a zero inverse resolution puts every point into cell 0), the tables, the covariances, the voxels
	NdtOpts nopt{};
	HIPCHK(ctx, launch_ndt_crop(st, ndesc, B, d, nopt, nrec));
	HIPCHK(ctx, launch_gicp_begin(st, B, nrec, rec, head, frames, opt));
	HIPCHK(ctx, launch_reg_tables(st, tabs, B, 0, GICP_TABS, n_max, slots_max, d, head));
	HIPCHK(ctx, launch_gicp_knn(st, desc, tabs, B, n_max, d, opt, rec, head, cnt + 2));
	uint32_t *h_word = reinterpret_cast<uint32_t *>(h);
	HIPCHK(ctx, hipMemcpyAsync(h_word, cnt + 2, 4, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the descriptors have left the pinned buffer)
	HIPCHK(ctx, launch_gicp_brute(st, desc, tabs, B, std::min(*h_word, n_max), d, opt, rec, head));
	HIPCHK(ctx, launch_gicp_voxels(st, desc, tabs, B, slots_max, d, head));
	if (int rc = reg_host::tick_loop(ctx, cnt, h, (uint32_t)prm.max_iterations, [&](uint32_t *running, uint32_t *next) -> int {
			HIPCHK(ctx, launch_gicp_eval(st, desc, tabs, B, d, opt, rec, head));
			HIPCHK(ctx, launch_gicp_decide(st, desc, B, d, opt, rec, head, frames, running, next));
			return MULLS_OK;
		}))
		return rc;
	HIPCHK(ctx, launch_ndt_fitness(st, ndesc, B, ns_max, d, nrec, frames));
	std::vector<NdtRec> nrecs(B);
	std::vector<GicpRec> recs(B);
	std::vector<RegHead> heads(B);
	if (int rc = reg_host::download(ctx, h, {{nrec, nrecs.data(), nrec_bytes}, {rec, recs.data(), rec_bytes}, {head, heads.data(), head_bytes}}))
		return rc;
	for (uint32_t k = 0; k < B; k++)
	{
		const bool range = heads[k].status == GICP_ST_OK && heads[k].range;
		if (heads[k].status == GICP_ST_NONFINITE || range)
		{
			ctx->err = reg_host::refusal_prefix(who, single, idx[k]) + (range ? "a coordinate lies beyond 2^20 voxels" : "a coordinate is not finite");
			return range ? MULLS_E_UNSUPPORTED : MULLS_E_INVALID;
		}
	}
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_gicp_problem &P = problems[idx[k]];
		const Plan &L = plans[idx[k]];
		const GicpRec &R = recs[k];
		const RegHead &H = heads[k];
		mulls_gicp_result &res = results[idx[k]];
		std::memset(&res, 0, sizeof(res));
		res.n_src = H.n[0], res.n_tgt = H.n[1];
		if (H.status == GICP_ST_FEW)
		{
			reg_host::idle_pose(P, L.apply_guess, res.T);
			res.fitness = DBL_MAX;
			res.code = -3;
			continue;
		}
		res.n_voxels = H.occupied[GICP_TAB_VOXEL], res.n_corr = R.S.n_corr, res.loss = R.S.loss;
		res.iterations = R.S.iterations, res.converged = R.S.converged, res.stop = R.S.stop;
		res.fitness = nrecs[k].fitness;
		res.code = res.fitness > (double)prm.fitness_score_thre ? -3 : 1;
		reg_host::pose_of(R.S.R, R.S.t, P, L.apply_guess, res.T); // T = (exp(r), t) guess
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
	if (int rc = reg_host::check_problems(ctx, problems, n_problems, who, single))
		return rc;
	if (!n_problems)
		return MULLS_OK;
	GicpOpts opt{};
	opt.resolution = params->voxel_resolution;
	opt.knn_edge = (double)params->voxel_resolution;
	opt.rotation_epsilon = params->rotation_epsilon, opt.transformation_epsilon = params->transformation_epsilon;
	opt.k = params->k_correspondences, opt.max_iterations = params->max_iterations;
	for (int k = 0; k < 3; k++)
		opt.start_rotvec[k] = params->start_rotvec[k];
	std::vector<Plan> plans(n_problems);
	std::vector<uint64_t> bytes(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
	{
		Plan &L = plans[b];
		L.apply_guess = reg_host::crop_desc(problems[b], params->apply_intersection_filter != 0, L.N);
		reg_host::Arena dry;
		Plan t = L;
		lay_out(t, problems[b], opt, dry);
		bytes[b] = dry.off;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t limit = params->scratch_limit_bytes ? (size_t)params->scratch_limit_bytes : (size_t)MULLS_GICP_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<mulls_gicp_result> out(n_problems); // (results are written only when the whole call succeeds)
	std::vector<uint32_t> work(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
		work[b] = b;
	const std::vector<uint32_t> cuts = reg_host::cuts_of(bytes, limit);
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
