// ndt.cpp — mulls_ndt / mulls_ndt_batch: CRegistration::omp_ndt (cregistration.hpp:945-1021) with what it calls.  Host side: argument checks of every
// problem before any device work, the score constants, the arena of a sub-batch, the uploads, the lock-step tick loop (k_ndt.hip) and the results.  What
// a call and a sub-batch have in common with mulls_gicp's and mulls_pcl_icp's is reg_host.h's.  include/mulls_hip.h has the definition this file follows.
#include <cfloat>
#include <cmath>

#include "ctx.h"
#include "ndt_launch.h"
#include "reg_host.h"

namespace
{
struct Plan
{
	bool apply_guess = false;
	NdtDesc D{};
};

const char *check_params(const mulls_ndt_params &p)
{
	if (!(p.resolution > 0.f) || !std::isfinite(p.resolution))
		return "resolution is not a positive number";
	if (p.search_method < MULLS_NDT_KDTREE || p.search_method > MULLS_NDT_DIRECT1)
		return "an unknown search_method";
	if (p.max_iterations < 0 || p.max_iterations > 1000 || p.max_step_iterations < 0 || p.max_step_iterations > 1000)
		return "max_iterations or max_step_iterations outside 0 .. 1000";
	if (p.min_points_per_voxel < 1)
		return "min_points_per_voxel below 1";
	const double v[] = {p.step_size, p.transformation_epsilon, p.outlier_ratio, p.min_covar_eigvalue_mult, (double)p.fitness_score_thre};
	for (double x : v)
		if (!(x >= 0.0) || !std::isfinite(x))
			return "a negative or non-finite step_size, transformation_epsilon, outlier_ratio, min_covar_eigvalue_mult or fitness_score_thre";
	if (!(p.outlier_ratio > 0.0 && p.outlier_ratio < 1.0))
		return "outlier_ratio outside (0, 1)";
	return nullptr;
}

void lay_out(NdtDesc &D, const mulls_ndt_problem &P, reg_host::Arena &take)
{
	const size_t ns = P.src.n, nt = P.tgt.n;
	D.n_src_in = P.src.n, D.n_tgt_in = P.tgt.n;
	uint32_t ts = MULLS_NDT_SEG, lg = 10;
	while ((size_t)ts < 2 * nt)
		ts <<= 1, lg++;
	D.table_size = ts, D.table_shift = 32u - lg;
	D.o_src_in = take(12 * ns), D.o_tgt_in = take(12 * nt), D.o_src = take(12 * ns), D.o_tgt = take(12 * nt);
	D.o_cell = take(4 * nt), D.o_list = take(4 * nt);
	D.o_keys = take(4ull * ts), D.o_count = take(4ull * ts), D.o_start = take(4ull * ts), D.o_fill = take(4ull * ts);
	D.o_leaves = take(sizeof(ndt::Leaf) * nt), D.o_partial = take(8ull * 28u * MULLS_NDT_TREE), D.o_dist = take(4 * ns);
}

// one sub-batch: problems idx[0 .. B) of the call
int run_sub_batch(mulls_ctx *ctx, const mulls_ndt_problem *problems, std::vector<Plan> &plans, const uint32_t *idx, uint32_t B, const mulls_ndt_params &prm,
				  const NdtOpts &opt, mulls_ndt_result *results, const std::string &who, bool single)
{
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	// the first evaluation, then per Newton iteration (at most max_iterations + 2 of them) one trial, the inner steps and the Hessian pass
	const uint32_t max_ticks = (uint32_t)(prm.max_iterations + 2) * (uint32_t)(prm.max_step_iterations + 2) + 1u;
	reg_host::Arena take;
	const size_t desc_bytes = sizeof(NdtDesc) * (size_t)B, rec_bytes = sizeof(NdtRec) * (size_t)B;
	const size_t o_desc = take(desc_bytes), o_rec = take(rec_bytes), o_cnt = take(8);
	uint32_t ns_max = 0, nt_max = 0, table_max = 0;
	std::vector<NdtDesc> descs(B);
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_ndt_problem &P = problems[idx[k]];
		lay_out(plans[idx[k]].D, P, take);
		descs[k] = plans[idx[k]].D;
		ns_max = std::max(ns_max, P.src.n), nt_max = std::max(nt_max, P.tgt.n), table_max = std::max(table_max, descs[k].table_size);
	}
	unsigned char *d, *h;
	if (int rc = reg_host::reserve(ctx, take.off, std::max<size_t>(up256(std::max(desc_bytes, rec_bytes)), 12ull * std::max(ns_max, nt_max)), &d, &h))
		return rc;
	for (uint32_t k = 0; k < B; k++)
		if (int rc = reg_host::upload_problem(ctx, problems[idx[k]], descs[k], d, h))
			return rc;
	if (int rc = reg_host::stage(ctx, h, {{d + o_desc, descs.data(), desc_bytes}}))
		return rc;
	HIPCHK(ctx, hipMemsetAsync(d + o_rec, 0, rec_bytes, st));
	HIPCHK(ctx, hipMemsetAsync(d + o_cnt, 0, 8, st));
	const NdtDesc *desc = reinterpret_cast<const NdtDesc *>(d + o_desc);
	NdtRec *rec = reinterpret_cast<NdtRec *>(d + o_rec);
	HIPCHK(ctx, launch_ndt_crop(st, desc, B, d, opt, rec));
	HIPCHK(ctx, launch_ndt_cells(st, desc, B, nt_max, table_max, d, opt, rec));
	HIPCHK(ctx, launch_ndt_offsets(st, desc, B, d, rec));
	HIPCHK(ctx, launch_ndt_scatter(st, desc, B, nt_max, d, rec));
	HIPCHK(ctx, launch_ndt_leaves(st, desc, B, table_max, d, opt, rec));
	HIPCHK(ctx, launch_ndt_begin(st, B, rec));
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the descriptors have left the pinned buffer)
	if (int rc = reg_host::tick_loop(ctx, reinterpret_cast<uint32_t *>(d + o_cnt), h, max_ticks, [&](uint32_t *running, uint32_t *next) -> int {
			HIPCHK(ctx, launch_ndt_eval(st, desc, B, d, opt, rec));
			HIPCHK(ctx, launch_ndt_decide(st, desc, B, d, opt, rec, running, next));
			return MULLS_OK;
		}))
		return rc;
	HIPCHK(ctx, launch_ndt_fitness(st, desc, B, ns_max, d, rec, nullptr));
	std::vector<NdtRec> recs(B);
	if (int rc = reg_host::download(ctx, h, {{rec, recs.data(), rec_bytes}}))
		return rc;
	for (uint32_t k = 0; k < B; k++)
		if (recs[k].status == NDT_ST_NONFINITE || recs[k].status == NDT_ST_GRID)
		{
			ctx->err = reg_host::refusal_prefix(who, single, idx[k]) +
					   (recs[k].status == NDT_ST_GRID ? "the voxel grid has more than INT32_MAX cells" : "a coordinate is not finite");
			return recs[k].status == NDT_ST_GRID ? MULLS_E_UNSUPPORTED : MULLS_E_INVALID;
		}
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_ndt_problem &P = problems[idx[k]];
		const Plan &L = plans[idx[k]];
		const NdtRec &R = recs[k];
		mulls_ndt_result &res = results[idx[k]];
		res.n_src = R.n_src, res.n_tgt = R.n_tgt;
		if (R.status == NDT_ST_EMPTY)
		{
			reg_host::idle_pose(P, L.apply_guess, res.T);
			res.fitness = DBL_MAX;
			res.code = -3;
			continue;
		}
		res.n_leaves = R.n_leaves, res.n_leaves_used = R.n_leaves_used;
		res.iterations = R.S.nr_iterations, res.evaluations = R.S.evaluations, res.converged = R.S.converged;
		res.line_search_reversals = R.S.reversals, res.inner_steps = R.S.inner_steps;
		res.trans_probability = R.S.trans_probability;
		res.fitness = R.fitness;
		res.code = res.fitness > (double)prm.fitness_score_thre ? -3 : 1;
		ndt::Frame F; // T = T(p) guess
		ndt::make_frame(R.S.p, &F);
		reg_host::pose_of(F.R, F.t, P, L.apply_guess, res.T);
	}
	return MULLS_OK;
}

int ndt_run(mulls_ctx *ctx, const mulls_ndt_problem *problems, uint32_t n_problems, const mulls_ndt_params *params, mulls_ndt_result *results,
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
	if (params->search_method == MULLS_NDT_KDTREE)
	{
		ctx->err = who + "the kd-tree search over leaf centroids (use_direct_search = false) is not built";
		return MULLS_E_UNSUPPORTED;
	}
	if (int rc = reg_host::check_problems(ctx, problems, n_problems, who, single))
		return rc;
	if (!n_problems)
		return MULLS_OK;
	// the score constants (ndt_omp_impl.hpp:86-93), by the host's C library
	NdtOpts opt{};
	const double c1 = 10 * (1 - params->outlier_ratio), c2 = params->outlier_ratio / std::pow((double)params->resolution, 3);
	const double d3 = -std::log(c2), d1 = -std::log(c1 + c2) - d3, d2 = -2 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / d1);
	opt.d1 = d1, opt.d2 = d2, opt.eig_mult = params->min_covar_eigvalue_mult;
	opt.resolution = params->resolution, opt.inv_resolution = 1.0f / params->resolution, opt.min_points = params->min_points_per_voxel;
	opt.o.step_size = params->step_size, opt.o.transformation_epsilon = params->transformation_epsilon, opt.o.mu = 1.e-4, opt.o.nu = 0.9;
	opt.o.max_iterations = params->max_iterations, opt.o.max_step_iterations = params->max_step_iterations;
	std::vector<Plan> plans(n_problems);
	std::vector<uint64_t> bytes(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
	{
		Plan &L = plans[b];
		L.apply_guess = reg_host::crop_desc(problems[b], params->apply_intersection_filter != 0, L.D);
		L.D.n_offsets = params->search_method == MULLS_NDT_DIRECT1 ? 1 : (params->search_method == MULLS_NDT_DIRECT7 ? 7 : 26);
		L.D.offset_first = params->search_method == MULLS_NDT_DIRECT26 ? 7 : 0;
		reg_host::Arena dry;
		NdtDesc t = L.D;
		lay_out(t, problems[b], dry);
		bytes[b] = dry.off;
		mulls_ndt_result &res = results[b];
		std::memset(&res, 0, sizeof(res));
		res.gauss_d1 = d1, res.gauss_d2 = d2, res.gauss_d3 = d3;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t limit = params->scratch_limit_bytes ? (size_t)params->scratch_limit_bytes : (size_t)MULLS_NDT_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<uint32_t> work(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
		work[b] = b;
	const std::vector<uint32_t> cuts = reg_host::cuts_of(bytes, limit);
	for (size_t c = 0; c + 1 < cuts.size(); c++)
		if (int rc = run_sub_batch(ctx, problems, plans, work.data() + cuts[c], cuts[c + 1] - cuts[c], *params, opt, results, who, single))
			return rc;
	return MULLS_OK;
}
} // namespace

extern "C"
{
	void mulls_ndt_default_params(mulls_ndt_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->resolution = 1.0f;
		p->search_method = MULLS_NDT_DIRECT7;
		p->apply_intersection_filter = 1;
		p->fitness_score_thre = 10.0f;
		p->step_size = 0.1;
		p->transformation_epsilon = 0.1;
		p->outlier_ratio = 0.55;
		p->min_covar_eigvalue_mult = 0.01;
		p->max_iterations = 35;
		p->max_step_iterations = 10;
		p->min_points_per_voxel = 6;
	}

	int mulls_ndt(mulls_ctx *ctx, const mulls_ndt_problem *problem, const mulls_ndt_params *params, mulls_ndt_result *result)
	try
	{
		if (!problem || !result)
			return MULLS_E_INVALID;
		return ndt_run(ctx, problem, 1, params, result, "mulls_ndt", true);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	int mulls_ndt_batch(mulls_ctx *ctx, const mulls_ndt_problem *problems, uint32_t n_problems, const mulls_ndt_params *params, mulls_ndt_result *results)
	try
	{
		return ndt_run(ctx, problems, n_problems, params, results, "mulls_ndt_batch", false);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}
}
