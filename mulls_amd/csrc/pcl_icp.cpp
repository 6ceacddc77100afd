// pcl_icp.cpp — mulls_pcl_icp / mulls_pcl_icp_batch: CRegistration::pcl_icp (cregistration.hpp:882-942) over icp_registration (:84-315), the part that
// is plain ICP.  Host side: argument checks of every problem before any device work, the arena of a sub-batch, the uploads, the setup launch set (the
// cell tables: reg_launch.h), the lock-step tick loop (k_pcl_icp.hip) and the results.  The crop and the nearest-neighbour pass of the fitness are
// mulls_ndt's (ndt_launch.h); what a call and a sub-batch have in common with mulls_ndt's and mulls_gicp's is reg_host.h's.  include/mulls_hip.h has the
// definition this file follows.
#include <cfloat>
#include <cmath>

#include "ctx.h"
#include "pcl_icp_launch.h"
#include "reg_host.h"

namespace
{
constexpr double CELL_MARGIN = 1.0 + 0x1p-20; // a cell's edge over the distance it serves: the 27-cell walks are exact (include/mulls_hip.h)

struct Plan
{
	bool apply_guess = false;
	NdtDesc N{};
	PclIcpDesc D{};
	RegTab tab[MULLS_REG_TABS]{};
};

// -> the message and MULLS_E_INVALID or MULLS_E_UNSUPPORTED, or MULLS_OK
int check_params(const mulls_pcl_icp_params &p, const char **msg)
{
	auto bad = [&](const char *m, int rc) {
		*msg = m;
		return rc;
	};
	if (p.max_iter_num < 1)
		return bad("max_iter_num below 1", MULLS_E_INVALID);
	if (!(p.dis_thre_unit > 0.f) || !std::isfinite(p.dis_thre_unit))
		return bad("dis_thre_unit is not a positive number", MULLS_E_INVALID);
	if (!(p.neighbor_radius > 0.f) || !std::isfinite(p.neighbor_radius))
		return bad("neighbor_radius is not a positive number", MULLS_E_INVALID);
	if (!(p.transformation_epsilon >= 0.0) || !std::isfinite(p.transformation_epsilon) || !(p.euclidean_fitness_epsilon >= 0.0) ||
		!std::isfinite(p.euclidean_fitness_epsilon))
		return bad("a negative or non-finite transformation_epsilon or euclidean_fitness_epsilon", MULLS_E_INVALID);
	if (!(p.fitness_score_thre >= 0.f) || !std::isfinite(p.fitness_score_thre))
		return bad("a negative or non-finite fitness_score_thre", MULLS_E_INVALID);
	if (p.metrics < MULLS_PCL_ICP_POINT2POINT || p.metrics > MULLS_PCL_ICP_PLANE2PLANE)
		return bad("metrics outside Point2Point .. Plane2Plane", MULLS_E_INVALID);
	if (p.ce < MULLS_PCL_ICP_NN || p.ce > MULLS_PCL_ICP_NS)
		return bad("ce is neither NN nor NS", MULLS_E_INVALID);
	if (p.te < MULLS_PCL_ICP_SVD || p.te > MULLS_PCL_ICP_LLS)
		return bad("te outside SVD .. LLS", MULLS_E_INVALID);
	if (p.metrics == MULLS_PCL_ICP_PLANE2PLANE)
		return bad("metrics = Plane2Plane (PCL's GeneralizedIterativeClosestPoint) is not built", MULLS_E_UNSUPPORTED);
	if (p.te == MULLS_PCL_ICP_LM)
		return bad("te = LM (Levenberg-Marquardt estimation) is not built", MULLS_E_UNSUPPORTED);
	if (p.ce == MULLS_PCL_ICP_NS)
		return bad("ce = NS (normal shooting) is not built", MULLS_E_UNSUPPORTED);
	if (p.use_trimmed_rejector)
		return bad("use_trimmed_rejector (CorrespondenceRejectorVarTrimmed removes the distance bound) is not built", MULLS_E_UNSUPPORTED);
	return MULLS_OK;
}

void lay_out(Plan &L, const mulls_pcl_icp_problem &P, const mulls_pcl_icp_params &prm, reg_host::Arena &take)
{
	const bool plane = prm.metrics == MULLS_PCL_ICP_POINT2PLANE, reciprocal = prm.use_reciprocal_correspondence != 0;
	NdtDesc &N = L.N;
	PclIcpDesc &D = L.D;
	const size_t ns = P.src.n, nt = P.tgt.n;
	N.n_src_in = P.src.n, N.n_tgt_in = P.tgt.n;
	N.o_src_in = take(12 * ns), N.o_tgt_in = take(12 * nt), N.o_src = take(12 * ns), N.o_tgt = take(12 * nt);
	N.o_dist = take(4 * ns);
	D.n_src_cap = P.src.n, D.n_tgt_cap = P.tgt.n;
	D.o_src = N.o_src, D.o_tgt = N.o_tgt, D.o_dist = N.o_dist;
	D.o_mov = take(12 * ns), D.o_match = take(4 * ns), D.o_d2 = take(4 * ns);
	D.o_nrm = plane ? take(12 * nt) : 0;
	for (int tb = 0; tb < PCL_ICP_TABS; tb++)
	{
		RegTab &T = L.tab[tb];
		T = RegTab{};
		// the moved source's table is built again every tick, and a moved point outside the cells' range takes no part
		T.cloud = tb == PCL_ICP_TAB_SRC ? 0 : 1, T.rebuilt = tb == PCL_ICP_TAB_SRC, T.refuses = tb != PCL_ICP_TAB_SRC;
		T.rule = REG_COORD_CELL;
		T.inv_edge = 1.0 / ((double)(tb == PCL_ICP_TAB_NRM ? prm.neighbor_radius : prm.dis_thre_unit) * CELL_MARGIN);
		if ((tb == PCL_ICP_TAB_NRM && !plane) || (tb == PCL_ICP_TAB_SRC && !reciprocal))
			continue;
		reg_table_lay_out(T, T.cloud ? nt : ns, T.cloud ? N.o_tgt : D.o_mov, true, take);
	}
	D.o_partial = take(8ull * pcl_icp::N_SUMS * MULLS_NDT_TREE), D.o_hits = take(4ull * MULLS_NDT_TREE);
}

// one sub-batch: problems idx[0 .. B) of the call
int run_sub_batch(mulls_ctx *ctx, const mulls_pcl_icp_problem *problems, std::vector<Plan> &plans, const uint32_t *idx, uint32_t B, const mulls_pcl_icp_params &prm,
				  const PclIcpOpts &opt, mulls_pcl_icp_result *results, const std::string &who, bool single)
{
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	const bool plane = opt.metric == pcl_icp::POINT2PLANE, reciprocal = opt.reciprocal != 0;
	reg_host::Arena take;
	const size_t ndesc_bytes = sizeof(NdtDesc) * (size_t)B, desc_bytes = sizeof(PclIcpDesc) * (size_t)B, tab_bytes = sizeof(RegTab) * MULLS_REG_TABS * (size_t)B;
	const size_t nrec_bytes = sizeof(NdtRec) * (size_t)B, rec_bytes = sizeof(PclIcpRec) * (size_t)B, head_bytes = sizeof(RegHead) * (size_t)B;
	const size_t o_ndesc = take(ndesc_bytes), o_desc = take(desc_bytes), o_tabs = take(tab_bytes);
	const size_t o_nrec = take(nrec_bytes), o_rec = take(rec_bytes), o_head = take(head_bytes);
	const size_t o_frames = take(96ull * B), o_cnt = take(8);
	uint32_t ns_max = 0, nt_max = 0, slots_max[PCL_ICP_TABS] = {0, 0, 0};
	std::vector<NdtDesc> ndescs(B);
	std::vector<PclIcpDesc> descs(B);
	std::vector<RegTab> tabs_h(MULLS_REG_TABS * (size_t)B);
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_pcl_icp_problem &P = problems[idx[k]];
		Plan &L = plans[idx[k]];
		lay_out(L, P, prm, take);
		ndescs[k] = L.N, descs[k] = L.D;
		for (int tb = 0; tb < PCL_ICP_TABS; tb++)
			tabs_h[MULLS_REG_TABS * (size_t)k + tb] = L.tab[tb], slots_max[tb] = std::max(slots_max[tb], L.tab[tb].slots);
		ns_max = std::max(ns_max, P.src.n), nt_max = std::max(nt_max, P.tgt.n);
	}
	const size_t pin_need = std::max<size_t>({reg_host::pinned_bytes({ndesc_bytes, desc_bytes, tab_bytes}), reg_host::pinned_bytes({rec_bytes, head_bytes}),
											  (size_t)12 * std::max(ns_max, nt_max)});
	unsigned char *d, *h;
	if (int rc = reg_host::reserve(ctx, take.off, pin_need, &d, &h))
		return rc;
	for (uint32_t k = 0; k < B; k++)
		if (int rc = reg_host::upload_problem(ctx, problems[idx[k]], ndescs[k], d, h))
			return rc;
	if (int rc = reg_host::stage(ctx, h, {{d + o_ndesc, ndescs.data(), ndesc_bytes}, {d + o_desc, descs.data(), desc_bytes}, {d + o_tabs, tabs_h.data(), tab_bytes}}))
		return rc;
	HIPCHK(ctx, hipMemsetAsync(d + o_nrec, 0, nrec_bytes, st));
	HIPCHK(ctx, hipMemsetAsync(d + o_cnt, 0, 8, st));
	const NdtDesc *ndesc = reinterpret_cast<const NdtDesc *>(d + o_ndesc);
	const PclIcpDesc *desc = reinterpret_cast<const PclIcpDesc *>(d + o_desc);
	const RegTab *tabs = reinterpret_cast<const RegTab *>(d + o_tabs);
	NdtRec *nrec = reinterpret_cast<NdtRec *>(d + o_nrec);
	PclIcpRec *rec = reinterpret_cast<PclIcpRec *>(d + o_rec); // (written whole by k_pcl_icp_begin, as the heads are)
	RegHead *head = reinterpret_cast<RegHead *>(d + o_head);
	double *frames = reinterpret_cast<double *>(d + o_frames);
	// the setup's launch set: the crop (no NDT grid: a zero inverse resolution puts every point into cell 0), the target's tables, the normals
	NdtOpts nopt{};
	HIPCHK(ctx, launch_ndt_crop(st, ndesc, B, d, nopt, nrec));
	HIPCHK(ctx, launch_pcl_icp_begin(st, desc, tabs, B, ns_max, d, nrec, rec, head, frames));
	HIPCHK(ctx, launch_reg_tables(st, tabs, B, PCL_ICP_TAB_TGT, 1, nt_max, slots_max[PCL_ICP_TAB_TGT], d, head));
	if (plane)
	{
		HIPCHK(ctx, launch_reg_tables(st, tabs, B, PCL_ICP_TAB_NRM, 1, nt_max, slots_max[PCL_ICP_TAB_NRM], d, head));
		HIPCHK(ctx, launch_pcl_icp_normals(st, desc, tabs, B, slots_max[PCL_ICP_TAB_NRM], d, opt, head));
	}
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the descriptors have left the pinned buffer)
	if (int rc = reg_host::tick_loop(ctx, reinterpret_cast<uint32_t *>(d + o_cnt), h, (uint32_t)prm.max_iter_num, [&](uint32_t *running, uint32_t *next) -> int {
			if (reciprocal)
				HIPCHK(ctx, launch_reg_tables(st, tabs, B, PCL_ICP_TAB_SRC, 1, ns_max, slots_max[PCL_ICP_TAB_SRC], d, head));
			HIPCHK(ctx, launch_pcl_icp_search(st, desc, tabs, B, ns_max, d, opt, rec, head));
			HIPCHK(ctx, launch_pcl_icp_accum(st, desc, B, d, opt, rec, head));
			HIPCHK(ctx, launch_pcl_icp_decide(st, desc, B, d, opt, rec, head, frames, running, next));
			return MULLS_OK;
		}))
		return rc;
	HIPCHK(ctx, launch_ndt_fitness(st, ndesc, B, ns_max, d, nrec, frames));
	HIPCHK(ctx, launch_pcl_icp_fitness(st, desc, B, d, opt, rec, head));
	std::vector<PclIcpRec> recs(B);
	std::vector<RegHead> heads(B);
	if (int rc = reg_host::download(ctx, h, {{rec, recs.data(), rec_bytes}, {head, heads.data(), head_bytes}}))
		return rc;
	for (uint32_t k = 0; k < B; k++)
	{
		const bool range = heads[k].status == PCL_ICP_ST_OK && heads[k].range;
		if (heads[k].status == PCL_ICP_ST_NONFINITE || range)
		{
			ctx->err = reg_host::refusal_prefix(who, single, idx[k]) + (range ? "a coordinate lies beyond 2^20 cells" : "a coordinate is not finite");
			return range ? MULLS_E_UNSUPPORTED : MULLS_E_INVALID;
		}
	}
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_pcl_icp_problem &P = problems[idx[k]];
		const Plan &L = plans[idx[k]];
		const PclIcpRec &R = recs[k];
		const RegHead &H = heads[k];
		mulls_pcl_icp_result &res = results[idx[k]];
		std::memset(&res, 0, sizeof(res));
		res.n_src = H.n[0], res.n_tgt = H.n[1];
		if (H.status == PCL_ICP_ST_EMPTY)
		{
			reg_host::idle_pose(P, L.apply_guess, res.T);
			res.fitness = DBL_MAX;
			res.code = -3;
			continue;
		}
		res.n_corr = R.S.n_corr, res.mse = R.S.mse, res.n_fit = R.n_fit;
		res.iterations = R.S.iterations, res.converged = R.S.converged, res.stop = R.S.stop;
		res.fitness = R.fitness;
		res.code = res.fitness > (double)prm.fitness_score_thre ? -3 : 1;
		reg_host::pose_of(R.S.R, R.S.t, P, L.apply_guess, res.T); // T = T_icp guess
	}
	return MULLS_OK;
}

int pcl_icp_run(mulls_ctx *ctx, const mulls_pcl_icp_problem *problems, uint32_t n_problems, const mulls_pcl_icp_params *params, mulls_pcl_icp_result *results,
				const char *name, bool single)
{
	if (!ctx || !params || (n_problems && (!problems || !results)))
		return MULLS_E_INVALID;
	const std::string who = std::string(name) + ": ";
	const char *bad = nullptr;
	if (int rc = check_params(*params, &bad))
	{
		ctx->err = who + bad;
		return rc;
	}
	if (int rc = reg_host::check_problems(ctx, problems, n_problems, who, single))
		return rc;
	if (!n_problems)
		return MULLS_OK;
	PclIcpOpts opt{};
	const double thr = (double)params->dis_thre_unit, radius = (double)params->neighbor_radius;
	opt.thr2 = thr * thr, opt.radius2 = radius * radius, opt.fit_range = thr;
	opt.transformation_epsilon = params->transformation_epsilon, opt.euclidean_fitness_epsilon = params->euclidean_fitness_epsilon;
	opt.metric = params->metrics == MULLS_PCL_ICP_POINT2PLANE ? pcl_icp::POINT2PLANE : pcl_icp::POINT2POINT;
	opt.reciprocal = params->use_reciprocal_correspondence ? 1 : 0, opt.max_iter_num = params->max_iter_num;
	std::vector<Plan> plans(n_problems);
	std::vector<uint64_t> bytes(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
	{
		Plan &L = plans[b];
		L.apply_guess = reg_host::crop_desc(problems[b], params->apply_intersection_filter != 0, L.N);
		reg_host::Arena dry;
		Plan t = L;
		lay_out(t, problems[b], *params, dry);
		bytes[b] = dry.off;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const size_t limit = params->scratch_limit_bytes ? (size_t)params->scratch_limit_bytes : (size_t)MULLS_PCL_ICP_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<mulls_pcl_icp_result> out(n_problems); // (results are written only when the whole call succeeds)
	std::vector<uint32_t> work(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
		work[b] = b;
	const std::vector<uint32_t> cuts = reg_host::cuts_of(bytes, limit);
	for (size_t c = 0; c + 1 < cuts.size(); c++)
		if (int rc = run_sub_batch(ctx, problems, plans, work.data() + cuts[c], cuts[c + 1] - cuts[c], *params, opt, out.data(), who, single))
			return rc;
	std::memcpy(results, out.data(), sizeof(mulls_pcl_icp_result) * (size_t)n_problems);
	return MULLS_OK;
}
} // namespace

extern "C"
{
	void mulls_pcl_icp_default_params(mulls_pcl_icp_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->max_iter_num = 20;
		p->dis_thre_unit = 1.5f;
		p->metrics = MULLS_PCL_ICP_POINT2POINT, p->ce = MULLS_PCL_ICP_NN, p->te = MULLS_PCL_ICP_SVD;
		p->neighbor_radius = 2.0f;
		p->apply_intersection_filter = 1;
		p->fitness_score_thre = 10.0f;
		p->transformation_epsilon = 1e-8;
		p->euclidean_fitness_epsilon = 1e-5;
	}

	int mulls_pcl_icp(mulls_ctx *ctx, const mulls_pcl_icp_problem *problem, const mulls_pcl_icp_params *params, mulls_pcl_icp_result *result)
	try
	{
		if (!problem || !result)
			return MULLS_E_INVALID;
		return pcl_icp_run(ctx, problem, 1, params, result, "mulls_pcl_icp", true);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	int mulls_pcl_icp_batch(mulls_ctx *ctx, const mulls_pcl_icp_problem *problems, uint32_t n_problems, const mulls_pcl_icp_params *params,
							mulls_pcl_icp_result *results)
	try
	{
		return pcl_icp_run(ctx, problems, n_problems, params, results, "mulls_pcl_icp_batch", false);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}
}
