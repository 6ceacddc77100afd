// pcl_icp.cpp — mulls_pcl_icp / mulls_pcl_icp_batch: CRegistration::pcl_icp (cregistration.hpp:882-942) over icp_registration (:84-315), the part that
// is plain ICP.  Host side: argument checks of every problem before any device work, the identity test of the guess, the arena of a sub-batch, the
// uploads, the setup launch set, the lock-step tick loop (k_pcl_icp.hip) and the output pose.  The pre-steps, the crop and the nearest-neighbour pass of
// the fitness are mulls_ndt's (ndt_host.h, ndt_launch.h).  include/mulls_hip.h has the definition this file follows.
#include <cfloat>
#include <cmath>

#include "ctx.h"
#include "ndt_host.h"
#include "pcl_icp_launch.h"
#include "subbatch.h"

// a context's scratch of this entry point: one device arena, one pinned host buffer; grow-only
struct mulls_pcl_icp_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr;
	size_t dev_cap = 0, pin_cap = 0;
};

void mulls_pcl_icp_release(mulls_ctx *ctx)
{
	if (!ctx->pcl_icp)
		return;
	staggered_free(ctx->pcl_icp->dev);
	if (ctx->pcl_icp->pin)
		(void)hipHostFree(ctx->pcl_icp->pin);
	delete ctx->pcl_icp;
	ctx->pcl_icp = nullptr;
}

namespace
{
constexpr uint32_t MAX_SUB_BATCH = 4096u; // problems of one sub-batch (one grid dimension of the per-point launches)
constexpr double CELL_MARGIN = 1.0 + 0x1p-20; // a cell's edge over the distance it serves: the 27-cell walks are exact (include/mulls_hip.h)

struct Plan
{
	bool apply_guess = false;
	size_t bytes = 0;
	NdtDesc N{};
	PclIcpDesc D{};
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

void lay_out(Plan &L, const mulls_pcl_icp_problem &P, bool plane, bool reciprocal, size_t &off)
{
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return (uint64_t)at;
	};
	NdtDesc &N = L.N;
	PclIcpDesc &D = L.D;
	const size_t ns = P.src.n, nt = P.tgt.n;
	N.n_src_in = P.src.n, N.n_tgt_in = P.tgt.n;
	N.o_src_in = take(12 * ns), N.o_tgt_in = take(12 * nt), N.o_src = take(12 * ns), N.o_tgt = take(12 * nt);
	N.o_dist = take(4 * ns);
	D.n_src_cap = P.src.n, D.n_tgt_cap = P.tgt.n;
	D.o_src = N.o_src, D.o_dist = N.o_dist;
	D.o_mov = take(12 * ns), D.o_match = take(4 * ns), D.o_d2 = take(4 * ns);
	D.o_nrm = plane ? take(12 * nt) : 0;
	for (int tb = 0; tb < PCL_ICP_TABS; tb++)
	{
		PclIcpTab &T = D.tab[tb];
		T = PclIcpTab{};
		if ((tb == PCL_ICP_TAB_NRM && !plane) || (tb == PCL_ICP_TAB_SRC && !reciprocal))
			continue;
		const size_t n = tb == PCL_ICP_TAB_SRC ? ns : nt;
		uint32_t slots = MULLS_PCL_ICP_SEG, lg = 10;
		while ((size_t)slots < 2 * n)
			slots <<= 1, lg++;
		T.n_cap = (uint32_t)n, T.slots = slots, T.shift = 64u - lg;
		T.o_pts = tb == PCL_ICP_TAB_SRC ? D.o_mov : N.o_tgt;
		T.o_cell = take(4 * n), T.o_list = take(4 * n), T.o_sorted = take(12 * n);
		T.o_keys = take(8ull * slots);
		T.o_count = take(4ull * slots), T.o_start = take(4ull * slots), T.o_fill = take(4ull * slots); // (contiguous: cleared together)
	}
	D.o_partial = take(8ull * pcl_icp::N_SUMS * MULLS_NDT_TREE), D.o_hits = take(4ull * MULLS_NDT_TREE);
}

void fill_result_idle(const mulls_pcl_icp_problem &P, const Plan &L, mulls_pcl_icp_result &res)
{
	for (int k = 0; k < 16; k++)
		res.T[k] = L.apply_guess ? P.init_guess[k] : (k % 5 == 0 ? 1.0 : 0.0);
	res.fitness = DBL_MAX;
	res.code = -3;
}

// one sub-batch: problems idx[0 .. B) of the call
int run_sub_batch(mulls_ctx *ctx, const mulls_pcl_icp_problem *problems, std::vector<Plan> &plans, const uint32_t *idx, uint32_t B, const mulls_pcl_icp_params &prm,
				  const PclIcpOpts &opt, mulls_pcl_icp_result *results, const std::string &who, bool single)
{
	mulls_pcl_icp_scratch &sc = *ctx->pcl_icp;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	const bool plane = opt.metric == pcl_icp::POINT2PLANE, reciprocal = opt.reciprocal != 0;
	size_t off = 0;
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return at;
	};
	const size_t o_ndesc = take(sizeof(NdtDesc) * (size_t)B), o_desc = take(sizeof(PclIcpDesc) * (size_t)B);
	const size_t o_nrec = take(sizeof(NdtRec) * (size_t)B), o_rec = take(sizeof(PclIcpRec) * (size_t)B);
	const size_t o_frames = take(96ull * B), o_cnt = take(8);
	uint32_t ns_max = 0, nt_max = 0, slots_max[PCL_ICP_TABS] = {0, 0, 0};
	size_t pin_need = std::max(up256(sizeof(NdtDesc) * (size_t)B) + up256(sizeof(PclIcpDesc) * (size_t)B), up256(sizeof(NdtRec) * (size_t)B) + up256(sizeof(PclIcpRec) * (size_t)B));
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_pcl_icp_problem &P = problems[idx[k]];
		Plan &L = plans[idx[k]];
		lay_out(L, P, plane, reciprocal, off);
		ns_max = std::max(ns_max, P.src.n), nt_max = std::max(nt_max, P.tgt.n);
		for (int tb = 0; tb < PCL_ICP_TABS; tb++)
			slots_max[tb] = std::max(slots_max[tb], L.D.tab[tb].slots);
		pin_need = std::max<size_t>(pin_need, 12ull * std::max(P.src.n, P.tgt.n));
	}
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
		return rc;
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, pin_need, hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin;
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_pcl_icp_problem &P = problems[idx[k]];
		const Plan &L = plans[idx[k]];
		if (int rc = ndt_host::upload_cloud(ctx, P.src, d + L.N.o_src_in, h))
			return rc;
		if (int rc = ndt_host::upload_cloud(ctx, P.tgt, d + L.N.o_tgt_in, h))
			return rc;
		for (int tb = 0; tb < PCL_ICP_TAB_SRC; tb++) // (the source's table is cleared on the device, every tick)
		{
			const PclIcpTab &T = L.D.tab[tb];
			if (!T.n_cap)
				continue;
			HIPCHK(ctx, hipMemsetAsync(d + T.o_keys, 0xff, 8ull * T.slots, st));
			HIPCHK(ctx, hipMemsetAsync(d + T.o_count, 0, 3 * up256(4ull * T.slots), st)); // count, start, fill
		}
	}
	{
		NdtDesc *hn = reinterpret_cast<NdtDesc *>(h);
		PclIcpDesc *hd = reinterpret_cast<PclIcpDesc *>(h + up256(sizeof(NdtDesc) * (size_t)B));
		for (uint32_t k = 0; k < B; k++)
			hn[k] = plans[idx[k]].N, hd[k] = plans[idx[k]].D;
		HIPCHK(ctx, hipMemcpyAsync(d + o_ndesc, hn, sizeof(NdtDesc) * (size_t)B, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, hipMemcpyAsync(d + o_desc, hd, sizeof(PclIcpDesc) * (size_t)B, hipMemcpyHostToDevice, st));
	}
	HIPCHK(ctx, hipMemsetAsync(d + o_nrec, 0, sizeof(NdtRec) * (size_t)B, st));
	HIPCHK(ctx, hipMemsetAsync(d + o_rec, 0, sizeof(PclIcpRec) * (size_t)B, st));
	HIPCHK(ctx, hipMemsetAsync(d + o_cnt, 0, 8, st));
	const NdtDesc *ndesc = reinterpret_cast<const NdtDesc *>(d + o_ndesc);
	const PclIcpDesc *desc = reinterpret_cast<const PclIcpDesc *>(d + o_desc);
	NdtRec *nrec = reinterpret_cast<NdtRec *>(d + o_nrec);
	PclIcpRec *rec = reinterpret_cast<PclIcpRec *>(d + o_rec);
	double *frames = reinterpret_cast<double *>(d + o_frames);
	uint32_t *cnt = reinterpret_cast<uint32_t *>(d + o_cnt); // [tick & 1]: the problems still running after the tick
	// the setup's launch set: the crop (no NDT grid: a zero inverse resolution puts every point into cell 0), the target's tables, the normals
	NdtOpts nopt{};
	HIPCHK(ctx, launch_ndt_crop(st, ndesc, B, d, nopt, nrec));
	HIPCHK(ctx, launch_pcl_icp_begin(st, desc, B, ns_max, d, opt, nrec, rec, frames));
	HIPCHK(ctx, launch_pcl_icp_table(st, desc, B, PCL_ICP_TAB_TGT, nt_max, slots_max[PCL_ICP_TAB_TGT], false, d, opt, rec));
	if (plane)
	{
		HIPCHK(ctx, launch_pcl_icp_table(st, desc, B, PCL_ICP_TAB_NRM, nt_max, slots_max[PCL_ICP_TAB_NRM], false, d, opt, rec));
		HIPCHK(ctx, launch_pcl_icp_normals(st, desc, B, slots_max[PCL_ICP_TAB_NRM], d, opt, rec));
	}
	uint32_t *h_word = reinterpret_cast<uint32_t *>(h);
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the descriptors have left the pinned buffer)
	for (uint32_t tick = 0; tick < (uint32_t)prm.max_iter_num; tick++)
	{
		if (reciprocal)
			HIPCHK(ctx, launch_pcl_icp_table(st, desc, B, PCL_ICP_TAB_SRC, ns_max, slots_max[PCL_ICP_TAB_SRC], true, d, opt, rec));
		HIPCHK(ctx, launch_pcl_icp_search(st, desc, B, ns_max, d, opt, rec));
		HIPCHK(ctx, launch_pcl_icp_accum(st, desc, B, d, opt, rec));
		HIPCHK(ctx, launch_pcl_icp_decide(st, desc, B, d, opt, rec, frames, cnt + (tick & 1u), cnt + ((tick + 1u) & 1u)));
		HIPCHK(ctx, hipMemcpyAsync(h_word, cnt + (tick & 1u), 4, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		if (*h_word == 0)
			break;
	}
	HIPCHK(ctx, launch_ndt_fitness(st, ndesc, B, ns_max, d, nrec, frames));
	HIPCHK(ctx, launch_pcl_icp_fitness(st, desc, B, d, opt, rec));
	std::vector<PclIcpRec> recs(B);
	HIPCHK(ctx, hipMemcpyAsync(h, rec, sizeof(PclIcpRec) * (size_t)B, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::memcpy(recs.data(), h, sizeof(PclIcpRec) * (size_t)B);
	for (uint32_t k = 0; k < B; k++)
	{
		const bool range = recs[k].status == PCL_ICP_ST_OK && recs[k].range;
		if (recs[k].status == PCL_ICP_ST_NONFINITE || range)
		{
			ctx->err = who + (single ? std::string() : "problem " + std::to_string(idx[k]) + ": ") +
					   (range ? "a coordinate lies beyond 2^20 cells" : "a coordinate is not finite");
			return range ? MULLS_E_UNSUPPORTED : MULLS_E_INVALID;
		}
	}
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_pcl_icp_problem &P = problems[idx[k]];
		const Plan &L = plans[idx[k]];
		const PclIcpRec &R = recs[k];
		mulls_pcl_icp_result &res = results[idx[k]];
		std::memset(&res, 0, sizeof(res));
		res.n_src = R.n[0], res.n_tgt = R.n[1];
		if (R.status == PCL_ICP_ST_EMPTY)
		{
			fill_result_idle(P, L, res);
			continue;
		}
		res.n_corr = R.S.n_corr, res.mse = R.S.mse, res.n_fit = R.n_fit;
		res.iterations = R.S.iterations, res.converged = R.S.converged, res.stop = R.S.stop;
		res.fitness = R.fitness;
		res.code = res.fitness > (double)prm.fitness_score_thre ? -3 : 1;
		// T = T_icp guess
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
	PclIcpOpts opt{};
	const double thr = (double)params->dis_thre_unit, radius = (double)params->neighbor_radius;
	opt.inv_edge[PCL_ICP_TAB_TGT] = opt.inv_edge[PCL_ICP_TAB_SRC] = 1.0 / (thr * CELL_MARGIN);
	opt.inv_edge[PCL_ICP_TAB_NRM] = 1.0 / (radius * CELL_MARGIN);
	opt.thr2 = thr * thr, opt.radius2 = radius * radius, opt.fit_range = thr;
	opt.transformation_epsilon = params->transformation_epsilon, opt.euclidean_fitness_epsilon = params->euclidean_fitness_epsilon;
	opt.metric = params->metrics == MULLS_PCL_ICP_POINT2PLANE ? pcl_icp::POINT2PLANE : pcl_icp::POINT2POINT;
	opt.reciprocal = params->use_reciprocal_correspondence ? 1 : 0, opt.max_iter_num = params->max_iter_num;
	for (uint32_t b = 0; b < n_problems; b++)
	{
		const mulls_pcl_icp_problem &P = problems[b];
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
		lay_out(t, P, opt.metric == pcl_icp::POINT2PLANE, opt.reciprocal != 0, off);
		L.bytes = off;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (!ctx->pcl_icp)
		ctx->pcl_icp = new mulls_pcl_icp_scratch();
	const size_t limit = params->scratch_limit_bytes ? (size_t)params->scratch_limit_bytes : (size_t)MULLS_PCL_ICP_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<mulls_pcl_icp_result> out(n_problems); // (results are written only when the whole call succeeds)
	std::vector<uint32_t> work(n_problems), cuts;
	std::vector<uint64_t> bytes(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
		work[b] = b, bytes[b] = plans[b].bytes;
	sub_batch_cuts(bytes.data(), n_problems, limit, MAX_SUB_BATCH, &cuts);
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
