// ndt.cpp — mulls_ndt / mulls_ndt_batch: CRegistration::omp_ndt (cregistration.hpp:945-1021) with what it calls.  Host side: argument checks of every
// problem before any device work, the identity test of the guess, the score constants, the arena of a sub-batch, the uploads, the lock-step tick loop
// (k_ndt.hip) and the output pose.  include/mulls_hip.h has the definition this file follows.
#include <cfloat>
#include <cmath>

#include "ctx.h"
#include "ndt_host.h"
#include "ndt_launch.h"
#include "subbatch.h"

// a context's scratch of this entry point: one device arena, one pinned host buffer; grow-only
struct mulls_ndt_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr;
	size_t dev_cap = 0, pin_cap = 0;
};

void mulls_ndt_release(mulls_ctx *ctx)
{
	if (!ctx->ndt)
		return;
	staggered_free(ctx->ndt->dev);
	if (ctx->ndt->pin)
		(void)hipHostFree(ctx->ndt->pin);
	delete ctx->ndt;
	ctx->ndt = nullptr;
}

// what mulls_gicp shares with this file (ndt_host.h): the pre-steps of omp_ndt and omp_gicp are the same text upstream
namespace ndt_host
{
bool cloud_on_device(mulls_ctx *ctx, const mulls_cloud &c)
{
	if (mulls_is_map_memory(ctx, c.pts, (size_t)c.n * c.stride))
		return true;
	hipPointerAttribute_t at;
	std::memset(&at, 0, sizeof(at));
	if (hipPointerGetAttributes(&at, c.pts) == hipSuccess)
		return at.type == hipMemoryTypeDevice;
	(void)hipGetLastError(); // (an ordinary host pointer: the query reports an error on some runtimes — cleared)
	return false;
}

// Eigen's isIdentity(prec) of a column-major 4 x 4
bool is_identity(const double *G, double prec)
{
	for (int c = 0; c < 4; c++)
		for (int r = 0; r < 4; r++)
		{
			const double v = G[r + 4 * c];
			if (r == c)
			{
				if (!(std::fabs(v - 1.0) <= std::min(std::fabs(v), 1.0) * prec))
					return false;
			}
			else if (!(std::fabs(v) <= prec))
				return false;
		}
	return true;
}

int check_problem(const mulls_ndt_problem &P, std::string &msg)
{
	const mulls_cloud *cl[2] = {&P.tgt, &P.src};
	for (int k = 0; k < 2; k++)
	{
		const char *name = k ? "the source" : "the target";
		if (cl[k]->n == 0)
		{
			msg = std::string(name) + " is empty";
			return MULLS_E_INVALID;
		}
		if (!cl[k]->pts)
		{
			msg = std::string(name) + " is NULL";
			return MULLS_E_INVALID;
		}
		if (cl[k]->stride < 12 || cl[k]->stride % 4)
		{
			msg = std::string(name) + " has a stride below 12 or not a multiple of 4";
			return MULLS_E_INVALID;
		}
		if (cl[k]->n > MULLS_NDT_MAX_POINTS)
		{
			msg = std::string(name) + " has more than 2^24 points";
			return MULLS_E_UNSUPPORTED;
		}
	}
	for (int k = 0; k < 16; k++)
		if (!std::isfinite(P.init_guess[k]))
		{
			msg = "init_guess is not finite";
			return MULLS_E_INVALID;
		}
	for (int k = 0; k < 6; k++)
		if (!std::isfinite(P.tgt_bound[k]) || !std::isfinite(P.src_bound[k]))
		{
			msg = "a bound is not finite";
			return MULLS_E_INVALID;
		}
	return MULLS_OK;
}

// the coordinates of a cloud, packed to 12 bytes a point, into the arena (a host cloud through the pinned buffer, a device cloud by a strided copy)
int upload_cloud(mulls_ctx *ctx, const mulls_cloud &c, unsigned char *dst, unsigned char *pinned)
{
	hipStream_t st = ctx->stream;
	if (cloud_on_device(ctx, c))
		HIPCHK(ctx, hipMemcpy2DAsync(dst, 12, c.pts, c.stride, 12, c.n, hipMemcpyDeviceToDevice, st));
	else
	{
		const unsigned char *src = static_cast<const unsigned char *>(c.pts);
		for (uint32_t i = 0; i < c.n; i++)
			std::memcpy(pinned + 12ull * i, src + (size_t)i * c.stride, 12);
		HIPCHK(ctx, hipMemcpyAsync(dst, pinned, 12ull * c.n, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, hipStreamSynchronize(st)); // (the pinned buffer is reused)
	}
	return MULLS_OK;
}

// T = Tn * G (column-major 4 x 4, G = NULL: the identity)
void pose_times_guess(const double *Tn, const double *G, double *T)
{
	if (!G)
	{
		std::memcpy(T, Tn, 16 * sizeof(double));
		return;
	}
	for (int r = 0; r < 4; r++)
		for (int c = 0; c < 4; c++)
			T[r + 4 * c] = ((Tn[r] * G[4 * c] + Tn[r + 4] * G[1 + 4 * c]) + Tn[r + 8] * G[2 + 4 * c]) + Tn[r + 12] * G[3 + 4 * c];
}
} // namespace ndt_host

namespace
{
using namespace ndt_host;
constexpr uint32_t MAX_SUB_BATCH = 4096u; // problems of one sub-batch (one grid dimension of the per-point launches)

struct Plan
{
	bool apply_guess = false;
	size_t bytes = 0;
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

void lay_out(Plan &L, const mulls_ndt_problem &P, size_t &off)
{
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return (uint64_t)at;
	};
	NdtDesc &D = L.D;
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

void fill_result_idle(const mulls_ndt_problem &P, const Plan &L, mulls_ndt_result &res)
{
	for (int k = 0; k < 16; k++)
		res.T[k] = L.apply_guess ? P.init_guess[k] : (k % 5 == 0 ? 1.0 : 0.0);
	res.fitness = DBL_MAX;
	res.code = -3;
}

// one sub-batch: problems idx[0 .. B) of the call
int run_sub_batch(mulls_ctx *ctx, const mulls_ndt_problem *problems, std::vector<Plan> &plans, const uint32_t *idx, uint32_t B, const mulls_ndt_params &prm,
				  const NdtOpts &opt, mulls_ndt_result *results, const std::string &who, bool single)
{
	mulls_ndt_scratch &sc = *ctx->ndt;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	// the first evaluation, then per Newton iteration (at most max_iterations + 2 of them) one trial, the inner steps and the Hessian pass
	const uint32_t max_ticks = (uint32_t)(prm.max_iterations + 2) * (uint32_t)(prm.max_step_iterations + 2) + 1u;
	size_t off = 0;
	const size_t o_desc = off;
	off += up256(sizeof(NdtDesc) * (size_t)B);
	const size_t o_rec = off;
	off += up256(sizeof(NdtRec) * (size_t)B);
	const size_t o_cnt = off;
	off += up256(4ull * (max_ticks + 1u));
	uint32_t ns_max = 0, nt_max = 0, table_max = 0;
	size_t pin_need = std::max(up256(sizeof(NdtDesc) * (size_t)B), up256(sizeof(NdtRec) * (size_t)B));
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_ndt_problem &P = problems[idx[k]];
		Plan &L = plans[idx[k]];
		lay_out(L, P, off);
		ns_max = std::max(ns_max, P.src.n), nt_max = std::max(nt_max, P.tgt.n), table_max = std::max(table_max, L.D.table_size);
		pin_need = std::max<size_t>(pin_need, 12ull * std::max(P.src.n, P.tgt.n));
	}
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
		return rc;
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, pin_need, hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin;
	// up: the clouds' coordinates, packed (a host cloud through the pinned buffer, a device cloud by a strided copy), and the empty hash tables
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_ndt_problem &P = problems[idx[k]];
		const NdtDesc &D = plans[idx[k]].D;
		if (int rc = ndt_host::upload_cloud(ctx, P.src, d + D.o_src_in, h))
			return rc;
		if (int rc = ndt_host::upload_cloud(ctx, P.tgt, d + D.o_tgt_in, h))
			return rc;
		HIPCHK(ctx, hipMemsetAsync(d + D.o_keys, 0xff, 4ull * D.table_size, st));
		HIPCHK(ctx, hipMemsetAsync(d + D.o_count, 0, D.o_leaves - D.o_count, st)); // count, start, fill
	}
	{
		NdtDesc *hd = reinterpret_cast<NdtDesc *>(h);
		for (uint32_t k = 0; k < B; k++)
			hd[k] = plans[idx[k]].D;
		HIPCHK(ctx, hipMemcpyAsync(d + o_desc, h, sizeof(NdtDesc) * (size_t)B, hipMemcpyHostToDevice, st));
	}
	HIPCHK(ctx, hipMemsetAsync(d + o_rec, 0, sizeof(NdtRec) * (size_t)B, st));
	HIPCHK(ctx, hipMemsetAsync(d + o_cnt, 0, 4ull * (max_ticks + 1u), st));
	const NdtDesc *desc = reinterpret_cast<const NdtDesc *>(d + o_desc);
	NdtRec *rec = reinterpret_cast<NdtRec *>(d + o_rec);
	uint32_t *cnt = reinterpret_cast<uint32_t *>(d + o_cnt);
	HIPCHK(ctx, launch_ndt_crop(st, desc, B, d, opt, rec));
	HIPCHK(ctx, launch_ndt_cells(st, desc, B, nt_max, d, opt, rec));
	HIPCHK(ctx, launch_ndt_offsets(st, desc, B, d, rec));
	HIPCHK(ctx, launch_ndt_scatter(st, desc, B, nt_max, d, rec));
	HIPCHK(ctx, launch_ndt_leaves(st, desc, B, table_max, d, opt, rec));
	HIPCHK(ctx, launch_ndt_begin(st, B, rec));
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the descriptors have left the pinned buffer)
	uint32_t *h_running = reinterpret_cast<uint32_t *>(h);
	for (uint32_t tick = 0; tick < max_ticks; tick++)
	{
		HIPCHK(ctx, launch_ndt_eval(st, desc, B, d, opt, rec));
		HIPCHK(ctx, launch_ndt_decide(st, desc, B, d, opt, rec, cnt + tick));
		HIPCHK(ctx, hipMemcpyAsync(h_running, cnt + tick, 4, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		if (*h_running == 0)
			break;
	}
	HIPCHK(ctx, launch_ndt_fitness(st, desc, B, ns_max, d, rec, nullptr));
	std::vector<NdtRec> recs(B);
	HIPCHK(ctx, hipMemcpyAsync(h, rec, sizeof(NdtRec) * (size_t)B, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::memcpy(recs.data(), h, sizeof(NdtRec) * (size_t)B);
	for (uint32_t k = 0; k < B; k++)
		if (recs[k].status == NDT_ST_NONFINITE || recs[k].status == NDT_ST_GRID)
		{
			ctx->err = who + (single ? std::string() : "problem " + std::to_string(idx[k]) + ": ") +
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
			fill_result_idle(P, L, res);
			continue;
		}
		res.n_leaves = R.n_leaves, res.n_leaves_used = R.n_leaves_used;
		res.iterations = R.S.nr_iterations, res.evaluations = R.S.evaluations, res.converged = R.S.converged;
		res.line_search_reversals = R.S.reversals, res.inner_steps = R.S.inner_steps;
		res.trans_probability = R.S.trans_probability;
		res.fitness = R.fitness;
		res.code = res.fitness > (double)prm.fitness_score_thre ? -3 : 1;
		// T = T(p) guess
		ndt::Frame F;
		ndt::make_frame(R.S.p, &F);
		double Tn[16] = {0};
		for (int r = 0; r < 3; r++)
		{
			for (int c = 0; c < 3; c++)
				Tn[r + 4 * c] = F.R[3 * r + c];
			Tn[r + 12] = F.t[r];
		}
		Tn[15] = 1.0;
		ndt_host::pose_times_guess(Tn, L.apply_guess ? P.init_guess : nullptr, res.T);
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
	std::vector<Plan> plans(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
	{
		std::string msg;
		if (int rc = check_problem(problems[b], msg))
		{
			ctx->err = who + (single ? std::string() : "problem " + std::to_string(b) + ": ") + msg;
			return rc;
		}
	}
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
	for (uint32_t b = 0; b < n_problems; b++)
	{
		const mulls_ndt_problem &P = problems[b];
		Plan &L = plans[b];
		NdtDesc &D = L.D;
		L.apply_guess = !is_identity(P.init_guess, 1e-6);
		D.apply_guess = L.apply_guess ? 1 : 0, D.crop = params->apply_intersection_filter ? 1 : 0;
		D.n_offsets = params->search_method == MULLS_NDT_DIRECT1 ? 1 : (params->search_method == MULLS_NDT_DIRECT7 ? 7 : 26);
		D.offset_first = params->search_method == MULLS_NDT_DIRECT26 ? 7 : 0;
		for (int r = 0; r < 3; r++)
		{
			for (int c = 0; c < 3; c++)
				D.G[3 * r + c] = P.init_guess[r + 4 * c];
			D.G[9 + r] = P.init_guess[12 + r];
		}
		std::memcpy(D.tgt_bound, P.tgt_bound, sizeof(D.tgt_bound)), std::memcpy(D.src_bound, P.src_bound, sizeof(D.src_bound));
		size_t off = 0;
		Plan t = L;
		lay_out(t, P, off);
		L.bytes = off;
		mulls_ndt_result &res = results[b];
		std::memset(&res, 0, sizeof(res));
		res.gauss_d1 = d1, res.gauss_d2 = d2, res.gauss_d3 = d3;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (!ctx->ndt)
		ctx->ndt = new mulls_ndt_scratch();
	const size_t limit = params->scratch_limit_bytes ? (size_t)params->scratch_limit_bytes : (size_t)MULLS_NDT_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<uint32_t> work(n_problems), cuts;
	std::vector<uint64_t> bytes(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
		work[b] = b, bytes[b] = plans[b].bytes;
	sub_batch_cuts(bytes.data(), n_problems, limit, MAX_SUB_BATCH, &cuts);
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
