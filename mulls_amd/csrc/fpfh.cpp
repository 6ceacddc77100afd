// fpfh.cpp — mulls_fpfh (CRegistration::compute_fpfh_feature, cregistration.hpp:351-369) and mulls_coarse_reg_fpfhsac (coarse_reg_fpfhsac, :372-406).
// Host side: the argument checks before any device work, the arena, the uploads, the launch sets of k_fpfh.hip and the results.  The cell tables are
// the registrations' (reg_launch.h), the sub-batch arena, staging and downloads reg_host.h's, the nearest-target pass mulls_ndt's (ndt_launch.h), the
// draws fpfh_math.h's.  include/mulls_hip.h has the definition this file follows.  mulls_compute_fpfh_batch and mulls_coarse_reg_fpfhsac_batch: the same
// frame over a sub-batch's distinct clouds and its problems in lock step (k_fpfh_batch.hip; the cuts and the stretches of hypotheses are fpfh_batch.h's).
#include <cmath>
#include <cstring>

#include "ctx.h"
#include "fpfh_batch.h"
#include "fpfh_launch.h"
#include "reg_host.h"

namespace
{
constexpr double CELL_MARGIN = 1.0 + 0x1p-20; // a cell's edge over the radius it serves: the 27-cell walks are exact (include/mulls_hip.h)

struct CloudPlan
{
	FpfhDesc D{};
	RegTab tab[MULLS_REG_TABS]{};
	RegHead H{};
};

int check_cloud(const mulls_cloud *c, const char *name, uint32_t least, std::string &msg)
{
	if (!c || (c->n && !c->pts))
	{
		msg = std::string(name) + " is NULL";
		return MULLS_E_INVALID;
	}
	if (c->n < least)
	{
		msg = std::string(name) + " has fewer than " + std::to_string(least) + (least == 1 ? " point" : " points");
		return MULLS_E_INVALID;
	}
	if (c->stride < 28 || c->stride % 4)
	{
		msg = std::string(name) + " has a stride below 28 (the normal ends there) or not a multiple of 4";
		return MULLS_E_INVALID;
	}
	if (c->n > MULLS_NDT_MAX_POINTS)
	{
		msg = std::string(name) + " has more than 2^24 points";
		return MULLS_E_UNSUPPORTED;
	}
	return MULLS_OK;
}

void lay_out(CloudPlan &L, uint32_t n, float r, reg_host::Arena &take)
{
	FpfhDesc &D = L.D;
	const size_t m = n;
	D.n = n;
	D.o_pts = take(12 * m), D.o_nrm = take(12 * m), D.o_cpts = take(12 * m), D.o_cnrm = take(12 * m);
	D.o_spfh = take(4 * MULLS_FPFH_DIMS * m), D.o_hist = take(4 * MULLS_FPFH_DIMS * m), D.o_k = take(4 * m);
	RegTab &T = L.tab[0];
	T.cloud = 0, T.rule = REG_COORD_CELL, T.refuses = 1, T.rebuilt = 0;
	T.inv_edge = 1.0 / ((double)r * CELL_MARGIN);
	reg_table_lay_out(T, n, D.o_pts, false, take);
	L.H.n[0] = n;
}

// the descriptors of C clouds in one launch set (C <= fpfh_batch::MAX_CLOUDS: blockIdx.y is the cloud)
struct Features
{
	uint32_t C = 0;
	std::vector<CloudPlan> plan;
	size_t o_desc = 0, o_tabs = 0, o_head = 0;
	uint32_t n_max = 0, slots_max = 0;
	void lay_out_all(const mulls_cloud *const *clouds, uint32_t count, float r, reg_host::Arena &take)
	{
		C = count;
		plan.assign(C, CloudPlan());
		o_desc = take(sizeof(FpfhDesc) * C), o_tabs = take(sizeof(RegTab) * MULLS_REG_TABS * C), o_head = take(sizeof(RegHead) * C);
		for (uint32_t c = 0; c < C; c++)
		{
			lay_out(plan[c], clouds[c]->n, r, take);
			n_max = std::max(n_max, clouds[c]->n), slots_max = std::max(slots_max, plan[c].tab[0].slots);
		}
	}
	size_t staged() const { return reg_host::pinned_bytes({sizeof(FpfhDesc) * C, sizeof(RegTab) * MULLS_REG_TABS * C, sizeof(RegHead) * C}); }
	// the uploads (a cloud's coordinates and its normals: two packed copies), the staging of the descriptors and the launch set; nothing waits for the
	// launches: read_heads() does, and until then the pinned buffer holds the descriptors
	int run(mulls_ctx *ctx, const mulls_cloud *const *clouds, float r, unsigned char *d, unsigned char *h, reg_host::Block more = {nullptr, nullptr, 0})
	{
		for (uint32_t c = 0; c < C; c++)
		{
			if (int rc = reg_host::upload_xyz(ctx, *clouds[c], 0, d + plan[c].D.o_pts, h))
				return rc;
			if (int rc = reg_host::upload_xyz(ctx, *clouds[c], 16, d + plan[c].D.o_nrm, h))
				return rc;
		}
		std::vector<FpfhDesc> descs_v(C);
		std::vector<RegTab> tabs_v((size_t)MULLS_REG_TABS * C);
		std::vector<RegHead> heads_v(C);
		FpfhDesc *descs = descs_v.data();
		RegTab *tabs = tabs_v.data();
		RegHead *heads = heads_v.data();
		for (uint32_t c = 0; c < C; c++)
		{
			descs[c] = plan[c].D, heads[c] = plan[c].H;
			for (int tb = 0; tb < MULLS_REG_TABS; tb++)
				tabs[MULLS_REG_TABS * c + tb] = plan[c].tab[tb];
		}
		// one staging copy set for all tables: the clouds' and, for a sub-batch of problems, its problem table (more)
		const reg_host::Block own[3] = {{d + o_desc, descs, sizeof(FpfhDesc) * C}, {d + o_tabs, tabs, sizeof(RegTab) * MULLS_REG_TABS * C}, {d + o_head, heads, sizeof(RegHead) * C}};
		if (int rc = more.bytes ? reg_host::stage(ctx, h, {own[0], own[1], own[2], more}) : reg_host::stage(ctx, h, {own[0], own[1], own[2]}))
			return rc;
		const double r2 = (double)r * (double)r;
		HIPCHK(ctx, launch_fpfh_features(ctx->stream, reinterpret_cast<const FpfhDesc *>(d + o_desc), reinterpret_cast<const RegTab *>(d + o_tabs), C, n_max, slots_max, d,
										 r2, reinterpret_cast<RegHead *>(d + o_head)));
		return MULLS_OK;
	}
	// waits for the launch set; -> the clouds' heads
	int read_heads(mulls_ctx *ctx, unsigned char *d, unsigned char *h, RegHead *heads) const
	{
		return reg_host::download(ctx, h, {{d + o_head, heads, sizeof(RegHead) * C}});
	}
	// what the device found wrong with a cloud, after the heads came back
	int refusal(mulls_ctx *ctx, const RegHead *heads, const std::string &who, const char *const *names, uint32_t count) const
	{
		for (uint32_t c = 0; c < count; c++)
			if (heads[c].range)
			{
				const uint32_t f = heads[c].range;
				ctx->err = who + names[c] +
						   (f & MULLS_FPFH_NONFINITE ? ": a coordinate or a normal is not finite"
							: f & MULLS_FPFH_RANGE   ? ": a coordinate lies beyond 2^20 cells"
													 : ": a cell of the feature radius holds more than MULLS_FPFH_MAX_CELL_POINTS points");
				return f & MULLS_FPFH_NONFINITE ? MULLS_E_INVALID : MULLS_E_UNSUPPORTED;
			}
		return MULLS_OK;
	}
};

bool good_radius(float r) { return r > 0.f && std::isfinite(r) && std::isfinite(2.0f * r); }

int fpfh_run(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_fpfh_params *params, float *hist, uint32_t *n_neighbours)
{
	if (!ctx || !params || !hist)
		return MULLS_E_INVALID;
	const std::string who = "mulls_fpfh: ";
	if (!good_radius(params->search_radius))
	{
		ctx->err = who + "search_radius is not a positive number";
		return MULLS_E_INVALID;
	}
	std::string msg;
	if (int rc = check_cloud(cloud, "the cloud", 1, msg))
	{
		ctx->err = who + msg;
		return rc;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	mulls::StreamDrain drain{ctx->stream};
	const float r = 2.0f * params->search_radius;
	reg_host::Arena take;
	Features F;
	F.lay_out_all(&cloud, 1, r, take);
	unsigned char *d, *h;
	if (int rc = reg_host::reserve(ctx, take.off, std::max<size_t>(F.staged(), 12ull * cloud->n), &d, &h))
		return rc;
	if (int rc = F.run(ctx, &cloud, r, d, h))
		return rc;
	RegHead head;
	if (int rc = F.read_heads(ctx, d, h, &head))
		return rc;
	const char *names[1] = {"the cloud"};
	if (int rc = F.refusal(ctx, &head, who, names, 1))
		return rc;
	HIPCHK(ctx, hipMemcpyAsync(hist, d + F.plan[0].D.o_hist, 4ull * MULLS_FPFH_DIMS * cloud->n, hipMemcpyDefault, ctx->stream));
	if (n_neighbours)
		HIPCHK(ctx, hipMemcpyAsync(n_neighbours, d + F.plan[0].D.o_k, 4ull * cloud->n, hipMemcpyDefault, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return MULLS_OK;
}

int check_params(const mulls_fpfhsac_params &p, const char **msg)
{
	auto bad = [&](const char *m, int rc) {
		*msg = m;
		return rc;
	};
	if (!good_radius(p.search_radius))
		return bad("search_radius is not a positive number", MULLS_E_INVALID);
	if (p.nr_samples < 1)
		return bad("nr_samples below 1", MULLS_E_INVALID);
	if (p.k_correspondences < 1 || p.k_correspondences > 64)
		return bad("k_correspondences outside 1 .. 64", MULLS_E_INVALID);
	if (p.max_iterations < 1)
		return bad("max_iterations below 1", MULLS_E_INVALID);
	if (!(p.min_sample_distance >= 0.f) || !std::isfinite(p.min_sample_distance))
		return bad("a negative or non-finite min_sample_distance", MULLS_E_INVALID);
	if (!(p.max_correspondence_distance > 0.f))
		return bad("max_correspondence_distance is not above 0 (+inf is allowed)", MULLS_E_INVALID);
	if (p.error_function != MULLS_SACIA_TRUNCATED && p.error_function != MULLS_SACIA_HUBER)
		return bad("error_function is neither TRUNCATED nor HUBER", MULLS_E_INVALID);
	if (p.nr_samples != 3)
		return bad("nr_samples other than 3 is not built", MULLS_E_UNSUPPORTED);
	if (p.max_iterations > 65536)
		return bad("max_iterations above 65536 is not built", MULLS_E_UNSUPPORTED);
	return MULLS_OK;
}

// the result of a problem from what the device left of it
mulls_fpfhsac_result result_of(const FpfhSacOut &O, double fitness, uint32_t iters, uint32_t ns, uint32_t nt)
{
	mulls_fpfhsac_result res;
	std::memset(&res, 0, sizeof(res));
	res.best_iteration = O.best, res.iterations = (int32_t)iters, res.n_src = ns, res.n_tgt = nt;
	res.best_error = O.error, res.fitness = fitness;
	for (int rr = 0; rr < 3; rr++)
	{
		for (int c = 0; c < 3; c++)
			res.T[rr + 4 * c] = O.frame[3 * rr + c];
		res.T[12 + rr] = O.frame[9 + rr];
	}
	res.T[15] = 1.0;
	return res;
}

int fpfhsac_run(mulls_ctx *ctx, const mulls_cloud *tgt, const mulls_cloud *src, const mulls_fpfhsac_params *params, mulls_fpfhsac_result *result)
{
	if (!ctx || !params || !result)
		return MULLS_E_INVALID;
	const std::string who = "mulls_coarse_reg_fpfhsac: ";
	const char *bad = nullptr;
	if (int rc = check_params(*params, &bad))
	{
		ctx->err = who + bad;
		return rc;
	}
	std::string msg;
	if (int rc = check_cloud(src, "the source", 3, msg))
	{
		ctx->err = who + msg;
		return rc;
	}
	if (int rc = check_cloud(tgt, "the target", 1, msg))
	{
		ctx->err = who + msg;
		return rc;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	const float r = 2.0f * params->search_radius;
	const uint32_t ns = src->n, nt = tgt->n, iters = (uint32_t)params->max_iterations, n_samples = 3u * iters;
	const uint32_t k_eff = std::min<uint32_t>((uint32_t)params->k_correspondences, nt);
	const uint32_t chunk = std::max<uint32_t>(1u, std::min<uint32_t>({iters, MULLS_FPFH_HYP_CHUNK, (64u << 20) / ns}));
	const mulls_cloud *clouds[2] = {src, tgt};
	reg_host::Arena take;
	Features F;
	F.lay_out_all(clouds, 2, r, take);
	const size_t idx_bytes = 4ull * n_samples;
	const size_t o_samples = take(idx_bytes), o_ranks = take(idx_bytes), o_corr = take(idx_bytes);
	const size_t o_frames = take(96ull * iters), o_err = take(8ull * iters), o_out = take(sizeof(FpfhSacOut));
	const size_t o_ndesc = take(sizeof(NdtDesc) * (size_t)chunk), o_nrec = take(sizeof(NdtRec) * (size_t)chunk), o_dist = take(4ull * ns * chunk);
	const size_t pin_need = std::max<size_t>({F.staged(), 12ull * std::max(ns, nt), reg_host::pinned_bytes({idx_bytes, idx_bytes}),
											  reg_host::pinned_bytes({sizeof(RegHead) * 2, sizeof(FpfhSacOut), sizeof(NdtRec)})});
	unsigned char *d, *h;
	if (int rc = reg_host::reserve(ctx, take.off, pin_need, &d, &h))
		return rc;
	if (int rc = F.run(ctx, clouds, r, d, h))
		return rc;
	// The draws, from the source's packed coordinates.  A host source: drawn while the descriptors' launch set runs.  A device source: its coordinates
	// come back with the heads, and the draws follow.
	std::vector<float> xyz(3 * (size_t)ns);
	std::vector<int32_t> samples, ranks;
	const bool src_on_device = reg_host::on_device(ctx, *src);
	if (src_on_device)
		HIPCHK(ctx, hipMemcpyAsync(xyz.data(), d + F.plan[0].D.o_pts, 12ull * ns, hipMemcpyDeviceToHost, st));
	else
	{
		for (uint32_t i = 0; i < ns; i++)
			std::memcpy(&xyz[3 * (size_t)i], static_cast<const unsigned char *>(src->pts) + (size_t)i * src->stride, 12);
		(void)fpfh::draw_all(xyz.data(), ns, k_eff, 3, (int)iters, params->min_sample_distance, params->seed, samples, ranks);
	}
	// the clouds' refusals, before anything else is launched
	RegHead heads[2];
	if (int rc = F.read_heads(ctx, d, h, heads))
		return rc;
	const char *names[2] = {"the source", "the target"};
	if (int rc = F.refusal(ctx, heads, who, names, 2))
		return rc;
	if (src_on_device)
		(void)fpfh::draw_all(xyz.data(), ns, k_eff, 3, (int)iters, params->min_sample_distance, params->seed, samples, ranks);
	if (int rc = reg_host::stage(ctx, h, {{d + o_samples, samples.data(), idx_bytes}, {d + o_ranks, ranks.data(), idx_bytes}}))
		return rc;
	const float *src_pts = reinterpret_cast<const float *>(d + F.plan[0].D.o_pts), *tgt_pts = reinterpret_cast<const float *>(d + F.plan[1].D.o_pts);
	const int32_t *d_samples = reinterpret_cast<const int32_t *>(d + o_samples), *d_ranks = reinterpret_cast<const int32_t *>(d + o_ranks);
	int32_t *d_corr = reinterpret_cast<int32_t *>(d + o_corr);
	double *frames = reinterpret_cast<double *>(d + o_frames), *err = reinterpret_cast<double *>(d + o_err);
	FpfhSacOut *out = reinterpret_cast<FpfhSacOut *>(d + o_out);
	NdtDesc *ndesc = reinterpret_cast<NdtDesc *>(d + o_ndesc);
	NdtRec *nrec = reinterpret_cast<NdtRec *>(d + o_nrec);
	HIPCHK(ctx, launch_fpfh_similar(st, reinterpret_cast<const float *>(d + F.plan[0].D.o_hist), reinterpret_cast<const float *>(d + F.plan[1].D.o_hist), d_samples, d_ranks,
									n_samples, ns, nt, k_eff, d_corr));
	HIPCHK(ctx, launch_fpfh_models(st, src_pts, tgt_pts, d_samples, d_corr, iters, ns, nt, frames));
	NdtDesc base{};
	base.n_src_in = ns, base.n_tgt_in = nt;
	base.o_src = F.plan[0].D.o_pts, base.o_tgt = F.plan[1].D.o_pts, base.o_dist = o_dist;
	HIPCHK(ctx, launch_fpfh_slots(st, base, ns, nt, chunk, ndesc, nrec));
	const int huber = params->error_function == MULLS_SACIA_HUBER;
	for (uint32_t h0 = 0; h0 < iters; h0 += chunk)
	{
		const uint32_t hc = std::min(chunk, iters - h0);
		HIPCHK(ctx, launch_ndt_fitness(st, ndesc, hc, ns, d, nrec, frames + 12ull * h0));
		HIPCHK(ctx, launch_fpfh_errors(st, ndesc, hc, ns, d, params->max_correspondence_distance, huber, err + h0));
	}
	HIPCHK(ctx, launch_fpfh_pick(st, err, frames, iters, out));
	HIPCHK(ctx, launch_ndt_fitness(st, ndesc, 1, ns, d, nrec, out->frame)); // the winner's mean squared distance, in slot 0
	FpfhSacOut O;
	NdtRec R0;
	if (int rc = reg_host::download(ctx, h, {{out, &O, sizeof(O)}, {nrec, &R0, sizeof(R0)}}))
		return rc;
	*result = result_of(O, R0.fitness, iters, ns, nt);
	return MULLS_OK;
}
// ---- many clouds, many problems per call ----
constexpr size_t r256(size_t v) { return (v + 255u) & ~(size_t)255u; } // (up256 at compile time)
static_assert(sizeof(NdtDesc) + sizeof(NdtRec) <= fpfh_batch::SLOT_BYTES, "a slot of a stretch is counted with SLOT_BYTES");
static_assert(r256(sizeof(FpfhDesc)) + r256(sizeof(RegTab) * MULLS_REG_TABS) + r256(sizeof(RegHead)) <= fpfh_batch::CLOUD_TABLE_BYTES, "a cloud's table entries");
static_assert(r256(sizeof(FpfhProb)) + r256(sizeof(FpfhSacOut)) + r256(96) + r256(sizeof(NdtDesc)) + r256(sizeof(NdtRec)) <= fpfh_batch::PROBLEM_TABLE_BYTES,
			  "a problem's table entries");

// the distinct clouds among a sub-batch's: identity is (pts, n, stride)
struct Distinct
{
	std::vector<const mulls_cloud *> clouds;
	uint32_t id_of(const mulls_cloud *c)
	{
		for (uint32_t k = 0; k < clouds.size(); k++)
			if (clouds[k]->pts == c->pts && clouds[k]->n == c->n && clouds[k]->stride == c->stride)
				return k;
		clouds.push_back(c);
		return (uint32_t)clouds.size() - 1u;
	}
	size_t largest() const
	{
		size_t n = 0;
		for (const mulls_cloud *c : clouds)
			n = std::max<size_t>(n, c->n);
		return n;
	}
};

uint64_t limit_of(uint64_t scratch_limit_bytes) { return scratch_limit_bytes ? scratch_limit_bytes : MULLS_FPFHSAC_BATCH_DEFAULT_SCRATCH_BYTES; }

// One sub-batch of the descriptor batch: clouds[c0 .. c1).  copy_out false: only the heads are read.  *refused: the first entry whose cloud the device
// refused (ctx->err names it), else untouched.
int fpfh_sub_batch(mulls_ctx *ctx, const mulls_cloud *clouds, uint32_t c0, uint32_t c1, float r, float *const *hist, uint32_t *const *n_neighbours, bool copy_out,
				   const std::string &who)
{
	Distinct U;
	std::vector<uint32_t> id(c1 - c0);
	for (uint32_t c = c0; c < c1; c++)
		id[c - c0] = U.id_of(&clouds[c]);
	reg_host::Arena take;
	Features F;
	F.lay_out_all(U.clouds.data(), (uint32_t)U.clouds.size(), r, take);
	unsigned char *d, *h;
	if (int rc = reg_host::reserve(ctx, take.off, std::max<size_t>(F.staged(), 12ull * U.largest()), &d, &h))
		return rc;
	if (int rc = F.run(ctx, U.clouds.data(), r, d, h))
		return rc;
	std::vector<RegHead> heads(F.C);
	if (int rc = F.read_heads(ctx, d, h, heads.data()))
		return rc;
	for (uint32_t c = c0; c < c1; c++)
		if (heads[id[c - c0]].range)
		{
			const std::string name = "cloud " + std::to_string(c);
			const char *names[1] = {name.c_str()};
			return F.refusal(ctx, &heads[id[c - c0]], who, names, 1);
		}
	if (!copy_out)
		return MULLS_OK;
	for (uint32_t c = c0; c < c1; c++)
	{
		const FpfhDesc &D = F.plan[id[c - c0]].D;
		HIPCHK(ctx, hipMemcpyAsync(hist[c], d + D.o_hist, 4ull * MULLS_FPFH_DIMS * D.n, hipMemcpyDefault, ctx->stream));
		if (n_neighbours && n_neighbours[c])
			HIPCHK(ctx, hipMemcpyAsync(n_neighbours[c], d + D.o_k, 4ull * D.n, hipMemcpyDefault, ctx->stream));
	}
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	return MULLS_OK;
}

int fpfh_batch_run(mulls_ctx *ctx, const mulls_cloud *clouds, uint32_t n_clouds, const mulls_fpfh_params *params, float *const *hist, uint32_t *const *n_neighbours,
				   uint64_t scratch_limit_bytes)
{
	if (!ctx)
		return MULLS_E_INVALID;
	if (!n_clouds)
		return MULLS_OK;
	const std::string who = "mulls_compute_fpfh_batch: ";
	if (!clouds || !params || !hist)
	{
		ctx->err = who + "clouds, params or hist is NULL";
		return MULLS_E_INVALID;
	}
	if (!good_radius(params->search_radius))
	{
		ctx->err = who + "search_radius is not a positive number";
		return MULLS_E_INVALID;
	}
	for (uint32_t c = 0; c < n_clouds; c++)
	{
		std::string msg;
		const std::string name = "cloud " + std::to_string(c);
		if (int rc = check_cloud(&clouds[c], name.c_str(), 1, msg))
		{
			ctx->err = who + msg;
			return rc;
		}
		if (!hist[c])
		{
			ctx->err = who + name + ": hist is NULL";
			return MULLS_E_INVALID;
		}
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	mulls::StreamDrain drain{ctx->stream};
	const float r = 2.0f * params->search_radius;
	std::vector<uint64_t> bytes(n_clouds);
	for (uint32_t c = 0; c < n_clouds; c++)
		bytes[c] = fpfh_batch::cloud_bytes(clouds[c].n);
	std::vector<uint32_t> cuts;
	sub_batch_cuts(bytes.data(), n_clouds, limit_of(scratch_limit_bytes), fpfh_batch::MAX_CLOUDS, &cuts);
	const size_t subs = cuts.size() - 1;
	// One sub-batch: its heads are read, then its descriptors leave the arena.  Several: a first pass reads every sub-batch's heads and copies nothing; only
	// when all were good a second pass computes the sub-batches again and copies out, so that a refusal leaves every output untouched.
	if (subs > 1)
		for (size_t k = 0; k < subs; k++)
			if (int rc = fpfh_sub_batch(ctx, clouds, cuts[k], cuts[k + 1], r, hist, n_neighbours, false, who))
				return rc;
	for (size_t k = 0; k < subs; k++)
		if (int rc = fpfh_sub_batch(ctx, clouds, cuts[k], cuts[k + 1], r, hist, n_neighbours, true, who))
			return rc;
	return MULLS_OK;
}

// One sub-batch of SAC-IA: problems[b0 .. b1) -> res[b0 .. b1) (host memory of the call's own)
int fpfhsac_sub_batch(mulls_ctx *ctx, const mulls_fpfhsac_problem *problems, uint32_t b0, uint32_t b1, const mulls_fpfhsac_params &prm, uint64_t counted, uint64_t limit,
					  const std::string &who, mulls_fpfhsac_result *res)
{
	hipStream_t st = ctx->stream;
	const uint32_t P = b1 - b0, iters = (uint32_t)prm.max_iterations;
	const float r = 2.0f * prm.search_radius;
	Distinct U;
	std::vector<uint32_t> sid(P), tid(P), ns(P);
	for (uint32_t b = 0; b < P; b++)
		sid[b] = U.id_of(&problems[b0 + b].src), tid[b] = U.id_of(&problems[b0 + b].tgt), ns[b] = problems[b0 + b].src.n;
	const size_t n_hyp = (size_t)P * iters, n_samples = 3 * n_hyp;
	std::vector<fpfh_batch::Stretch> stretch;
	fpfh_batch::stretches(ns.data(), P, iters, fpfh_batch::pool_bytes(ns.data(), P, iters, counted, limit), &stretch);
	size_t pool = 0;
	for (const fpfh_batch::Stretch &S : stretch)
		pool = std::max<size_t>(pool, S.bytes);
	reg_host::Arena take;
	Features F;
	F.lay_out_all(U.clouds.data(), (uint32_t)U.clouds.size(), r, take);
	const size_t idx_bytes = 4 * n_samples;
	const size_t o_prob = take(sizeof(FpfhProb) * P), o_samples = take(idx_bytes), o_ranks = take(idx_bytes), o_corr = take(idx_bytes);
	const size_t o_frames = take(96 * n_hyp), o_err = take(8 * n_hyp), o_out = take(sizeof(FpfhSacOut) * P), o_wframes = take(96ull * P);
	const size_t o_wdesc = take(sizeof(NdtDesc) * P), o_wrec = take(sizeof(NdtRec) * P);
	const size_t o_ndesc = take(sizeof(NdtDesc) * fpfh_batch::MAX_SLOTS), o_nrec = take(sizeof(NdtRec) * fpfh_batch::MAX_SLOTS);
	std::vector<FpfhProb> prob(P);
	const std::vector<uint64_t> dist_first = fpfh_batch::dist_prefix(ns.data(), P, iters);
	uint32_t ns_max = 0;
	for (uint32_t b = 0; b < P; b++)
	{
		FpfhProb &B = prob[b];
		const FpfhDesc &S = F.plan[sid[b]].D, &T = F.plan[tid[b]].D;
		B.o_src = S.o_pts, B.o_tgt = T.o_pts, B.o_src_hist = S.o_hist, B.o_tgt_hist = T.o_hist;
		B.o_win_dist = take(4ull * ns[b]), B.dist_first = dist_first[b];
		B.n_src = S.n, B.n_tgt = T.n, B.k_eff = std::min<uint32_t>((uint32_t)prm.k_correspondences, T.n);
		B.first_sample = 3u * b * iters, B.first_hyp = b * iters, B.n_hyp = iters;
		ns_max = std::max(ns_max, ns[b]);
	}
	const size_t o_pool = take(pool);
	const size_t pin_need = std::max<size_t>({F.staged() + up256(sizeof(FpfhProb) * P), 12ull * U.largest(), reg_host::pinned_bytes({idx_bytes, idx_bytes}),
											  reg_host::pinned_bytes({sizeof(RegHead) * F.C}), reg_host::pinned_bytes({sizeof(FpfhSacOut) * P, sizeof(NdtRec) * P})});
	unsigned char *d, *h;
	if (int rc = reg_host::reserve(ctx, take.off, pin_need, &d, &h))
		return rc;
	if (int rc = F.run(ctx, U.clouds.data(), r, d, h, {d + o_prob, prob.data(), sizeof(FpfhProb) * P}))
		return rc;
	// The draws, per problem on the host pool, from the source's packed coordinates.  Host sources: drawn while the descriptors' launch set runs.  Device
	// sources: their coordinates come back with the heads, and their draws follow.
	std::vector<std::vector<float>> xyz(U.clouds.size());
	std::vector<char> is_source(U.clouds.size(), 0), on_dev(U.clouds.size(), 0);
	for (uint32_t b = 0; b < P; b++)
		is_source[sid[b]] = 1;
	for (size_t c = 0; c < U.clouds.size(); c++)
	{
		if (!is_source[c])
			continue;
		const mulls_cloud &cl = *U.clouds[c];
		xyz[c].resize(3 * (size_t)cl.n);
		on_dev[c] = reg_host::on_device(ctx, cl) ? 1 : 0;
		if (on_dev[c])
			HIPCHK(ctx, hipMemcpyAsync(xyz[c].data(), d + F.plan[c].D.o_pts, 12ull * cl.n, hipMemcpyDeviceToHost, st));
		else
			for (uint32_t i = 0; i < cl.n; i++)
				std::memcpy(&xyz[c][3 * (size_t)i], static_cast<const unsigned char *>(cl.pts) + (size_t)i * cl.stride, 12);
	}
	std::vector<int32_t> samples(n_samples), ranks(n_samples);
	auto draw_where = [&](char device_sources) {
		std::vector<uint32_t> todo;
		for (uint32_t b = 0; b < P; b++)
			if (on_dev[sid[b]] == device_sources)
				todo.push_back(b);
		shared_host_pool().parallel_for(0, (long)todo.size(), 1, [&](long k) {
			const uint32_t b = todo[(size_t)k];
			std::vector<int32_t> s, q;
			(void)fpfh::draw_all(xyz[sid[b]].data(), ns[b], prob[b].k_eff, 3, (int)iters, prm.min_sample_distance, prm.seed, s, q);
			std::memcpy(&samples[(size_t)prob[b].first_sample], s.data(), 12ull * iters), std::memcpy(&ranks[(size_t)prob[b].first_sample], q.data(), 12ull * iters);
		});
	};
	draw_where(0);
	// the clouds' refusals, before anything else is launched
	std::vector<RegHead> heads(F.C);
	if (int rc = F.read_heads(ctx, d, h, heads.data()))
		return rc;
	for (uint32_t b = 0; b < P; b++)
		for (int which = 0; which < 2; which++)
		{
			const uint32_t c = which ? tid[b] : sid[b];
			if (!heads[c].range)
				continue;
			const char *names[1] = {which ? "the target" : "the source"};
			return F.refusal(ctx, &heads[c], reg_host::refusal_prefix(who, false, b0 + b), names, 1);
		}
	draw_where(1);
	if (int rc = reg_host::stage(ctx, h, {{d + o_samples, samples.data(), idx_bytes}, {d + o_ranks, ranks.data(), idx_bytes}}))
		return rc;
	const FpfhProb *d_prob = reinterpret_cast<const FpfhProb *>(d + o_prob);
	const int32_t *d_samples = reinterpret_cast<const int32_t *>(d + o_samples), *d_ranks = reinterpret_cast<const int32_t *>(d + o_ranks);
	int32_t *d_corr = reinterpret_cast<int32_t *>(d + o_corr);
	double *frames = reinterpret_cast<double *>(d + o_frames), *err = reinterpret_cast<double *>(d + o_err), *wframes = reinterpret_cast<double *>(d + o_wframes);
	FpfhSacOut *out = reinterpret_cast<FpfhSacOut *>(d + o_out);
	NdtDesc *ndesc = reinterpret_cast<NdtDesc *>(d + o_ndesc), *wdesc = reinterpret_cast<NdtDesc *>(d + o_wdesc);
	NdtRec *nrec = reinterpret_cast<NdtRec *>(d + o_nrec), *wrec = reinterpret_cast<NdtRec *>(d + o_wrec);
	HIPCHK(ctx, launch_fpfh_batch_similar(st, d_prob, P, d, d_samples, d_ranks, (uint32_t)n_samples, d_corr));
	HIPCHK(ctx, launch_fpfh_batch_models(st, d_prob, P, d, d_samples, d_corr, (uint32_t)n_hyp, frames));
	const int huber = prm.error_function == MULLS_SACIA_HUBER;
	for (const fpfh_batch::Stretch &S : stretch)
	{
		HIPCHK(ctx, launch_fpfh_batch_slots(st, d_prob, P, S.h0, S.n, o_pool, S.d0, ndesc, nrec));
		HIPCHK(ctx, launch_ndt_fitness(st, ndesc, S.n, S.n_src_max, d, nrec, frames + 12ull * S.h0));
		HIPCHK(ctx, launch_fpfh_batch_errors(st, ndesc, S.n, d, prm.max_correspondence_distance, huber, err + S.h0));
	}
	HIPCHK(ctx, launch_fpfh_batch_pick(st, d_prob, P, err, frames, out, wframes, wdesc, wrec));
	HIPCHK(ctx, launch_ndt_fitness(st, wdesc, P, ns_max, d, wrec, wframes)); // the winners' mean squared distances
	std::vector<FpfhSacOut> O(P);
	std::vector<NdtRec> R(P);
	if (int rc = reg_host::download(ctx, h, {{out, O.data(), sizeof(FpfhSacOut) * P}, {wrec, R.data(), sizeof(NdtRec) * P}}))
		return rc;
	for (uint32_t b = 0; b < P; b++)
		res[b0 + b] = result_of(O[b], R[b].fitness, iters, prob[b].n_src, prob[b].n_tgt);
	return MULLS_OK;
}

int fpfhsac_batch_run(mulls_ctx *ctx, const mulls_fpfhsac_problem *problems, uint32_t n_problems, const mulls_fpfhsac_params *params, uint64_t scratch_limit_bytes,
					  mulls_fpfhsac_result *results)
{
	if (!ctx)
		return MULLS_E_INVALID;
	if (!n_problems)
		return MULLS_OK;
	const std::string who = "mulls_coarse_reg_fpfhsac_batch: ";
	if (!problems || !params || !results)
	{
		ctx->err = who + "problems, params or results is NULL";
		return MULLS_E_INVALID;
	}
	const char *bad = nullptr;
	if (int rc = check_params(*params, &bad))
	{
		ctx->err = reg_host::refusal_prefix(who, false, 0) + bad; // (a refused parameter refuses problem 0)
		return rc;
	}
	for (uint32_t b = 0; b < n_problems; b++)
	{
		std::string msg;
		int rc = check_cloud(&problems[b].src, "the source", 3, msg);
		if (!rc)
			rc = check_cloud(&problems[b].tgt, "the target", 1, msg);
		if (rc)
		{
			ctx->err = reg_host::refusal_prefix(who, false, b) + msg;
			return rc;
		}
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	mulls::StreamDrain drain{ctx->stream};
	const uint64_t limit = limit_of(scratch_limit_bytes);
	std::vector<uint64_t> bytes(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
		bytes[b] = fpfh_batch::problem_bytes(problems[b].src.n, problems[b].tgt.n, (uint64_t)params->max_iterations);
	std::vector<uint32_t> cuts;
	sub_batch_cuts(bytes.data(), n_problems, limit, fpfh_batch::MAX_SLOTS, &cuts, fpfh_batch::HEAD_BYTES);
	std::vector<mulls_fpfhsac_result> res(n_problems); // copied out only after the last sub-batch succeeded
	for (size_t k = 0; k + 1 < cuts.size(); k++)
	{
		uint64_t counted = fpfh_batch::HEAD_BYTES;
		for (uint32_t b = cuts[k]; b < cuts[k + 1]; b++)
			counted += bytes[b];
		if (int rc = fpfhsac_sub_batch(ctx, problems, cuts[k], cuts[k + 1], *params, counted, limit, who, res.data()))
			return rc;
	}
	std::memcpy(results, res.data(), sizeof(mulls_fpfhsac_result) * n_problems);
	return MULLS_OK;
}
} // namespace

extern "C"
{
	void mulls_fpfh_default_params(mulls_fpfh_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->search_radius = 1.0f;
	}

	int mulls_fpfh(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_fpfh_params *params, float *hist, uint32_t *n_neighbours)
	try
	{
		return fpfh_run(ctx, cloud, params, hist, n_neighbours);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	void mulls_fpfhsac_default_params(mulls_fpfhsac_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->search_radius = 1.0f;
		p->nr_samples = 3, p->k_correspondences = 15, p->max_iterations = 10;
		p->min_sample_distance = 0.f, p->max_correspondence_distance = HUGE_VALF;
		p->error_function = MULLS_SACIA_TRUNCATED;
		p->seed = 0;
	}

	int mulls_coarse_reg_fpfhsac(mulls_ctx *ctx, const mulls_cloud *tgt, const mulls_cloud *src, const mulls_fpfhsac_params *params, mulls_fpfhsac_result *result)
	try
	{
		return fpfhsac_run(ctx, tgt, src, params, result);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	int mulls_compute_fpfh_batch(mulls_ctx *ctx, const mulls_cloud *clouds, uint32_t n_clouds, const mulls_fpfh_params *params, float *const *hist,
								 uint32_t *const *n_neighbours, uint64_t scratch_limit_bytes)
	try
	{
		return fpfh_batch_run(ctx, clouds, n_clouds, params, hist, n_neighbours, scratch_limit_bytes);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	int mulls_coarse_reg_fpfhsac_batch(mulls_ctx *ctx, const mulls_fpfhsac_problem *problems, uint32_t n_problems, const mulls_fpfhsac_params *params,
									   uint64_t scratch_limit_bytes, mulls_fpfhsac_result *results)
	try
	{
		return fpfhsac_batch_run(ctx, problems, n_problems, params, scratch_limit_bytes, results);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}
}
