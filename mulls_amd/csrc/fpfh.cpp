// fpfh.cpp — mulls_fpfh (CRegistration::compute_fpfh_feature, cregistration.hpp:351-369) and mulls_coarse_reg_fpfhsac (coarse_reg_fpfhsac, :372-406).
// Host side: the argument checks before any device work, the arena, the uploads, the launch sets of k_fpfh.hip and the results.  The cell tables are
// the registrations' (reg_launch.h), the sub-batch arena, staging and downloads reg_host.h's, the nearest-target pass mulls_ndt's (ndt_launch.h), the
// draws fpfh_math.h's.  include/mulls_hip.h has the definition this file follows.
#include <cmath>
#include <cstring>

#include "ctx.h"
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

// the descriptors of C clouds in one launch set
struct Features
{
	uint32_t C = 0;
	CloudPlan plan[2];
	size_t o_desc = 0, o_tabs = 0, o_head = 0;
	uint32_t n_max = 0, slots_max = 0;
	void lay_out_all(const mulls_cloud *const *clouds, uint32_t count, float r, reg_host::Arena &take)
	{
		C = count;
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
	int run(mulls_ctx *ctx, const mulls_cloud *const *clouds, float r, unsigned char *d, unsigned char *h)
	{
		for (uint32_t c = 0; c < C; c++)
		{
			if (int rc = reg_host::upload_xyz(ctx, *clouds[c], 0, d + plan[c].D.o_pts, h))
				return rc;
			if (int rc = reg_host::upload_xyz(ctx, *clouds[c], 16, d + plan[c].D.o_nrm, h))
				return rc;
		}
		FpfhDesc descs[2];
		RegTab tabs[2 * MULLS_REG_TABS];
		RegHead heads[2];
		for (uint32_t c = 0; c < C; c++)
		{
			descs[c] = plan[c].D, heads[c] = plan[c].H;
			for (int tb = 0; tb < MULLS_REG_TABS; tb++)
				tabs[MULLS_REG_TABS * c + tb] = plan[c].tab[tb];
		}
		if (int rc = reg_host::stage(ctx, h, {{d + o_desc, descs, sizeof(FpfhDesc) * C}, {d + o_tabs, tabs, sizeof(RegTab) * MULLS_REG_TABS * C}, {d + o_head, heads, sizeof(RegHead) * C}}))
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
	int refusal(mulls_ctx *ctx, const RegHead *heads, const std::string &who, const char *const *names) const
	{
		for (uint32_t c = 0; c < C; c++)
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
	if (int rc = F.refusal(ctx, &head, who, names))
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
	if (int rc = F.refusal(ctx, heads, who, names))
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
	mulls_fpfhsac_result res;
	std::memset(&res, 0, sizeof(res));
	res.best_iteration = O.best, res.iterations = (int32_t)iters, res.n_src = ns, res.n_tgt = nt;
	res.best_error = O.error, res.fitness = R0.fitness;
	for (int rr = 0; rr < 3; rr++)
	{
		for (int c = 0; c < 3; c++)
			res.T[rr + 4 * c] = O.frame[3 * rr + c];
		res.T[12 + rr] = O.frame[9 + rr];
	}
	res.T[15] = 1.0;
	*result = res;
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
}
