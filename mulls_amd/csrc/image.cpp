// image.cpp — mulls_cloud_centre, mulls_map_image_2d, mulls_range_image and mulls_scan_images_batch: CloudUtility::get_cloud_cpt, CFilter::generate_2d_map
// and CFilter::pointcloud_to_rangeimage (test/mulls_slam.cpp:722-733, :1016-1025) on the device (k_image.hip).  Host side: argument checks for the whole call
// before anything runs, the scans of a call cut into sub-batches by a byte budget (host scans staged, device scans read where they are), per sub-batch one
// upload of the tables, one zeroing, one launch per pass, one download of the stats and the 8-bit images.  The single calls are a batch of one scan.
// include/mulls_hip.h has the definition this file follows.
#include <chrono>
#include <cmath>

#include "ctx.h"
#include "image_launch.h"
#include "subbatch.h"

// a context's scratch of these entry points: one device arena, one pinned host buffer (tables up, stats and images down); grow-only
struct mulls_image_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr;
	size_t dev_cap = 0, pin_cap = 0;
};

namespace
{
using namespace mulls::image;
constexpr size_t REC = MULLS_POINT_BYTES;
constexpr uint64_t ARENA_BUDGET_BYTES = 1ull << 30; // a sub-batch's images, partial sums and staged host scans (a scan beyond it runs alone)
constexpr uint32_t MAX_SCANS_PER_SUBBATCH = 4096u;
constexpr uint64_t MAX_CHUNKS_PER_SUBBATCH = 1u << 22;
constexpr int DEFAULT_COUNT_FORM = 2; // count_form 0: the faster form on the merged map and on the per-frame views (profiles/images.txt)

bool cloud_on_device(mulls_ctx *ctx, const mulls_cloud &c)
{
	if (mulls_is_map_memory(ctx, c.pts, (size_t)c.n * REC))
		return true;
	hipPointerAttribute_t at;
	std::memset(&at, 0, sizeof(at));
	if (hipPointerGetAttributes(&at, c.pts) == hipSuccess)
		return at.type == hipMemoryTypeDevice;
	(void)hipGetLastError(); // (an ordinary host pointer: the query reports an error on some runtimes — cleared)
	return false;
}

uint32_t chunks_of(uint32_t n) { return n / MULLS_SCAN_CHUNK + (n % MULLS_SCAN_CHUNK ? 1u : 0u); }

// what a call asks for.  rp / bp NULL: no such image; centres: NULL or 3 doubles per scan; counts: NULL, or the one scan's counts
struct Want
{
	const mulls_range_image_params *rp;
	const mulls_image2d_params *bp;
	uint8_t *const *range_out, *const *bev_out;
	int32_t *counts;
	mulls_image2d_report *reports;
	double *centres;
};

int images_run(mulls_ctx *ctx, const char *who, const mulls_cloud *scans, uint32_t S, const Want &w)
{
	const auto t0 = std::chrono::steady_clock::now();
	// every refusal of the call, before anything is written
	auto refuse = [&](int rc, const std::string &why) {
		ctx->err = std::string(who) + ": " + why;
		return rc;
	};
	if (S && !scans)
		return refuse(MULLS_E_INVALID, "scans is NULL");
	if (w.rp)
		if (const char *why = refusal(*w.rp))
			return refuse(MULLS_E_INVALID, why);
	if (w.bp)
		if (const char *why = refusal(*w.bp))
			return refuse(MULLS_E_INVALID, why);
	if (S && ((w.rp && !w.range_out) || (w.bp && !w.bev_out)))
		return refuse(MULLS_E_INVALID, "an image is NULL");
	for (uint32_t s = 0; s < S; s++)
	{
		if ((scans[s].n && !scans[s].pts) || scans[s].stride != MULLS_POINT_BYTES)
			return refuse(MULLS_E_INVALID, "a cloud (stride 48)");
		if ((w.rp && !w.range_out[s]) || (w.bp && !w.bev_out[s]))
			return refuse(MULLS_E_INVALID, "an image is NULL");
	}
	for (uint32_t s = 0; s < S; s++)
		if (scans[s].n > MULLS_SCAN_MAX_POINTS)
			return refuse(MULLS_E_UNSUPPORTED, "more than 2^24 = 16777216 points");
	if (S == 0)
		return MULLS_OK;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const bool want_centre = w.bp || w.centres;
	const uint32_t mp = w.bp ? (uint32_t)w.bp->map_width * (uint32_t)w.bp->map_height : 0u;
	const uint32_t rpix = w.rp ? (uint32_t)w.rp->width * (uint32_t)w.rp->height : 0u;
	Map2d M{};
	Range R{};
	if (w.bp)
		M = derive(*w.bp);
	if (w.rp)
		R = derive(*w.rp);
	const int form = M.form ? M.form : DEFAULT_COUNT_FORM;

	std::vector<uint8_t> dev(S);
	std::vector<uint64_t> bytes(S), wgs(S);
	for (uint32_t s = 0; s < S; s++)
	{
		dev[s] = scans[s].n && cloud_on_device(ctx, scans[s]);
		bytes[s] = 5ull * ((uint64_t)mp + rpix) + (want_centre ? 24ull * MULLS_NDT_TREE : 0ull) + (dev[s] ? 0ull : up256((uint64_t)scans[s].n * REC)) + 128u;
		wgs[s] = chunks_of(scans[s].n);
	}
	std::vector<uint32_t> cuts;
	sub_batch_cuts(bytes.data(), S, ARENA_BUDGET_BYTES, MAX_SCANS_PER_SUBBATCH, &cuts, 16u * 256u, wgs.data(), MAX_CHUNKS_PER_SUBBATCH);

	if (!ctx->image)
		ctx->image = new mulls_image_scratch();
	mulls_image_scratch &sc = *ctx->image;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	std::vector<ImageStat> stats(S);
	for (size_t k = 0; k + 1 < cuts.size(); k++)
	{
		const uint32_t s0 = cuts[k], Ss = cuts[k + 1] - s0;
		size_t off = 0;
		auto take = [&](size_t n_bytes) {
			const size_t o = off;
			off += up256(n_bytes);
			return o;
		};
		const size_t o_scans = take(Ss * sizeof(ImageScan)), o_chunk0 = take((Ss + 1u) * 4u), table_bytes = off;
		const size_t o_partial = take(want_centre ? (size_t)Ss * 24u * MULLS_NDT_TREE : 0u);
		const size_t o_counters = take((size_t)Ss * 16u), o_counts = take((size_t)Ss * mp * 4u), o_words = take((size_t)Ss * rpix * 4u), zero_end = off;
		const size_t o_stats = take(Ss * sizeof(ImageStat)), o_bev = take((size_t)Ss * mp), o_range = take((size_t)Ss * rpix), down_end = off;
		size_t staged = 0;
		for (uint32_t j = 0; j < Ss; j++)
			staged += dev[s0 + j] ? 0u : up256((size_t)scans[s0 + j].n * REC);
		const size_t o_stage = take(staged);
		if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
			return rc;
		const size_t down_bytes = down_end - o_stats;
		if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, table_bytes + down_bytes, hipHostMallocDefault))
			return rc;
		unsigned char *d = sc.dev, *h = sc.pin;
		ImageScan *hs = reinterpret_cast<ImageScan *>(h + o_scans);
		uint32_t *hc = reinterpret_cast<uint32_t *>(h + o_chunk0);
		size_t so = o_stage;
		uint32_t g = 0;
		for (uint32_t j = 0; j < Ss; j++)
		{
			const mulls_cloud &c = scans[s0 + j];
			hs[j].n = c.n, hs[j].chunk0 = hc[j] = g;
			g += chunks_of(c.n);
			if (dev[s0 + j] || c.n == 0)
				hs[j].in = static_cast<const float4 *>(c.pts);
			else
			{
				hs[j].in = reinterpret_cast<const float4 *>(d + so);
				HIPCHK(ctx, hipMemcpyAsync(d + so, c.pts, (size_t)c.n * REC, hipMemcpyHostToDevice, st));
				so += up256((size_t)c.n * REC);
			}
		}
		hc[Ss] = g;
		ImageBatch B;
		B.scans = reinterpret_cast<const ImageScan *>(d + o_scans), B.chunk0 = reinterpret_cast<const uint32_t *>(d + o_chunk0);
		B.partial = reinterpret_cast<double *>(d + o_partial), B.counters = reinterpret_cast<uint32_t *>(d + o_counters);
		B.counts = reinterpret_cast<int32_t *>(d + o_counts), B.words = reinterpret_cast<uint32_t *>(d + o_words);
		B.stats = reinterpret_cast<ImageStat *>(d + o_stats), B.bev = d + o_bev, B.range = d + o_range;
		B.S = Ss, B.G = g, B.map_pixels = mp, B.range_pixels = rpix;
		HIPCHK(ctx, hipMemcpyAsync(d, h, table_bytes, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, hipMemsetAsync(d + o_counters, 0, zero_end - o_counters, st)); // the one zeroing: counters, counts and words of every scan
		if (want_centre)
			HIPCHK(ctx, launch_image_centre(st, B));
		if (w.bp)
			HIPCHK(ctx, launch_image_count(st, B, M, form));
		if (w.rp)
			HIPCHK(ctx, launch_image_range(st, B, R));
		HIPCHK(ctx, launch_image_convert(st, B, M));
		unsigned char *down = h + table_bytes; // the stats and the 8-bit images as they lie on the device from o_stats on
		HIPCHK(ctx, hipMemcpyAsync(down, d + o_stats, down_bytes, hipMemcpyDeviceToHost, st));
		if (w.counts) // (the single call's second product: straight to the caller)
			HIPCHK(ctx, hipMemcpyAsync(w.counts, B.counts, (size_t)mp * 4u, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		std::memcpy(&stats[s0], down, Ss * sizeof(ImageStat));
		for (uint32_t j = 0; j < Ss; j++)
		{
			if (w.bp)
				std::memcpy(w.bev_out[s0 + j], down + (o_bev - o_stats) + (size_t)j * mp, mp);
			if (w.rp)
				std::memcpy(w.range_out[s0 + j], down + (o_range - o_stats) + (size_t)j * rpix, rpix);
		}
	}
	const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	for (uint32_t s = 0; s < S; s++)
	{
		if (w.centres)
			std::memcpy(w.centres + 3 * (size_t)s, stats[s].centre, 24);
		if (w.bp && w.reports)
		{
			mulls_image2d_report &r = w.reports[s];
			std::memcpy(r.centre, stats[s].centre, 24);
			r.n_counted = stats[s].counted, r.n_skipped_height = stats[s].skipped_height, r.n_skipped_frame = stats[s].skipped_frame;
			r.ms_total = ms;
		}
	}
	return MULLS_OK;
}
} // namespace

void mulls_image_release(mulls_ctx *ctx)
{
	if (!ctx->image)
		return;
	staggered_free(ctx->image->dev);
	if (ctx->image->pin)
		(void)hipHostFree(ctx->image->pin);
	delete ctx->image;
	ctx->image = nullptr;
}

extern "C"
{
	void mulls_image2d_default_params(mulls_image2d_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->m2pix = 1.0; // test/mulls_slam.cpp:1018: generate_2d_map(pc_map_merged, 1, 1920, 1080, 20, 1000, -FLT_MAX, FLT_MAX, true)
		p->map_width = 1920, p->map_height = 1080;
		p->min_points_in_pix = 20, p->max_points_in_pix = 1000;
		p->min_height = -3.4028234663852886e38, p->max_height = 3.4028234663852886e38;
		p->shift = 1;
	}

	void mulls_range_image_default_params(mulls_range_image_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->width = 900, p->height = 64; // cfilter.hpp:2717-2721
		p->f_up_deg = 3.0f, p->f_down_deg = 25.0f, p->max_distance = 70.0f;
	}

	int mulls_cloud_centre(mulls_ctx *ctx, const mulls_cloud *cloud, double c[3])
	try
	{
		if (!ctx || !cloud || !c)
			return MULLS_E_INVALID;
		Want w{};
		double centre[3] = {0.0, 0.0, 0.0};
		w.centres = centre;
		if (int rc = images_run(ctx, "mulls_cloud_centre", cloud, 1, w))
			return rc;
		std::memcpy(c, centre, sizeof(centre));
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_map_image_2d(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_image2d_params *p, uint8_t *image, int32_t *counts, mulls_image2d_report *report)
	try
	{
		if (!ctx || !cloud || !p)
			return MULLS_E_INVALID;
		Want w{};
		w.bp = p, w.bev_out = &image, w.counts = counts, w.reports = report;
		return images_run(ctx, "mulls_map_image_2d", cloud, 1, w);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_range_image(mulls_ctx *ctx, const mulls_cloud *scan, const mulls_range_image_params *p, uint8_t *image)
	try
	{
		if (!ctx || !scan || !p)
			return MULLS_E_INVALID;
		Want w{};
		w.rp = p, w.range_out = &image;
		return images_run(ctx, "mulls_range_image", scan, 1, w);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_scan_images_batch(mulls_ctx *ctx, const mulls_cloud *scans, uint32_t n_scans, const mulls_range_image_params *rp, const mulls_image2d_params *bp,
								uint8_t *const *range_out, uint8_t *const *bev_out, mulls_image2d_report *reports)
	try
	{
		if (!ctx)
			return MULLS_E_INVALID;
		Want w{};
		w.rp = rp, w.bp = bp, w.range_out = range_out, w.bev_out = bev_out, w.reports = reports;
		return images_run(ctx, "mulls_scan_images_batch", scans, n_scans, w);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}
}
