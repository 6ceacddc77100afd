// sor.cpp — mulls_sor_filter: CFilter<PointT>::sor_filter (cfilter.hpp:204-247, pcl::StatisticalOutlierRemoval), the filter of the merged map
// mulls_slam exports (mulls_slam.cpp:1009), on the device (k_sor.hip).  Host side: argument checks, staging, the choice of the cell edge from a handful
// of probe queries, the sequence of grid levels and the brute-force pass over what they leave, one result download.  include/mulls_hip.h has the
// definition this file follows.
#include <chrono>
#include <cmath>

#include "ctx.h"
#include "sor_launch.h"
#include "subbatch.h"

// a context's scratch of this entry point: one device arena, one device buffer for a device cloud's kept records, one pinned host buffer; grow-only
struct mulls_sor_scratch
{
	unsigned char *dev = nullptr, *out = nullptr, *pin = nullptr;
	size_t dev_cap = 0, out_cap = 0, pin_cap = 0;
};

void mulls_sor_release(mulls_ctx *ctx)
{
	if (!ctx->sor)
		return;
	staggered_free(ctx->sor->dev);
	staggered_free(ctx->sor->out);
	if (ctx->sor->pin)
		(void)hipHostFree(ctx->sor->pin);
	delete ctx->sor;
	ctx->sor = nullptr;
}

namespace
{
constexpr uint32_t BRUTE_QUERIES_PER_LAUNCH = 65536u; // bounds one brute-force launch's work whatever the cloud looks like
constexpr size_t HDR_BYTES = 256;

bool cloud_on_device(mulls_ctx *ctx, const mulls_cloud &c)
{
	if (mulls_is_map_memory(ctx, c.pts, (size_t)c.n * MULLS_POINT_BYTES))
		return true;
	hipPointerAttribute_t at;
	std::memset(&at, 0, sizeof(at));
	if (hipPointerGetAttributes(&at, c.pts) == hipSuccess)
		return at.type == hipMemoryTypeDevice;
	(void)hipGetLastError(); // (an ordinary host pointer: the query reports an error on some runtimes — cleared)
	return false;
}

float dec_ordered(uint32_t u)
{
	const uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
	float f;
	std::memcpy(&f, &b, 4);
	return f;
}

int sor_run(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_sor_params *params, void *out, uint32_t cap, uint32_t *n_out, int32_t *kept_idx, uint32_t idx_cap,
			float *mean_dist, mulls_sor_report *report)
{
	const auto t0 = std::chrono::steady_clock::now();
	if (!ctx || !cloud || !params || !n_out || (cap && !out) || (idx_cap && !kept_idx))
		return MULLS_E_INVALID;
	*n_out = 0;
	if (report)
		std::memset(report, 0, sizeof(*report));
	const mulls_cloud Cl = *cloud;
	const uint32_t n = Cl.n;
	if (n && !Cl.pts)
		return MULLS_E_INVALID;
	if (params->mean_k < 1)
	{
		ctx->err = "mulls_sor_filter: mean_k < 1";
		return MULLS_E_INVALID;
	}
	if (params->mean_k > MULLS_SOR_MAX_K)
	{
		ctx->err = "mulls_sor_filter: mean_k above 64";
		return MULLS_E_UNSUPPORTED;
	}
	if (!std::isfinite(params->std_mul))
	{
		ctx->err = "mulls_sor_filter: std_mul is not finite";
		return MULLS_E_INVALID;
	}
	if (n == 0)
		return MULLS_OK;
	if (n <= (uint32_t)params->mean_k)
	{
		ctx->err = "mulls_sor_filter: the cloud has no more than mean_k points (upstream reads past the neighbour search's result there)";
		return MULLS_E_INVALID;
	}
	if (n > MULLS_SOR_MAX_POINTS)
	{
		ctx->err = "mulls_sor_filter: more than 2^24 = 16777216 points";
		return MULLS_E_UNSUPPORTED;
	}
	const int kk = params->mean_k + 1;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const bool on_dev = cloud_on_device(ctx, Cl);
	if (on_dev ? Cl.stride != MULLS_POINT_BYTES : (Cl.stride < MULLS_POINT_BYTES || Cl.stride % 4u))
	{
		ctx->err = "mulls_sor_filter: stride (device clouds: 48; host clouds: a multiple of 4, at least 48)";
		return MULLS_E_INVALID;
	}
	if (!ctx->sor)
		ctx->sor = new mulls_sor_scratch();
	mulls_sor_scratch &sc = *ctx->sor;

	const uint32_t slots = 2u * n + 1u; // load factor below one half
	const uint32_t n_probe = std::min(n, MULLS_SOR_PROBES);
	size_t off = 0;
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return at;
	};
	const size_t o_pts = take((size_t)n * 16u), o_sorted = take((size_t)n * 16u), o_slot = take((size_t)n * 4u), o_flags = take((size_t)n * 4u);
	const size_t o_pos = take(((size_t)n + 1u) * 4u), o_left0 = take((size_t)n * 4u), o_left1 = take((size_t)n * 4u);
	const size_t o_keys = take((size_t)slots * 8u), o_counts = take((size_t)slots * 4u), o_start = take(((size_t)slots + 1u) * 4u);
	const size_t o_tmp = take(((size_t)slots / 4096u + 3u) * 4u), o_part = take((size_t)MULLS_SOR_PARTIALS * 16u);
	const size_t o_probe = take(MULLS_SOR_PROBES * 4u);
	// what comes down, contiguous: header and the probes' radii; header, kept indices and distances
	const size_t o_hdr = take(HDR_BYTES - 1), o_kth = take(MULLS_SOR_PROBES * 4u);
	const size_t o_res = take(HDR_BYTES - 1), o_kept = take((size_t)n * 4u), o_dist = take((size_t)n * 4u);
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
		return rc;
	const size_t pin_need = std::max((size_t)n * 16u, up256(HDR_BYTES) + up256((size_t)n * 4u) * 2u) + 4096u;
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, pin_need, hipHostMallocDefault))
		return rc;
	static_assert(sizeof(SorHeader) <= HDR_BYTES, "SorHeader");
	unsigned char *d = sc.dev, *h = sc.pin;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	float4 *pts = reinterpret_cast<float4 *>(d + o_pts), *sorted = reinterpret_cast<float4 *>(d + o_sorted);
	uint32_t *left[2] = {reinterpret_cast<uint32_t *>(d + o_left0), reinterpret_cast<uint32_t *>(d + o_left1)};
	uint32_t *counts = reinterpret_cast<uint32_t *>(d + o_counts), *scan_tmp = reinterpret_cast<uint32_t *>(d + o_tmp);
	SorHeader *hdr = reinterpret_cast<SorHeader *>(d + o_hdr);
	float *dist = reinterpret_cast<float *>(d + o_dist);
	int32_t *d_kept = reinterpret_cast<int32_t *>(d + o_kept);
	SorHeader H;

	// staging: x, y, z and the index
	if (on_dev)
		HIPCHK(ctx, launch_sor_gather(st, Cl.pts, n, pts));
	else
	{
		const unsigned char *p = static_cast<const unsigned char *>(Cl.pts);
		const long chunk = 32768;
		shared_host_pool().parallel_for(0, ((long)n + chunk - 1) / chunk, 1, [&](long c) {
			const uint32_t e = (uint32_t)std::min<long>((c + 1) * chunk, n);
			for (uint32_t i = (uint32_t)(c * chunk); i < e; i++)
			{
				std::memcpy(h + (size_t)i * 16u, p + (size_t)i * Cl.stride, 12);
				std::memcpy(h + (size_t)i * 16u + 12u, &i, 4);
			}
		});
		HIPCHK(ctx, hipMemcpyAsync(pts, h, (size_t)n * 16u, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, hipStreamSynchronize(st)); // (the pinned buffer is reused below)
	}
	HIPCHK(ctx, launch_sor_bounds(st, pts, n, hdr));

	// probes: the kk-th neighbour distance of a few evenly spaced points, by brute force (over a thinned cloud above 2^20 points, with the rank thinned
	// alike); their median is the cell edge.  Whatever edge comes out, the result is the same: the edge decides only how much work the rings are.
	const uint32_t step = (n + (1u << 20) - 1u) >> 20;
	const int kk_probe = std::max(2, std::min(kk, (kk + (int)step - 1) / (int)step));
	{
		uint32_t *hp = reinterpret_cast<uint32_t *>(h);
		for (uint32_t s = 0; s < n_probe; s++)
			hp[s] = (uint32_t)(((uint64_t)s * n) / n_probe);
		HIPCHK(ctx, hipMemcpyAsync(d + o_probe, h, (size_t)n_probe * 4u, hipMemcpyHostToDevice, st));
	}
	HIPCHK(ctx, launch_sor_brute(st, pts, n, step, reinterpret_cast<const uint32_t *>(d + o_probe), n_probe, kk_probe, nullptr, reinterpret_cast<float *>(d + o_kth)));
	HIPCHK(ctx, hipMemcpyAsync(h + 1024, d + o_hdr, up256(HDR_BYTES) + (size_t)n_probe * 4u, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::memcpy(&H, h + 1024, sizeof(H));
	if (H.bad)
	{
		ctx->err = "mulls_sor_filter: a coordinate is not finite";
		return MULLS_E_INVALID;
	}
	double lo[3], extent = 0.0;
	for (int a = 0; a < 3; a++)
	{
		lo[a] = (double)dec_ordered(H.lo_enc[a]);
		extent = std::max(extent, (double)dec_ordered(H.hi_enc[a]) - lo[a]);
	}
	double edge = 0.0;
	{
		const float *kth = reinterpret_cast<const float *>(h + 1024 + up256(HDR_BYTES));
		std::vector<float> r;
		for (uint32_t s = 0; s < n_probe; s++)
			if (std::isfinite(kth[s]))
				r.push_back(kth[s]);
		if (!r.empty())
		{
			std::nth_element(r.begin(), r.begin() + r.size() / 2, r.end());
			edge = std::sqrt((double)r[r.size() / 2]);
		}
	}
	// the packed key holds 2^21 cells along an axis: the edge is raised until the extent takes at most 2^20 of them (k_sor_cells still checks)
	edge = std::max(std::max(edge, extent / 1048576.0), 1e-6);
	if (!std::isfinite(edge))
	{
		ctx->err = "mulls_sor_filter: the cloud's extent is not representable";
		return MULLS_E_UNSUPPORTED;
	}

	// grid levels: every query on the first, what a level leaves uncertified on the next
	uint32_t nq = n, n_fallback = 0;
	const uint32_t *qlist = nullptr;
	for (int level = 0; level < MULLS_SOR_LEVELS && nq; level++, edge *= 4.0)
	{
		SorGrid G;
		for (int a = 0; a < 3; a++)
			G.lo[a] = lo[a];
		G.edge = edge, G.inv_edge = 1.0 / edge;
		G.keys = reinterpret_cast<uint64_t *>(d + o_keys);
		G.start = reinterpret_cast<uint32_t *>(d + o_start);
		G.sorted = sorted;
		G.slots = slots;
		HIPCHK(ctx, launch_sor_build(st, pts, n, G, sorted, reinterpret_cast<uint32_t *>(d + o_slot), counts, scan_tmp, hdr));
		HIPCHK(ctx, launch_sor_search(st, G, pts, qlist, nq, kk, dist, left[level & 1], &hdr->n_left[level]));
		HIPCHK(ctx, hipMemcpyAsync(h + 1024, hdr, sizeof(SorHeader), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		std::memcpy(&H, h + 1024, sizeof(H));
		if (H.overflow)
		{
			ctx->err = "mulls_sor_filter: a cell coordinate does not fit 21 bits";
			return MULLS_E_UNSUPPORTED;
		}
		nq = H.n_left[level];
		qlist = left[level & 1];
	}
	n_fallback = nq;
	for (uint32_t first = 0; first < n_fallback; first += BRUTE_QUERIES_PER_LAUNCH)
		HIPCHK(ctx, launch_sor_brute(st, pts, n, 1u, qlist + first, std::min(BRUTE_QUERIES_PER_LAUNCH, n_fallback - first), kk, dist, nullptr));

	// statistics, flags, compaction; one download: header, kept indices, and the distances when asked for
	SorHeader *res = reinterpret_cast<SorHeader *>(d + o_res);
	HIPCHK(ctx, hipMemsetAsync(res, 0, sizeof(SorHeader), st));
	HIPCHK(ctx, launch_sor_finish(st, dist, n, params->std_mul, reinterpret_cast<double *>(d + o_part), reinterpret_cast<uint32_t *>(d + o_flags),
								  reinterpret_cast<uint32_t *>(d + o_pos), scan_tmp, d_kept, res));
	const size_t down = (mean_dist ? o_dist + (size_t)n * 4u : o_kept + (size_t)n * 4u) - o_res;
	HIPCHK(ctx, hipMemcpyAsync(h, d + o_res, down, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::memcpy(&H, h, sizeof(H));
	const int32_t *h_kept = reinterpret_cast<const int32_t *>(h + (o_kept - o_res));
	const uint32_t n_kept = H.n_kept;
	*n_out = n_kept;
	if (kept_idx)
		std::memcpy(kept_idx, h_kept, (size_t)std::min(n_kept, idx_cap) * 4u);
	if (mean_dist)
		std::memcpy(mean_dist, h + (o_dist - o_res), (size_t)n * 4u);
	const uint32_t n_rec = std::min(n_kept, cap);
	if (n_rec)
	{
		if (on_dev)
		{
			if (int rc = grow(ctx, &sc.out, &sc.out_cap, (size_t)n_rec * MULLS_POINT_BYTES))
				return rc;
			HIPCHK(ctx, launch_sor_emit(st, Cl.pts, d_kept, n_rec, sc.out));
			HIPCHK(ctx, hipMemcpyAsync(out, sc.out, (size_t)n_rec * MULLS_POINT_BYTES, hipMemcpyDeviceToHost, st));
			HIPCHK(ctx, hipStreamSynchronize(st));
		}
		else
		{
			const unsigned char *p = static_cast<const unsigned char *>(Cl.pts);
			unsigned char *o = static_cast<unsigned char *>(out);
			for (uint32_t j = 0; j < n_rec; j++)
				std::memcpy(o + (size_t)j * MULLS_POINT_BYTES, p + (size_t)(uint32_t)h_kept[j] * Cl.stride, MULLS_POINT_BYTES);
		}
	}
	if (report)
	{
		report->n_in = n;
		report->n_kept = n_kept;
		report->mean = H.mean, report->stddev = H.stddev, report->threshold = H.threshold;
		report->n_fallback = n_fallback;
		report->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	}
	return MULLS_OK;
}
} // namespace

extern "C"
{
	void mulls_sor_default_params(mulls_sor_params *p)
	{
		if (!p)
			return;
		p->mean_k = 20; // mulls_slam.cpp:1009
		p->reserved = 0;
		p->std_mul = 2.0;
	}

	int mulls_sor_filter(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_sor_params *params, void *out, uint32_t cap, uint32_t *n_out, int32_t *kept_idx,
						 uint32_t idx_cap, float *mean_dist, mulls_sor_report *report)
	try
	{
		return sor_run(ctx, cloud, params, out, cap, n_out, kept_idx, idx_cap, mean_dist, report);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}
}
