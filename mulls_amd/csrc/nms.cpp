// nms.cpp — mulls_non_max_suppress: CFilter<PointT>::non_max_suppress (cfilter.hpp:1183-1312), the thinning of the key points in front of the global
// registration (test/mulls_reg.cpp:145-149) and of loop closure (test/mulls_slam.cpp:462), on the device.  Host side: argument checks, the visiting order
// (nms_host.h: the std::sort upstream runs), staging the records in that order, the choice of the path, one or two downloads.  include/mulls_hip.h has the
// definition this file follows.
//   path 1   k_nms.hip: one workgroup, the cloud in LDS, rounds separated by barriers; one launch, one download.  On request only: it measures slower
//            mulls_non_max_suppress_batch runs the same kernel body with one workgroup per problem (nms_batch.h: the sub-batches and their arena)
//   path 2   the class-cloud suppression of mulls_classify_nground through one class slot (launch_cl_nms_lists, launch_cl_nms_round in batches with a
//            host poll between them, rounds.h), then the stable compaction of map_kernels.hip
#include <chrono>
#include <cmath>
#include <string>

#include "classify_launch.h"
#include "ctx.h"
#include "map_launch.h"
#include "nms_host.h"
#include "nms_launch.h"
#include "rounds.h"
#include "subbatch.h"

// a context's scratch of this entry point: one device arena, one pinned host buffer; grow-only
struct mulls_nms_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr;
	size_t dev_cap = 0, pin_cap = 0;
	uint32_t rounds_hint = 8; // rounds the multi-launch path needed in the previous call: this call's first batch
	unsigned char *bdev = nullptr, *bpin = nullptr; // mulls_non_max_suppress_batch: a sub-batch's arena and its pinned mirror (nms_batch.h); grow-only
	size_t bdev_cap = 0, bpin_cap = 0;
};

void mulls_nms_release(mulls_ctx *ctx)
{
	if (!ctx->nms)
		return;
	staggered_free(ctx->nms->dev);
	if (ctx->nms->pin)
		(void)hipHostFree(ctx->nms->pin);
	staggered_free(ctx->nms->bdev);
	if (ctx->nms->bpin)
		(void)hipHostFree(ctx->nms->bpin);
	delete ctx->nms;
	ctx->nms = nullptr;
}

namespace
{
constexpr size_t REC = MULLS_POINT_BYTES;
constexpr size_t HDR_BYTES = 256;

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

int nms_run(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_nms_params *params, void *out, uint32_t cap, uint32_t *n_out, int32_t *kept_idx, uint32_t idx_cap,
			int32_t *order, mulls_nms_report *report)
{
	const auto t0 = std::chrono::steady_clock::now();
	if (!ctx || !cloud || !params || (cap && !out) || (idx_cap && !kept_idx))
		return MULLS_E_INVALID;
	if (n_out)
		*n_out = 0;
	if (report)
		std::memset(report, 0, sizeof(*report));
	const mulls_cloud Cl = *cloud;
	const uint32_t n = Cl.n;
	if (n && !Cl.pts)
		return MULLS_E_INVALID;
	if (!std::isfinite(params->non_max_radius))
	{
		ctx->err = "mulls_non_max_suppress: the radius is not finite";
		return MULLS_E_INVALID;
	}
	if (params->path < 0 || params->path > 2)
	{
		ctx->err = "mulls_non_max_suppress: path is 0, 1 or 2";
		return MULLS_E_INVALID;
	}
	if (n == 0)
		return MULLS_OK;
	if (n > MULLS_NMS_MAX_POINTS)
	{
		ctx->err = "mulls_non_max_suppress: more than 2^18 = 262144 points";
		return MULLS_E_UNSUPPORTED;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const bool on_dev = cloud_on_device(ctx, Cl);
	if (on_dev ? Cl.stride != REC : (Cl.stride < REC || Cl.stride % 4u))
	{
		ctx->err = "mulls_non_max_suppress: stride (device clouds: 48; host clouds: a multiple of 4, at least 48)";
		return MULLS_E_INVALID;
	}
	const bool gate = n < 10u; // :1189-1191
	int path = 0;
	if (!gate)
	{
		// path 0: the multi-launch path at every size.  Measured (profiles/nms_kernel_stats.txt): on the demo key points and at 4096 points one workgroup takes
		// 0.65 - 0.80 ms per call against 0.20 - 0.25 ms — one CU issues the neighbour walks of 4096 points slower than 256 CUs test all pairs
		path = params->path ? params->path : 2;
		if (path == 1 && n > MULLS_NMS_LDS_MAX_POINTS)
		{
			ctx->err = "mulls_non_max_suppress: path 1 holds at most 4096 points";
			return MULLS_E_UNSUPPORTED;
		}
	}
	if (!ctx->nms)
		ctx->nms = new mulls_nms_scratch();
	mulls_nms_scratch &sc = *ctx->nms;

	// the device arena: what both paths use, then path 2's lists (sized as classify.cpp sizes a class slot)
	const uint32_t pool_cap = (uint32_t)std::min<size_t>((size_t)n * 64u, 0x7fffffffu);
	const size_t seg_cap = (size_t)6 * ((n + 4095u) / 4096u + 1u) + 16;
	size_t off = 0;
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return at;
	};
	const size_t o_src = take(on_dev ? (size_t)n * 4u : 0), o_perm = take(on_dev ? (size_t)n * 4u : 0); // a device cloud's keys, its visiting order
	const size_t o_recs = take((size_t)n * REC), o_out = take((size_t)n * REC);
	// what comes down, contiguous: header, kept positions (path 1) or header, round counters, compaction counts, keep mask (path 2)
	const size_t o_hdr = take(HDR_BYTES - 1), o_kept = take((size_t)n * 4u);
	size_t o_rcnt = 0, o_cnt6 = 0, o_keep = 0, o_list = 0, o_lcnt = 0, o_loff = 0, o_wcur = 0, o_pool = 0, o_used = 0, o_seg = 0;
	if (path == 2)
	{
		o_rcnt = take(64 * 4u), o_cnt6 = take(6 * 4u), o_keep = take(n);
		o_list = take((size_t)n * MULLS_CL_NMS_CAP * 4u), o_lcnt = take((size_t)n * 4u), o_loff = take((size_t)n * 4u), o_wcur = take((size_t)n * 4u);
		o_pool = take((size_t)pool_cap * 4u), o_used = take(8), o_seg = take(seg_cap * 4u);
	}
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
		return rc;
	// pinned: the records in visiting order on their way up / the kept ones on their way down; keys, permutation, header and positions behind them
	const size_t p_keys = up256((size_t)n * REC), p_perm = p_keys + up256((size_t)n * 4u), p_res = p_perm + up256((size_t)n * 4u);
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, p_res + up256(HDR_BYTES) + up256((size_t)n * 4u) + 4096u, hipHostMallocDefault))
		return rc;
	static_assert(sizeof(NmsHeader) <= HDR_BYTES, "NmsHeader");
	unsigned char *d = sc.dev, *h = sc.pin;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	float *keys = reinterpret_cast<float *>(h + p_keys);
	uint32_t *perm = reinterpret_cast<uint32_t *>(h + p_perm);
	float4 *recs = reinterpret_cast<float4 *>(d + o_recs), *d_out = reinterpret_cast<float4 *>(d + o_out);
	const unsigned char *src = static_cast<const unsigned char *>(Cl.pts);

	// keys (and the coordinates' check); under the gate only the check
	if (on_dev)
	{
		HIPCHK(ctx, hipMemsetAsync(d + o_hdr, 0, HDR_BYTES, st));
		HIPCHK(ctx, launch_nms_keys(st, Cl.pts, n, reinterpret_cast<float *>(d + o_src), reinterpret_cast<uint32_t *>(d + o_hdr)));
		HIPCHK(ctx, hipMemcpyAsync(keys, d + o_src, (size_t)n * 4u, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipMemcpyAsync(h + p_res, d + o_hdr, 4, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		uint32_t bad;
		std::memcpy(&bad, h + p_res, 4);
		if (bad)
		{
			ctx->err = "mulls_non_max_suppress: a coordinate is not finite";
			return MULLS_E_INVALID;
		}
	}
	else
		for (uint32_t i = 0; i < n; i++)
		{
			float v[3];
			std::memcpy(v, src + (size_t)i * Cl.stride, 12);
			std::memcpy(&keys[i], src + (size_t)i * Cl.stride + 28u, 4);
			if (!(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2])))
			{
				ctx->err = "mulls_non_max_suppress: a coordinate is not finite";
				return MULLS_E_INVALID;
			}
		}
	const uint32_t n_rec_max = std::min(n, cap);
	if (gate)
	{
		// the cloud as it is, in input order
		if (n_rec_max)
		{
			if (on_dev)
			{
				HIPCHK(ctx, hipMemcpyAsync(out, Cl.pts, (size_t)n_rec_max * REC, hipMemcpyDeviceToHost, st));
				HIPCHK(ctx, hipStreamSynchronize(st));
			}
			else
				for (uint32_t j = 0; j < n_rec_max; j++)
					std::memcpy(static_cast<unsigned char *>(out) + (size_t)j * REC, src + (size_t)j * Cl.stride, REC);
		}
		for (uint32_t j = 0; j < std::min(n, idx_cap); j++)
			kept_idx[j] = (int32_t)j;
		if (order)
			for (uint32_t j = 0; j < n; j++)
				order[j] = (int32_t)j;
		if (n_out)
			*n_out = n;
		if (report)
		{
			report->n_in = report->n_kept = n;
			report->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
		}
		return MULLS_OK;
	}
	for (uint32_t i = 0; i < n; i++)
		if (std::isnan(keys[i]))
		{
			ctx->err = "mulls_non_max_suppress: a key (normal[3]) is NaN: upstream's sort is undefined";
			return MULLS_E_INVALID;
		}
	nms_visiting_order(keys, n, perm);
	if (order)
		std::memcpy(order, perm, (size_t)n * 4u);

	// the records in visiting order on the device
	if (on_dev)
	{
		HIPCHK(ctx, hipMemcpyAsync(d + o_perm, perm, (size_t)n * 4u, hipMemcpyHostToDevice, st));
		launch_cl_gather(st, static_cast<const float4 *>(Cl.pts), reinterpret_cast<const uint32_t *>(d + o_perm), recs, n);
	}
	else
	{
		for (uint32_t i = 0; i < n; i++)
			std::memcpy(h + (size_t)i * REC, src + (size_t)perm[i] * Cl.stride, REC);
		HIPCHK(ctx, hipMemcpyAsync(recs, h, (size_t)n * REC, hipMemcpyHostToDevice, st));
	}
	const float r = params->non_max_radius;
	const float r2 = (float)((double)r * (double)r);
	uint32_t n_kept = 0, rounds = 0;
	std::vector<uint32_t> pos_host;		 // path 2: the kept positions, from the keep mask
	const uint32_t *kept_pos = nullptr; // positions in visiting order, ascending
	if (path == 1)
	{
		NmsHeader *hdr = reinterpret_cast<NmsHeader *>(d + o_hdr);
		HIPCHK(ctx, launch_nms_one(st, recs, n, r, hdr, reinterpret_cast<uint32_t *>(d + o_kept), n_rec_max ? d_out : nullptr, n_rec_max));
		HIPCHK(ctx, hipMemcpyAsync(h + p_res, d + o_hdr, up256(HDR_BYTES) + (size_t)n * 4u, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st)); // (also: the pinned records have gone up)
		NmsHeader H;
		std::memcpy(&H, h + p_res, sizeof(H));
		n_kept = H.n_kept, rounds = H.rounds;
		kept_pos = reinterpret_cast<const uint32_t *>(h + p_res + up256(HDR_BYTES));
	}
	else
	{
		ClNmsArgs na;
		std::memset(&na, 0, sizeof(na));
		na.r2 = r2;
		na.recs[0] = recs, na.n[0] = n;
		na.keep[0] = d + o_keep;
		na.list[0] = reinterpret_cast<uint32_t *>(d + o_list), na.cnt[0] = reinterpret_cast<uint32_t *>(d + o_lcnt);
		na.off[0] = reinterpret_cast<uint32_t *>(d + o_loff), na.wcur[0] = reinterpret_cast<uint32_t *>(d + o_wcur);
		na.pool = reinterpret_cast<uint32_t *>(d + o_pool), na.pool_used = reinterpret_cast<unsigned long long *>(d + o_used), na.pool_cap = pool_cap;
		uint32_t *round_cnt = reinterpret_cast<uint32_t *>(d + o_rcnt);
		launch_cl_nms_lists(st, na, round_cnt); // (zeroes the pool cursor and the round counters with its own arrays)
		if (int rc = run_rounds(ctx, st, round_cnt, 8u, &sc.rounds_hint, [&](uint32_t slot) { launch_cl_nms_round(st, na, round_cnt + slot); },
								"mulls_non_max_suppress: the suppression rounds did not settle"))
			return rc;
		rounds = sc.rounds_hint;
		MapCompactArgs ca;
		std::memset(&ca, 0, sizeof(ca));
		ca.cloud[0].in = recs, ca.cloud[0].out = d_out, ca.cloud[0].mask = na.keep[0], ca.cloud[0].n = n;
		ca.out_n = reinterpret_cast<uint32_t *>(d + o_cnt6);
		ca.mode = 0;
		if (n_rec_max)
			launch_map_compact(st, ca, reinterpret_cast<uint32_t *>(d + o_seg));
		HIPCHK(ctx, hipMemcpyAsync(h + p_res, d + o_keep, n, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		const unsigned char *keep = h + p_res;
		pos_host.reserve(n);
		for (uint32_t i = 0; i < n; i++)
			if (keep[i])
				pos_host.push_back(i);
		n_kept = (uint32_t)pos_host.size();
		kept_pos = pos_host.data();
	}
	if (n_kept > n) // (never: the positions below index the permutation)
	{
		ctx->err = "mulls_non_max_suppress: the device reported more kept points than points";
		return MULLS_E_HIP;
	}
	if (n_out)
		*n_out = n_kept;
	for (uint32_t j = 0; j < std::min(n_kept, idx_cap); j++)
		kept_idx[j] = (int32_t)perm[kept_pos[j]];
	const uint32_t n_rec = std::min(n_kept, cap);
	if (n_rec)
	{
		HIPCHK(ctx, hipMemcpyAsync(out, d_out, (size_t)n_rec * REC, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	if (report)
	{
		report->n_in = n;
		report->n_kept = n_kept;
		report->ran = 1;
		report->path = path;
		report->rounds = rounds;
		report->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	}
	return MULLS_OK;
}

// ---- mulls_non_max_suppress_batch
struct BatchProblem
{
	bool on_dev = false;
	std::vector<unsigned char> gate_recs; // a device-resident cloud below the gate: its records, read by the check
};

int batch_refuse(mulls_ctx *ctx, uint32_t b, int rc, const char *what)
{
	ctx->err = "mulls_non_max_suppress_batch: problem " + std::to_string(b) + ": " + what;
	return rc;
}

bool finite3(const unsigned char *rec)
{
	float v[3];
	std::memcpy(v, rec, 12);
	return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
}

int nms_batch_run(mulls_ctx *ctx, const mulls_nms_problem *problems, uint32_t B, const mulls_nms_params *params, uint64_t scratch_limit_bytes,
				  mulls_nms_report *reports)
{
	const auto t0 = std::chrono::steady_clock::now();
	if (!ctx)
		return MULLS_E_INVALID;
	if (B == 0)
		return MULLS_OK;
	if (!problems)
	{
		ctx->err = "mulls_non_max_suppress_batch: problems is NULL";
		return MULLS_E_INVALID;
	}
	if (reports)
		std::memset(reports, 0, sizeof(*reports) * (size_t)B);
	if (!params)
		return batch_refuse(ctx, 0, MULLS_E_INVALID, "params is NULL");
	if (!std::isfinite(params->non_max_radius))
		return batch_refuse(ctx, 0, MULLS_E_INVALID, "the radius is not finite");
	if (params->path < 0 || params->path > 2)
		return batch_refuse(ctx, 0, MULLS_E_INVALID, "path is 0, 1 or 2");
	HIPCHK(ctx, hipSetDevice(ctx->device));

	// the arguments and the host clouds, before any device work: the single call's checks in the single call's order
	std::vector<BatchProblem> prob(B);
	std::vector<NmsBatchShape> shape(B);
	for (uint32_t b = 0; b < B; b++)
	{
		const mulls_nms_problem &P = problems[b];
		const mulls_cloud &Cl = P.cloud;
		const uint32_t n = Cl.n;
		if ((P.cap && !P.out) || (P.idx_cap && !P.kept_idx) || (n && !Cl.pts))
			return batch_refuse(ctx, b, MULLS_E_INVALID, "a pointer that is needed is NULL");
		shape[b] = NmsBatchShape{Cl.pts, n, Cl.stride, P.cap, 0u, 0u, ~0u};
		if (n == 0)
			continue;
		if (n > MULLS_NMS_MAX_POINTS)
			return batch_refuse(ctx, b, MULLS_E_UNSUPPORTED, "more than 2^18 = 262144 points");
		const bool on_dev = prob[b].on_dev = cloud_on_device(ctx, Cl);
		if (on_dev ? Cl.stride != REC : (Cl.stride < REC || Cl.stride % 4u))
			return batch_refuse(ctx, b, MULLS_E_INVALID, "stride (device clouds: 48; host clouds: a multiple of 4, at least 48)");
		if (n >= 10u && params->path == 1 && n > MULLS_NMS_LDS_MAX_POINTS)
			return batch_refuse(ctx, b, MULLS_E_UNSUPPORTED, "path 1 holds at most 4096 points");
		shape[b].on_dev = on_dev ? 1u : 0u;
		shape[b].lds = nms_batch_takes_lds(n, params->path);
		if (on_dev)
			continue;
		const unsigned char *src = static_cast<const unsigned char *>(Cl.pts);
		for (uint32_t i = 0; i < n; i++)
			if (!finite3(src + (size_t)i * Cl.stride))
				return batch_refuse(ctx, b, MULLS_E_INVALID, "a coordinate is not finite");
		for (uint32_t i = 0; i < n && n >= 10u; i++)
		{
			float key;
			std::memcpy(&key, src + (size_t)i * Cl.stride + 28u, 4);
			if (std::isnan(key))
				return batch_refuse(ctx, b, MULLS_E_INVALID, "a key (normal[3]) is NaN: upstream's sort is undefined");
		}
	}

	// the sub-batches and their arenas
	std::vector<uint32_t> cuts;
	nms_batch_cuts(shape.data(), B, scratch_limit_bytes, &cuts);
	const uint32_t n_sub = (uint32_t)cuts.size() - 1u;
	std::vector<NmsBatchLayout> layout(n_sub);
	size_t need = 0;
	for (uint32_t k = 0; k < n_sub; k++)
	{
		nms_batch_layout(shape.data() + cuts[k], cuts[k + 1] - cuts[k], &layout[k]);
		need = std::max<size_t>(need, layout[k].dev_bytes);
	}
	if (!ctx->nms)
		ctx->nms = new mulls_nms_scratch();
	mulls_nms_scratch &sc = *ctx->nms;
	if (need)
	{
		if (int rc = grow(ctx, &sc.bdev, &sc.bdev_cap, need))
			return rc;
		if (int rc = grow_pinned(ctx, &sc.bpin, &sc.bpin_cap, need, hipHostMallocDefault))
			return rc;
	}
	unsigned char *d = sc.bdev, *h = sc.bpin;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	static_assert(sizeof(NmsBatchDesc) % 8 == 0 && sizeof(NmsBatchSrc) % 8 == 0 && sizeof(NmsBatchHeader) == 16, "the records of nms_batch.h");

	// the head of a sub-batch in the pinned mirror
	auto write_head = [&](uint32_t k) {
		NmsBatchLayout &L = layout[k];
		for (const NmsBatchStaged &S : L.staged)
			if (S.src != ~0u)
				L.src[S.src].src = (uint64_t)(uintptr_t)problems[cuts[k] + S.owner].cloud.pts;
		if (!L.desc.empty())
			std::memcpy(h + L.o_desc, L.desc.data(), sizeof(NmsBatchDesc) * L.desc.size());
		if (!L.src.empty())
			std::memcpy(h + L.o_src, L.src.data(), sizeof(NmsBatchSrc) * L.src.size());
		std::memcpy(h + L.o_blk, L.blk.data(), 4u * L.blk.size());
	};

	// the key pass over the device-resident clouds of every sub-batch (and the records of those below the gate): nothing is written before all of them
	// have passed.  dev_keys: the keys of sub-batch k's staged cloud s at key_at[k][s]
	std::vector<float> dev_keys;
	std::vector<std::vector<size_t>> key_at(n_sub);
	for (uint32_t b = 0; b < B; b++)
		if (prob[b].on_dev && problems[b].cloud.n < 10u)
		{
			const uint32_t n = problems[b].cloud.n;
			prob[b].gate_recs.resize((size_t)n * REC);
			HIPCHK(ctx, hipMemcpyAsync(prob[b].gate_recs.data(), problems[b].cloud.pts, (size_t)n * REC, hipMemcpyDeviceToHost, st));
			HIPCHK(ctx, hipStreamSynchronize(st));
			for (uint32_t i = 0; i < n; i++)
				if (!finite3(prob[b].gate_recs.data() + (size_t)i * REC))
					return batch_refuse(ctx, b, MULLS_E_INVALID, "a coordinate is not finite");
		}
	for (uint32_t k = 0; k < n_sub; k++)
	{
		NmsBatchLayout &L = layout[k];
		key_at[k].assign(L.staged.size(), 0);
		if (L.src.empty())
			continue;
		write_head(k);
		HIPCHK(ctx, hipMemcpyAsync(d, h, L.head_bytes, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, hipMemsetAsync(d + L.o_bad, 0, 4u * L.src.size(), st));
		HIPCHK(ctx, launch_nms_batch_keys(st, d, L));
		HIPCHK(ctx, hipMemcpyAsync(h + L.o_keys, d + L.o_keys, (size_t)(L.o_bad - L.o_keys) + 4u * L.src.size(), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		const uint32_t *bad = reinterpret_cast<const uint32_t *>(h + L.o_bad);
		for (size_t s = 0; s < L.staged.size(); s++) // (in the order of the clouds' first problems)
		{
			const NmsBatchStaged &S = L.staged[s];
			if (S.src == ~0u)
				continue;
			if (bad[S.src])
				return batch_refuse(ctx, cuts[k] + S.owner, MULLS_E_INVALID, "a coordinate is not finite");
			const float *keys = reinterpret_cast<const float *>(h + S.keys);
			for (uint32_t i = 0; i < S.n; i++)
				if (std::isnan(keys[i]))
					return batch_refuse(ctx, cuts[k] + S.owner, MULLS_E_INVALID, "a key (normal[3]) is NaN: upstream's sort is undefined");
			key_at[k][s] = dev_keys.size();
			dev_keys.insert(dev_keys.end(), keys, keys + S.n);
		}
	}

	const float radius = params->non_max_radius;
	for (uint32_t k = 0; k < n_sub; k++)
	{
		NmsBatchLayout &L = layout[k];
		const uint32_t b0 = cuts[k], count = cuts[k + 1] - cuts[k];
		std::vector<std::vector<uint32_t>> perm(L.staged.size());
		if (!L.desc.empty())
		{
			// the orders, and the host clouds' records in visiting order, per staged cloud on the pool
			shared_host_pool().parallel_for(0, (long)L.staged.size(), 1, [&](long s) {
				const NmsBatchStaged &S = L.staged[s];
				if (!S.lds)
					return;
				const mulls_cloud &Cl = problems[b0 + S.owner].cloud;
				const unsigned char *src = static_cast<const unsigned char *>(Cl.pts);
				std::vector<uint32_t> &pm = perm[s];
				pm.resize(S.n);
				if (S.on_dev)
				{
					nms_visiting_order(dev_keys.data() + key_at[k][s], S.n, pm.data());
					std::memcpy(h + S.perm, pm.data(), (size_t)S.n * 4u);
					return;
				}
				std::vector<float> keys(S.n);
				for (uint32_t i = 0; i < S.n; i++)
					std::memcpy(&keys[i], src + (size_t)i * Cl.stride + 28u, 4);
				nms_visiting_order(keys.data(), S.n, pm.data());
				for (uint32_t i = 0; i < S.n; i++)
					std::memcpy(h + S.recs + (size_t)i * REC, src + (size_t)pm[i] * Cl.stride, REC);
			});
			write_head(k);
			HIPCHK(ctx, hipMemcpyAsync(d, h, L.up_bytes, hipMemcpyHostToDevice, st));
			HIPCHK(ctx, launch_nms_batch_gather(st, d, L));
			HIPCHK(ctx, hipMemsetAsync(d + L.o_cursor, 0, 4, st));
			HIPCHK(ctx, launch_nms_batch(st, d, L, radius));
			HIPCHK(ctx, hipMemcpyAsync(h + L.o_cursor, d + L.o_cursor, L.down_bytes, hipMemcpyDeviceToHost, st));
			HIPCHK(ctx, hipStreamSynchronize(st));
			uint32_t reserved;
			std::memcpy(&reserved, h + L.o_cursor, 4);
			if (reserved > L.out_records)
			{
				ctx->err = "mulls_non_max_suppress_batch: the device reserved more kept records than the problems may return";
				return MULLS_E_HIP;
			}
			if (reserved)
			{
				HIPCHK(ctx, hipMemcpyAsync(h + L.o_out, d + L.o_out, (size_t)reserved * REC, hipMemcpyDeviceToHost, st));
				HIPCHK(ctx, hipStreamSynchronize(st));
			}
			for (const NmsBatchDesc &D : L.desc)
			{
				NmsBatchHeader H;
				std::memcpy(&H, h + D.hdr, sizeof(H));
				const uint32_t n_rec = std::min(H.n_kept, D.out_cap);
				if (H.n_kept > D.n || (uint64_t)H.out_at + n_rec > reserved)
				{
					ctx->err = "mulls_non_max_suppress_batch: the device reported more kept points than points";
					return MULLS_E_HIP;
				}
				const uint32_t b = b0 + D.problem;
				const mulls_nms_problem &P = problems[b];
				const std::vector<uint32_t> &pm = perm[shape[b].stage];
				const uint32_t *kept_pos = reinterpret_cast<const uint32_t *>(h + D.kept);
				if (n_rec)
					std::memcpy(P.out, h + L.o_out + (size_t)H.out_at * REC, (size_t)n_rec * REC);
				for (uint32_t j = 0; j < std::min(H.n_kept, P.idx_cap); j++)
					P.kept_idx[j] = (int32_t)pm[kept_pos[j]];
				if (P.order)
					std::memcpy(P.order, pm.data(), (size_t)D.n * 4u);
				if (reports)
				{
					mulls_nms_report &R = reports[b];
					R.n_in = D.n, R.n_kept = H.n_kept, R.ran = 1, R.path = 1, R.rounds = H.rounds;
				}
			}
		}
		// what takes no workgroup: the empty clouds, the clouds below the gate (the identity), and the multi-launch path, each as the single call runs it
		for (uint32_t b = b0; b < b0 + count; b++)
		{
			const mulls_nms_problem &P = problems[b];
			const uint32_t n = P.cloud.n;
			if (shape[b].lds || n == 0)
				continue;
			if (n < 10u)
			{
				const unsigned char *src = static_cast<const unsigned char *>(P.cloud.pts);
				for (uint32_t j = 0; j < std::min(n, P.cap); j++)
					std::memcpy(static_cast<unsigned char *>(P.out) + (size_t)j * REC,
								prob[b].on_dev ? prob[b].gate_recs.data() + (size_t)j * REC : src + (size_t)j * P.cloud.stride, REC);
				for (uint32_t j = 0; j < std::min(n, P.idx_cap); j++)
					P.kept_idx[j] = (int32_t)j;
				for (uint32_t j = 0; j < n && P.order; j++)
					P.order[j] = (int32_t)j;
				if (reports)
					reports[b].n_in = reports[b].n_kept = n;
				continue;
			}
			mulls_nms_params one = *params;
			one.path = 2;
			if (int rc = nms_run(ctx, &P.cloud, &one, P.out, P.cap, nullptr, P.kept_idx, P.idx_cap, P.order, reports ? &reports[b] : nullptr))
			{
				ctx->err = "mulls_non_max_suppress_batch: problem " + std::to_string(b) + ": " + ctx->err;
				return rc;
			}
		}
	}
	const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	for (uint32_t b = 0; b < B && reports; b++)
		reports[b].ms_total = ms;
	return MULLS_OK;
}
} // namespace

extern "C"
{
	void mulls_nms_default_params(mulls_nms_params *p)
	{
		if (!p)
			return;
		p->non_max_radius = 0.25f; // 0.25 * pca_neigh_r with the reference's pca_neigh_r = 1.0 (test/mulls_reg.cpp:107)
		p->path = 0;
	}

	int mulls_non_max_suppress(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_nms_params *params, void *out, uint32_t cap, uint32_t *n_out, int32_t *kept_idx,
							   uint32_t idx_cap, int32_t *order, mulls_nms_report *report)
	try
	{
		return nms_run(ctx, cloud, params, out, cap, n_out, kept_idx, idx_cap, order, report);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_non_max_suppress_batch(mulls_ctx *ctx, const mulls_nms_problem *problems, uint32_t n_problems, const mulls_nms_params *params,
									 uint64_t scratch_limit_bytes, mulls_nms_report *reports)
	try
	{
		return nms_batch_run(ctx, problems, n_problems, params, scratch_limit_bytes, reports);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	uint64_t mulls_nms_batch_arena_bytes(const mulls_ctx *ctx) { return ctx && ctx->nms ? (uint64_t)ctx->nms->bdev_cap : 0u; }
}
