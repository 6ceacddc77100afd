// map.cpp — device-resident local map (include/mulls_hip.h, "mulls_map_*"): MapManager::update_local_map
// (src/map_manager.cpp:18-140) and map-based dynamic-object removal (:149-268) on class clouds that stay in HBM between
// frames.  Kernels: map_kernels.hip (+ k_transform_aos of k_reduce.hip).  As everywhere in this library there is no CPU
// fallback: the only host-side arithmetic is the pose algebra, the kept-point counts and the seeded selection masks.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cmath>
#include <cstdlib>

#include "batch.h"
#include "ctx.h"
#include "device_types.h"
#include "hostmath.h"
#include "launch.h"
#include "map_internal.h"
#include "map_launch.h"

using namespace mulls_mapi; // (the map and the per-phase host arithmetic: map_internal.h, shared with map_batch.cpp)

bool mulls_is_map_memory(const mulls_ctx *ctx, const void *p, size_t bytes)
{
	const char *q = (const char *)p;
	for (const mulls_map *m : ctx->maps)
		for (int c = 0; c < MULLS_NC; c++)
		{
			const char *lo = (const char *)m->rec[c];
			if (lo && q >= lo && q + bytes <= lo + m->cap[c] * 3 * sizeof(float4))
				return true;
		}
	for (const mulls_block *b : ctx->blocks)
		if (b->buf && q >= (const char *)b->buf && q + bytes <= (const char *)b->buf + b->cap)
			return true;
	return mulls_submaps_memory(ctx, p, bytes);
}

bool mulls_map_snapshot(const mulls_ctx *ctx, const mulls_map *m, MapSnapshot *out)
{
	if (std::find(ctx->maps.begin(), ctx->maps.end(), m) == ctx->maps.end())
		return false;
	for (int c = 0; c < MULLS_NC; c++)
	{
		out->rec[c] = m->rec[c];
		out->n[c] = m->n[c];
	}
	std::memcpy(out->pose, m->pose, sizeof(m->pose));
	out->has_bounds = m->has_bounds;
	std::memcpy(out->local_bound, m->local_bound, sizeof(m->local_bound));
	std::memcpy(out->bound, m->bound, sizeof(m->bound));
	return true;
}

namespace
{
// capacity in records; keeps the contents when `keep_n` > 0
int reserve(mulls_ctx *ctx, float4 **p, size_t *cap, size_t need, size_t keep_n)
{
	if (*p && *cap >= need)
		return MULLS_OK;
	const size_t want = std::max<size_t>(need + need / 2, 1024);
	float4 *q = nullptr;
	HIPCHK(ctx, hipMalloc((void **)&q, want * REC));
	if (*p && keep_n)
		HIPCHK(ctx, hipMemcpyAsync(q, *p, keep_n * REC, hipMemcpyDeviceToDevice, ctx->stream));
	if (*p)
	{
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		(void)hipFree(*p);
	}
	*p = q;
	*cap = want;
	return MULLS_OK;
}

// the six clouds of a frame / a map at once: device-resident sources (a feature block's, another map's) move in one launch and nobody waits; host sources are
// copied one by one and waited for once
int upload_clouds(mulls_ctx *ctx, const mulls_cloud clouds[MULLS_NC], float4 **dst, size_t *cap)
{
	std::vector<unsigned char> pack[MULLS_NC];
	SegCopier dev(ctx);
	bool any_host = false;
	for (int c = 0; c < MULLS_NC; c++)
	{
		const mulls_cloud &cl = clouds[c];
		if (cl.n && (!cl.pts || cl.stride < REC))
		{
			ctx->err = "cloud with points but null pointer or stride < 48";
			return MULLS_E_INVALID;
		}
		const int rc = reserve(ctx, &dst[c], &cap[c], cl.n, 0);
		if (rc != MULLS_OK)
			return rc;
		if (!cl.n)
			continue;
		if (cl.stride == REC && mulls_is_map_memory(ctx, cl.pts, (size_t)cl.n * REC))
		{
			dev.add_dev(dst[c], cl.pts, (size_t)cl.n * REC);
			continue;
		}
		const void *src = cl.pts;
		if (cl.stride != REC)
		{
			pack[c].resize((size_t)cl.n * REC);
			for (uint32_t i = 0; i < cl.n; i++)
				std::memcpy(pack[c].data() + (size_t)i * REC, (const unsigned char *)cl.pts + (size_t)i * cl.stride, REC);
			src = pack[c].data();
		}
		HIPCHK(ctx, hipMemcpyAsync(dst[c], src, (size_t)cl.n * REC, hipMemcpyDefault, ctx->stream));
		any_host = true;
	}
	if (dev.flush(ctx->stream) != MULLS_OK)
		return MULLS_E_HIP;
	if (any_host)
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // `pack` / the caller's buffers may go away
	return MULLS_OK;
}

int compact(mulls_ctx *ctx, mulls_map *m, const MapCompactArgs &a)
{
	const size_t need = (size_t)map_compact_segments(a) + 8;
	if (m->cap_seg < need)
	{
		if (m->seg)
			(void)hipFree(m->seg);
		m->seg = nullptr;
		if (dmalloc(ctx, &m->seg, need * 2) != MULLS_OK)
			return MULLS_E_HIP;
		m->cap_seg = need * 2;
	}
	launch_map_compact(ctx->stream, a, m->seg);
	return MULLS_OK;
}

} // namespace

extern "C"
{
	void mulls_map_default_params(mulls_map_params *p)
	{
		std::memset(p, 0, sizeof(*p));
		p->local_map_radius = 80;
		p->max_num_pts = 20000;
		p->kept_vertex_num = 800;
		p->last_frame_reliable_radius = 60;
		std::strcpy(p->used_feature_type, "111110");
		p->dynamic_removal_center_radius = 30.0f;
		p->dynamic_dist_thre_min = 0.3f;
		p->dynamic_dist_thre_max = 3.0f;
		p->near_dist_thre = 0.03f;
		std::strcpy(p->tree_used, "000000");
	}

	int mulls_map_create(mulls_ctx *ctx, mulls_map **out)
	try
	{
		if (!ctx || !out)
			return MULLS_E_INVALID;
		*out = nullptr;
		HIPCHK(ctx, hipSetDevice(ctx->device));
		mulls_map *m = new mulls_map();
		if (dmalloc(ctx, &m->counts, 6) != MULLS_OK || dmalloc(ctx, &m->keys, 12) != MULLS_OK || dmalloc(ctx, &m->T12, 12) != MULLS_OK)
		{
			mulls_map_destroy(ctx, m);
			return MULLS_E_HIP;
		}
		ctx->maps.push_back(m);
		*out = m;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	void mulls_map_destroy(mulls_ctx *ctx, mulls_map *m)
	{
		if (!m)
			return;
		if (ctx)
		{
			(void)hipSetDevice(ctx->device);
			(void)hipStreamSynchronize(ctx->stream);
			ctx->maps.erase(std::remove(ctx->maps.begin(), ctx->maps.end(), m), ctx->maps.end());
		}
		for (int c = 0; c < MULLS_NC; c++)
		{
			void *p[] = {m->rec[c], m->alt[c], m->frame[c], m->frame_alt[c]};
			for (void *q : p)
				if (q)
					(void)hipFree(q);
		}
		void *p[] = {m->counts, m->keys, m->T12, m->best, m->keep, m->seg, m->dmask};
		for (void *q : p)
			if (q)
				(void)hipFree(q);
		delete m;
	}

	int mulls_map_set(mulls_ctx *ctx, mulls_map *m, const mulls_cloud clouds[6], const double pose_lo[16])
	try
	{
		if (!ctx || !m || !clouds || !pose_lo)
			return MULLS_E_INVALID;
		HIPCHK(ctx, hipSetDevice(ctx->device));
		const int rc_up = upload_clouds(ctx, clouds, m->rec, m->cap);
		if (rc_up != MULLS_OK)
			return rc_up;
		for (int c = 0; c < MULLS_NC; c++)
		{
			m->n[c] = clouds[c].n;
			m->frame_n[c] = 0;
		}
		std::memcpy(m->pose, pose_lo, sizeof(m->pose));
		m->has_bounds = false;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_map_update(mulls_ctx *ctx, mulls_map *m, const mulls_cloud frame_down[6], const double frame_pose_lo[16], const mulls_map_params *P,
						 mulls_map_report *rep)
	try
	{
		if (!ctx || !m || !frame_down || !frame_pose_lo || !P || !rep)
			return MULLS_E_INVALID;
		if (std::strlen(P->used_feature_type) < 6 || std::strlen(P->tree_used) < 6)
		{
			ctx->err = "used_feature_type and tree_used need 6 characters";
			return MULLS_E_INVALID;
		}
		HIPCHK(ctx, hipSetDevice(ctx->device));
		const auto wall0 = std::chrono::steady_clock::now();
		hipStream_t st = ctx->stream;
		std::memset(rep, 0, sizeof(*rep));
		m->has_bounds = false; // (until step 8 of this update)

		// 1. the frame's clouds on the device
		const int rc_up = upload_clouds(ctx, frame_down, m->frame, m->cap_frame);
		if (rc_up != MULLS_OK)
			return rc_up;
		for (int c = 0; c < MULLS_NC; c++)
			m->frame_n[c] = frame_down[c].n;
		// 2. tran_target_map = last_target.pose_lo^-1 * local_map.pose_lo (:28); the five *_down clouds go to the map frame (:32)
		UpdatePoses poses;
		update_poses(m->pose, frame_pose_lo, &poses);
		launch_transform_clouds(st, m->frame, m->frame_n, 5, poses.frame_to_map); // (the transform travels with the launch)

		// 3. map-based dynamic-object removal on the frame's pillar, beam and facade clouds (:37-47, :149-268)
		const float dmax = removal_dmax(P);
		const RemovalPlan plan = removal_plan(m, P);
		if (plan.ran)
		{
			rep->dynamic_removal_ran = 1;
			// the three classes side by side (nearest tree point, verdict), then ONE compaction and one read of the counts
			const int *order = removal_order();
			const bool *run = plan.run;
			const uint32_t *first = plan.first, total = plan.total;
			if (total)
			{
				if (m->cap_best < total)
				{
					HIPCHK(ctx, hipStreamSynchronize(st));
					if (m->best)
						(void)hipFree(m->best);
					if (m->keep)
						(void)hipFree(m->keep);
					m->best = nullptr, m->keep = nullptr;
					if (dmalloc(ctx, &m->best, (size_t)total * 2) != MULLS_OK || dmalloc(ctx, &m->keep, (size_t)total * 2) != MULLS_OK)
						return MULLS_E_HIP;
					m->cap_best = (size_t)total * 2;
				}
				HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)m->best, 0x7f800000, total, st));
				MapCompactArgs a;
				std::memset(&a, 0, sizeof(a));
				for (int k = 0; k < 3; k++)
				{
					if (!run[k])
						continue;
					const int c = order[k];
					const uint32_t nf = m->frame_n[c];
					launch_map_nn(st, m->frame[c], nf, m->rec[c], m->n[c], P->tree_mode == 2, P->tree_box, m->best + first[k]);
					launch_map_keep(st, m->frame[c], nf, m->best + first[k], P->dynamic_removal_center_radius, P->dynamic_dist_thre_min, dmax, P->near_dist_thre,
									m->keep + first[k]);
					const int rc = reserve(ctx, &m->frame_alt[c], &m->cap_frame_alt[c], nf, 0);
					if (rc != MULLS_OK)
						return rc;
					a.cloud[k].in = m->frame[c];
					a.cloud[k].out = m->frame_alt[c];
					a.cloud[k].mask = m->keep + first[k];
					a.cloud[k].n = nf;
				}
				a.out_n = m->counts;
				a.mode = 0;
				if (compact(ctx, m, a) != MULLS_OK) // the other slots are empty clouds
					return MULLS_E_HIP;
				uint32_t cnt[6];
				HIPCHK(ctx, hipMemcpyAsync(cnt, m->counts, sizeof(cnt), hipMemcpyDeviceToHost, st));
				HIPCHK(ctx, hipStreamSynchronize(st));
				for (int k = 0; k < 3; k++)
					if (run[k])
					{
						const int c = order[k];
						std::swap(m->frame[c], m->frame_alt[c]);
						std::swap(m->cap_frame[c], m->cap_frame_alt[c]);
						m->frame_n[c] = cnt[k];
					}
			}
		}
		for (int c = 0; c < MULLS_NC; c++)
			rep->frame_n[c] = m->frame_n[c];

		// 4. append_feature(last_target, true, used) (:54): the vertex cloud always
		{
			SegCopier app(ctx);
			for (int c = 0; c < MULLS_NC; c++)
				if ((c == MULLS_VERTEX || P->used_feature_type[c] == '1') && m->frame_n[c])
				{
					const int rc = reserve(ctx, &m->rec[c], &m->cap[c], (size_t)m->n[c] + m->frame_n[c], m->n[c]);
					if (rc != MULLS_OK)
						return rc;
					app.add_dev(m->rec[c] + (size_t)m->n[c] * 3, m->frame[c], (size_t)m->frame_n[c] * REC);
					m->n[c] += m->frame_n[c];
				}
			if (app.flush(st) != MULLS_OK)
				return MULLS_E_HIP;
		}
		// 5. the map moves to the frame's coordinates (:57-59)
		launch_transform_clouds(st, m->rec, m->n, MULLS_NC, poses.map_to_frame);
		std::memcpy(m->pose, frame_pose_lo, sizeof(m->pose));
		// 6. dist_filter(cloud, local_map_radius) on all six (:62-67)
		MapCompactArgs a;
		std::memset(&a, 0, sizeof(a));
		for (int c = 0; c < MULLS_NC; c++)
		{
			const int rc = reserve(ctx, &m->alt[c], &m->cap_alt[c], m->n[c], 0);
			if (rc != MULLS_OK)
				return rc;
			a.cloud[c].in = m->rec[c];
			a.cloud[c].out = m->alt[c];
			a.cloud[c].n = m->n[c];
		}
		a.out_n = m->counts;
		a.mode = 1;
		a.radius = (double)P->local_map_radius;
		if (compact(ctx, m, a) != MULLS_OK)
			return MULLS_E_HIP;
		uint32_t cnt[6];
		HIPCHK(ctx, hipMemcpyAsync(cnt, m->counts, sizeof(cnt), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		for (int c = 0; c < MULLS_NC; c++)
		{
			std::swap(m->rec[c], m->alt[c]);
			std::swap(m->cap[c], m->cap_alt[c]);
			m->n[c] = cnt[c];
		}
		// 7. random_downsample_pcl to the per-class share of max_num_pts (:70-86), seeded selection sampling
		int kept[MULLS_NC];
		const size_t mask_total = thinning_plan(m->n, P, kept);
		const bool any_thin = mask_total != 0;
		if (any_thin)
		{
			std::vector<uint8_t> mask(mask_total);
			if (m->cap_dmask < mask_total) // (grow-only: no allocator call per frame)
			{
				HIPCHK(ctx, hipStreamSynchronize(st));
				if (m->dmask)
					(void)hipFree(m->dmask);
				m->dmask = nullptr, m->cap_dmask = 0;
				if (dmalloc(ctx, &m->dmask, mask_total * 2) != MULLS_OK)
					return MULLS_E_HIP;
				m->cap_dmask = mask_total * 2;
			}
			uint8_t *dmask = m->dmask;
			std::memset(&a, 0, sizeof(a));
			size_t off = 0;
			uint32_t newn[MULLS_NC];
			for (int c = 0; c < MULLS_NC; c++)
			{
				newn[c] = m->n[c];
				if ((long)m->n[c] <= (long)kept[c])
					continue; // slot stays an empty cloud: nothing to do
				newn[c] = thin_mask(mask.data() + off, m->n[c], kept[c], P->rng_seed, 20 + c);
				a.cloud[c].in = m->rec[c];
				a.cloud[c].out = m->alt[c]; // capacity >= the pre-filter size
				a.cloud[c].mask = dmask + off;
				a.cloud[c].n = m->n[c];
				off += m->n[c];
			}
			a.out_n = m->counts;
			a.mode = 0;
			hipError_t e = hipMemcpyAsync(dmask, mask.data(), mask_total, hipMemcpyHostToDevice, st);
			if (e == hipSuccess)
			{
				if (compact(ctx, m, a) != MULLS_OK)
					e = hipErrorOutOfMemory;
				else
					e = hipStreamSynchronize(st);
			}
			if (e != hipSuccess)
			{
				ctx->err = std::string("map thinning: ") + hipGetErrorString(e);
				return MULLS_E_HIP;
			}
			for (int c = 0; c < MULLS_NC; c++)
				if ((long)m->n[c] > (long)kept[c])
				{
					std::swap(m->rec[c], m->alt[c]);
					std::swap(m->cap[c], m->cap_alt[c]);
					m->n[c] = newn[c];
				}
		}
		// 8. bounds of the merged cloud, local and posed (:88-94)
		uint32_t keys[12];
		bound_keys_init(keys);
		HIPCHK(ctx, hipMemcpyAsync(m->keys, keys, sizeof(keys), hipMemcpyHostToDevice, st));
		MapBoxArgs b;
		std::memset(&b, 0, sizeof(b));
		for (int c = 0; c < MULLS_NC; c++)
		{
			b.recs[c] = m->rec[c];
			b.n[c] = m->n[c];
		}
		std::memcpy(b.pose, poses.frame_pose, sizeof(b.pose));
		b.keys = m->keys;
		launch_map_bbox(st, b);
		HIPCHK(ctx, hipMemcpyAsync(keys, m->keys, sizeof(keys), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		bound_keys_decode(keys, m, rep);
		// 9. recalculate_feature_on (:98-118): principal directions of the pillar and beam clouds from their own neighbourhoods
		//    (pca_radius 1.8, pca_max_k 20, pca_min_k 6, min_linearity 0.65), pillars kept above sin 0.80, beams below sin 0.25
		{
			const int *cls = refresh_classes();
			for (int k = 0; k < 2; k++)
			{
				const int c = cls[k];
				const uint32_t nc = m->n[c];
				if (!refresh_runs(m, P, k))
					continue;
				if (m->cap_best < nc)
				{
					if (m->best)
						(void)hipFree(m->best);
					if (m->keep)
						(void)hipFree(m->keep);
					m->best = nullptr, m->keep = nullptr;
					m->cap_best = 0;
					if (dmalloc(ctx, &m->best, (size_t)nc * 2) != MULLS_OK || dmalloc(ctx, &m->keep, (size_t)nc * 2) != MULLS_OK)
						return MULLS_E_HIP;
					m->cap_best = (size_t)nc * 2;
				}
				MapPcaArgs pa;
				refresh_args(k, m->rec[c], nc, m->keep, &pa);
				launch_map_pca(st, pa);
				const int rc = reserve(ctx, &m->alt[c], &m->cap_alt[c], nc, 0);
				if (rc != MULLS_OK)
					return rc;
				std::memset(&a, 0, sizeof(a));
				a.cloud[0].in = m->rec[c];
				a.cloud[0].out = m->alt[c];
				a.cloud[0].mask = m->keep;
				a.cloud[0].n = nc;
				a.out_n = m->counts;
				a.mode = 0;
				if (compact(ctx, m, a) != MULLS_OK)
					return MULLS_E_HIP;
				HIPCHK(ctx, hipMemcpyAsync(cnt, m->counts, sizeof(cnt), hipMemcpyDeviceToHost, st));
				HIPCHK(ctx, hipStreamSynchronize(st));
				std::swap(m->rec[c], m->alt[c]);
				std::swap(m->cap[c], m->cap_alt[c]);
				m->n[c] = cnt[0];
			}
		}
		report_sizes(m, rep);
		rep->ms_total = (float)(std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count() * 1e3);
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_map_cloud(mulls_ctx *ctx, const mulls_map *m, int cls, mulls_cloud *out)
	try
	{
		if (!ctx || !m || !out || cls < 0 || cls >= MULLS_NC)
			return MULLS_E_INVALID;
		out->pts = m->rec[cls];
		out->n = m->n[cls];
		out->stride = (uint32_t)REC;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_map_pose(mulls_ctx *ctx, const mulls_map *m, double pose_lo[16])
	try
	{
		if (!ctx || !m || !pose_lo)
			return MULLS_E_INVALID;
		std::memcpy(pose_lo, m->pose, sizeof(m->pose));
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	static int download(mulls_ctx *ctx, const float4 *src, uint32_t have, void *pts, uint32_t cap, uint32_t *n)
	{
		if (n)
			*n = have;
		const uint32_t k = std::min(have, cap);
		if (k && !pts)
			return MULLS_E_INVALID;
		if (k)
		{
			HIPCHK(ctx, hipSetDevice(ctx->device));
			HIPCHK(ctx, hipMemcpyAsync(pts, src, (size_t)k * REC, hipMemcpyDeviceToHost, ctx->stream));
			HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		}
		return MULLS_OK;
	}
	int mulls_map_download(mulls_ctx *ctx, const mulls_map *m, int cls, void *pts, uint32_t cap, uint32_t *n)
	try
	{
		if (!ctx || !m || cls < 0 || cls >= MULLS_NC)
			return MULLS_E_INVALID;
		return download(ctx, m->rec[cls], m->n[cls], pts, cap, n);
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}
	int mulls_map_frame_download(mulls_ctx *ctx, const mulls_map *m, int cls, void *pts, uint32_t cap, uint32_t *n)
	try
	{
		if (!ctx || !m || cls < 0 || cls >= MULLS_NC)
			return MULLS_E_INVALID;
		return download(ctx, m->frame[cls], m->frame_n[cls], pts, cap, n);
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}
}
