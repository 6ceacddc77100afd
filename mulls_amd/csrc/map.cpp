// map.cpp — device-resident local map (include/mulls_hip.h, "mulls_map_*"): the class clouds that stay in HBM between frames — creation, mulls_map_set,
// the device clouds and the downloads.  The update itself (mulls_map_update, mulls_map_update_batch): map_batch.cpp.
#include <hip/hip_runtime_api.h>

#include "batch.h"
#include "ctx.h"
#include "device_types.h"
#include "hostmath.h"
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
// capacity in records; the contents are not kept
int reserve(mulls_ctx *ctx, float4 **p, size_t *cap, size_t need)
{
	if (*p && *cap >= need)
		return MULLS_OK;
	const size_t want = std::max<size_t>(need + need / 2, 1024);
	float4 *q = nullptr;
	HIPCHK(ctx, hipMalloc((void **)&q, want * REC));
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
		const int rc = reserve(ctx, &dst[c], &cap[c], cl.n);
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
