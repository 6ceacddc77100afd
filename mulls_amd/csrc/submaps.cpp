// submaps.cpp — mulls_submaps_*: the submaps of mulls_slam's back end kept in one device arena (include/mulls_hip.h, "the submap archive").  A push copies six
// class clouds (host or device, or a local map's) behind the last submap in cloudblock_t::merge_feature_points' order and takes both bounds on the device
// (k_submaps.hip); mulls_submaps_set_poses is update_optimized_nodes for many submaps in one launch set; the overlap search is host arithmetic on the poses
// and those bounds (submaps_host.h).  As everywhere in this library there is no CPU fallback for the device work.
#include <hip/hip_runtime_api.h>

#include <cmath>

#include "ctx.h"
#include "submaps_host.h"
#include "submaps_launch.h"

struct mulls_submaps
{
	float4 *arena = nullptr;
	uint32_t cap_points = 0, cap_submaps = 0, used = 0;
	std::vector<mulls_submap_info> subs;
	std::vector<uint32_t> job_first; // [count + 1]
	uint32_t *d_sub_off = nullptr, *d_job_first = nullptr; // [cap_submaps + 1]
	double *d_poses = nullptr, *d_out = nullptr;		   // [12 cap_submaps]
	uint32_t *d_keys = nullptr;							   // [12 cap_submaps]
};

namespace
{
constexpr size_t REC = MULLS_POINT_BYTES;
constexpr uint32_t MAX_POINTS = 1u << 30, MAX_SUBMAPS = 1u << 16;
// where class c (enum mulls_class) lies in a submap: merge_feature_points(pc, false) appends ground, facade, pillar, beam, roof, vertex
const int MERGE_ORDER[MULLS_NCLASS] = {MULLS_GROUND, MULLS_FACADE, MULLS_PILLAR, MULLS_BEAM, MULLS_ROOF, MULLS_VERTEX};

bool owns(const mulls_ctx *ctx, const mulls_submaps *s) { return std::find(ctx->submap_stores.begin(), ctx->submap_stores.end(), s) != ctx->submap_stores.end(); }

bool on_device(mulls_ctx *ctx, const void *pts, size_t bytes)
{
	if (mulls_is_map_memory(ctx, pts, bytes))
		return true;
	hipPointerAttribute_t at;
	std::memset(&at, 0, sizeof(at));
	if (hipPointerGetAttributes(&at, pts) == hipSuccess)
		return at.type == hipMemoryTypeDevice;
	(void)hipGetLastError(); // (an ordinary host pointer: the query reports an error on some runtimes — cleared)
	return false;
}

void rows12_of(const double pose[16], double out[12])
{
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 4; c++)
			out[r * 4 + c] = pose[r + 4 * c];
}

// first record (relative to the submap) and size of view `which`
void slice_of(const mulls_submap_info &I, int which, uint64_t *first, uint32_t *n)
{
	uint64_t off = 0;
	if (which == MULLS_SUBMAP_MERGED || which == MULLS_SUBMAP_MERGED_NO_GROUND)
	{
		uint64_t total = 0;
		for (int c = 0; c < MULLS_NCLASS; c++)
			total += I.n[c];
		const uint32_t skip = which == MULLS_SUBMAP_MERGED_NO_GROUND ? I.n[MULLS_GROUND] : 0u;
		*first = skip, *n = (uint32_t)(total - skip);
		return;
	}
	for (int m = 0; m < MULLS_NCLASS; m++)
	{
		if (MERGE_ORDER[m] == which)
			break;
		off += I.n[MERGE_ORDER[m]];
	}
	*first = off, *n = I.n[which];
}

int check_store(mulls_ctx *ctx, const mulls_submaps *S, const char *who)
{
	if (!owns(ctx, S))
	{
		ctx->err = std::string(who) + ": the store does not belong to this context";
		return MULLS_E_INVALID;
	}
	return MULLS_OK;
}

int check_view(mulls_ctx *ctx, const mulls_submaps *S, uint32_t id, int which, const char *who)
{
	if (int rc = check_store(ctx, S, who))
		return rc;
	if (id >= S->subs.size() || which < 0 || which > MULLS_SUBMAP_MERGED_NO_GROUND)
	{
		ctx->err = std::string(who) + ": submap id or `which` out of range";
		return MULLS_E_INVALID;
	}
	return MULLS_OK;
}

struct Src
{
	const void *pts;
	uint32_t n, stride;
	bool dev;
};

// the submap behind the last one: records, tables, bounds; nothing of the store changes unless everything succeeded.  given_lb / given_b: bounds to carry
// on instead of taking them (a local map's last report)
int push_impl(mulls_ctx *ctx, mulls_submaps *S, Src src[MULLS_NCLASS], const double pose[16], int32_t id_in_strip, float vertex_nms_radius, const double *given_lb,
			  const double *given_b, mulls_submap_info *info, const char *who)
{
	std::vector<unsigned char> nms_out;
	if (vertex_nms_radius > 0.0f && src[MULLS_VERTEX].n)
	{
		// mulls_slam.cpp:462 through the library's own entry point on its default path: the kept records come back to the host and go up with the rest
		mulls_cloud vc{src[MULLS_VERTEX].pts, src[MULLS_VERTEX].n, src[MULLS_VERTEX].stride};
		mulls_nms_params np;
		mulls_nms_default_params(&np);
		np.non_max_radius = vertex_nms_radius;
		nms_out.resize((size_t)vc.n * REC);
		uint32_t kept = 0;
		if (int rc = mulls_non_max_suppress(ctx, &vc, &np, nms_out.data(), vc.n, &kept, nullptr, 0, nullptr, nullptr))
			return rc;
		src[MULLS_VERTEX] = Src{nms_out.data(), kept, (uint32_t)REC, false};
	}
	std::memset(info, 0, sizeof(*info));
	uint64_t total = 0;
	for (int c = 0; c < MULLS_NCLASS; c++)
	{
		info->n[c] = src[c].n;
		total += src[c].n;
	}
	info->id_in_strip = id_in_strip;
	info->offset = S->used;
	info->points_needed = (uint64_t)S->used + total;
	info->submaps_needed = (uint32_t)S->subs.size() + 1u;
	std::memcpy(info->pose_lo, pose, sizeof(info->pose_lo));
	for (int k = 0; k < 6; k++)
	{
		info->local_bound[k] = info->bound[k] = k < 3 ? 1.7976931348623157e308 : -1.7976931348623157e308;
	}
	if (info->points_needed > S->cap_points || info->submaps_needed > S->cap_submaps)
	{
		ctx->err = std::string(who) + ": the store is full";
		return MULLS_E_UNSUPPORTED;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st}; // (the host vectors below are read by queued copies)
	std::vector<unsigned char> pack[MULLS_NCLASS];
	uint64_t off = S->used;
	for (int m = 0; m < MULLS_NCLASS; m++)
	{
		const Src &s = src[MERGE_ORDER[m]];
		float4 *dst = S->arena + off * 3u;
		off += s.n;
		if (!s.n)
			continue;
		if (s.dev && s.stride == REC)
			HIPCHK(ctx, hipMemcpyAsync(dst, s.pts, (size_t)s.n * REC, hipMemcpyDeviceToDevice, st));
		else if (s.dev)
			launch_submap_gather(st, dst, s.pts, s.stride, s.n);
		else
		{
			const void *from = s.pts;
			if (s.stride != REC)
			{
				std::vector<unsigned char> &p = pack[m];
				p.resize((size_t)s.n * REC);
				for (uint32_t i = 0; i < s.n; i++)
					std::memcpy(p.data() + (size_t)i * REC, (const unsigned char *)s.pts + (size_t)i * s.stride, REC);
				from = p.data();
			}
			HIPCHK(ctx, hipMemcpyAsync(dst, from, (size_t)s.n * REC, hipMemcpyHostToDevice, st));
		}
	}
	const uint32_t id = (uint32_t)S->subs.size();
	const uint32_t n_jobs = (uint32_t)((total + MULLS_SUBMAP_CHUNK - 1u) / MULLS_SUBMAP_CHUNK);
	const uint32_t tab[2] = {(uint32_t)(S->used + total), S->job_first[id] + n_jobs};
	HIPCHK(ctx, hipMemcpyAsync(S->d_sub_off + id + 1u, &tab[0], sizeof(uint32_t), hipMemcpyHostToDevice, st));
	HIPCHK(ctx, hipMemcpyAsync(S->d_job_first + id + 1u, &tab[1], sizeof(uint32_t), hipMemcpyHostToDevice, st));
	double out[12];
	if (given_lb && given_b)
	{
		std::memcpy(info->local_bound, given_lb, sizeof(info->local_bound));
		std::memcpy(info->bound, given_b, sizeof(info->bound));
		HIPCHK(ctx, hipStreamSynchronize(st));
	}
	else
	{
		double rows[12];
		rows12_of(pose, rows);
		HIPCHK(ctx, hipMemcpyAsync(S->d_poses, rows, sizeof(rows), hipMemcpyHostToDevice, st));
		SubmapBoundsArgs a;
		a.recs = S->arena, a.sub_off = S->d_sub_off, a.job_first = S->d_job_first, a.poses = S->d_poses, a.keys = S->d_keys, a.out = S->d_out;
		a.first = id, a.n = 1, a.with_local = 1;
		launch_submap_bounds(st, a, n_jobs);
		HIPCHK(ctx, hipGetLastError());
		HIPCHK(ctx, hipMemcpyAsync(out, S->d_out, sizeof(out), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		std::memcpy(info->local_bound, out, sizeof(info->local_bound));
		std::memcpy(info->bound, out + 6, sizeof(info->bound));
	}
	S->used = tab[0];
	S->job_first.push_back(tab[1]);
	S->subs.push_back(*info);
	return MULLS_OK;
}

bool radius_ok(float r) { return std::isfinite(r) && !(r < 0.0f); }
} // namespace

bool mulls_submaps_memory(const mulls_ctx *ctx, const void *p, size_t bytes)
{
	const char *q = (const char *)p;
	for (const mulls_submaps *s : ctx->submap_stores)
	{
		const char *lo = (const char *)s->arena;
		if (lo && q >= lo && q + bytes <= lo + (size_t)s->cap_points * REC)
			return true;
	}
	return false;
}

void mulls_submaps_release(mulls_ctx *ctx)
{
	while (!ctx->submap_stores.empty())
		mulls_submaps_destroy(ctx, ctx->submap_stores.back());
}

extern "C"
{
	void mulls_overlap_default_params(mulls_overlap_params *p)
	{
		std::memset(p, 0, sizeof(*p));
		p->neighbor_search_dist = 50.0f;
		p->min_iou_thre = 0.25f;
		p->adjacent_id_thre = 3;
		p->search_2d = 1;
		p->max_neighbor = 10;
	}

	int mulls_submaps_create(mulls_ctx *ctx, uint32_t capacity_points, uint32_t capacity_submaps, mulls_submaps **out)
	try
	{
		if (!ctx || !out)
			return MULLS_E_INVALID;
		*out = nullptr;
		if (capacity_points > MAX_POINTS || capacity_submaps > MAX_SUBMAPS)
		{
			ctx->err = "mulls_submaps_create: more than 2^30 points or 2^16 submaps";
			return MULLS_E_UNSUPPORTED;
		}
		HIPCHK(ctx, hipSetDevice(ctx->device));
		mulls_submaps *S = new mulls_submaps();
		S->cap_points = capacity_points, S->cap_submaps = capacity_submaps;
		S->job_first.assign(1, 0u);
		const size_t per = (size_t)capacity_submaps * 12u;
		bool ok = hipMalloc((void **)&S->arena, std::max<size_t>((size_t)capacity_points * REC, 64)) == hipSuccess;
		ok = ok && dmalloc(ctx, &S->d_sub_off, (size_t)capacity_submaps + 1u) == MULLS_OK && dmalloc(ctx, &S->d_job_first, (size_t)capacity_submaps + 1u) == MULLS_OK;
		ok = ok && dmalloc(ctx, &S->d_poses, std::max<size_t>(per, 12)) == MULLS_OK && dmalloc(ctx, &S->d_out, std::max<size_t>(per, 12)) == MULLS_OK;
		ok = ok && dmalloc(ctx, &S->d_keys, std::max<size_t>(per, 12)) == MULLS_OK;
		ok = ok && hipMemsetAsync(S->d_sub_off, 0, sizeof(uint32_t), ctx->stream) == hipSuccess && hipMemsetAsync(S->d_job_first, 0, sizeof(uint32_t), ctx->stream) == hipSuccess;
		ctx->submap_stores.push_back(S);
		if (!ok)
		{
			(void)hipGetLastError();
			mulls_submaps_destroy(ctx, S);
			ctx->err = "mulls_submaps_create: a device allocation failed";
			return MULLS_E_HIP;
		}
		*out = S;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	void mulls_submaps_destroy(mulls_ctx *ctx, mulls_submaps *S)
	{
		if (!S)
			return;
		if (ctx)
		{
			if (!owns(ctx, S))
				return; // (another context's store, or one destroyed already: not this call's to free)
			(void)hipSetDevice(ctx->device);
			(void)hipStreamSynchronize(ctx->stream);
			ctx->submap_stores.erase(std::remove(ctx->submap_stores.begin(), ctx->submap_stores.end(), S), ctx->submap_stores.end());
		}
		void *p[] = {S->arena, S->d_sub_off, S->d_job_first, S->d_poses, S->d_out, S->d_keys};
		for (void *q : p)
			if (q)
				(void)hipFree(q);
		delete S;
	}

	int mulls_submaps_push(mulls_ctx *ctx, mulls_submaps *S, const mulls_cloud clouds[MULLS_NCLASS], const double pose_lo[16], int32_t id_in_strip,
						   float vertex_nms_radius, mulls_submap_info *info)
	try
	{
		if (!ctx || !S || !clouds || !pose_lo || !info)
			return MULLS_E_INVALID;
		if (int rc = check_store(ctx, S, "mulls_submaps_push"))
			return rc;
		if (!radius_ok(vertex_nms_radius))
		{
			ctx->err = "mulls_submaps_push: vertex_nms_radius is negative or not finite";
			return MULLS_E_INVALID;
		}
		for (int c = 0; c < MULLS_NCLASS; c++)
			if (clouds[c].n && (!clouds[c].pts || clouds[c].stride < REC || clouds[c].stride % 4u || ((uintptr_t)clouds[c].pts & 3u)))
			{
				ctx->err = "mulls_submaps_push: a cloud with points and no address, or a stride under 48 or not a multiple of 4";
				return MULLS_E_INVALID;
			}
		HIPCHK(ctx, hipSetDevice(ctx->device));
		Src src[MULLS_NCLASS];
		for (int c = 0; c < MULLS_NCLASS; c++)
		{
			const mulls_cloud &cl = clouds[c];
			// (the last record ends 48 bytes in, not a whole stride)
			src[c] = Src{cl.pts, cl.n, cl.stride, cl.n ? on_device(ctx, cl.pts, (size_t)(cl.n - 1u) * cl.stride + REC) : false};
		}
		return push_impl(ctx, S, src, pose_lo, id_in_strip, vertex_nms_radius, nullptr, nullptr, info, "mulls_submaps_push");
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_submaps_push_map(mulls_ctx *ctx, mulls_submaps *S, const mulls_map *map, int32_t id_in_strip, float vertex_nms_radius, mulls_submap_info *info)
	try
	{
		if (!ctx || !S || !map || !info)
			return MULLS_E_INVALID;
		if (int rc = check_store(ctx, S, "mulls_submaps_push_map"))
			return rc;
		MapSnapshot snap;
		if (!mulls_map_snapshot(ctx, map, &snap))
		{
			ctx->err = "mulls_submaps_push_map: the map does not belong to this context";
			return MULLS_E_INVALID;
		}
		if (!radius_ok(vertex_nms_radius))
		{
			ctx->err = "mulls_submaps_push_map: vertex_nms_radius is negative or not finite";
			return MULLS_E_INVALID;
		}
		Src src[MULLS_NCLASS];
		for (int c = 0; c < MULLS_NCLASS; c++)
			src[c] = Src{snap.rec[c], snap.n[c], (uint32_t)REC, true};
		// the report's bounds describe the clouds as they are only while the vertex cloud goes in as it is
		const bool carry = snap.has_bounds && !(vertex_nms_radius > 0.0f);
		return push_impl(ctx, S, src, snap.pose, id_in_strip, vertex_nms_radius, carry ? snap.local_bound : nullptr, carry ? snap.bound : nullptr, info,
						 "mulls_submaps_push_map");
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_submaps_count(mulls_ctx *ctx, const mulls_submaps *S, uint32_t *n_submaps, uint64_t *n_points)
	try
	{
		if (!ctx || !S)
			return MULLS_E_INVALID;
		if (int rc = check_store(ctx, S, "mulls_submaps_count"))
			return rc;
		if (n_submaps)
			*n_submaps = (uint32_t)S->subs.size();
		if (n_points)
			*n_points = S->used;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_submaps_info(mulls_ctx *ctx, const mulls_submaps *S, uint32_t id, mulls_submap_info *info)
	try
	{
		if (!ctx || !S || !info)
			return MULLS_E_INVALID;
		if (int rc = check_view(ctx, S, id, 0, "mulls_submaps_info"))
			return rc;
		*info = S->subs[id];
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_submaps_cloud(mulls_ctx *ctx, const mulls_submaps *S, uint32_t id, int which, mulls_cloud *out)
	try
	{
		if (!ctx || !S || !out)
			return MULLS_E_INVALID;
		if (int rc = check_view(ctx, S, id, which, "mulls_submaps_cloud"))
			return rc;
		uint64_t first;
		uint32_t n;
		slice_of(S->subs[id], which, &first, &n);
		out->pts = S->arena + (S->subs[id].offset + first) * 3u;
		out->n = n;
		out->stride = (uint32_t)REC;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_submaps_download(mulls_ctx *ctx, const mulls_submaps *S, uint32_t id, int which, void *pts, uint32_t cap, uint32_t *n_out)
	try
	{
		if (!ctx || !S)
			return MULLS_E_INVALID;
		if (int rc = check_view(ctx, S, id, which, "mulls_submaps_download"))
			return rc;
		uint64_t first;
		uint32_t n;
		slice_of(S->subs[id], which, &first, &n);
		if (n_out)
			*n_out = n;
		const uint32_t k = std::min(n, cap);
		if (k && !pts)
			return MULLS_E_INVALID;
		if (k)
		{
			HIPCHK(ctx, hipSetDevice(ctx->device));
			HIPCHK(ctx, hipMemcpyAsync(pts, S->arena + (S->subs[id].offset + first) * 3u, (size_t)k * REC, hipMemcpyDeviceToHost, ctx->stream));
			HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		}
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_submaps_clear(mulls_ctx *ctx, mulls_submaps *S)
	try
	{
		if (!ctx || !S)
			return MULLS_E_INVALID;
		if (int rc = check_store(ctx, S, "mulls_submaps_clear"))
			return rc;
		HIPCHK(ctx, hipSetDevice(ctx->device));
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		S->used = 0;
		S->subs.clear();
		S->job_first.assign(1, 0u);
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_submaps_set_poses(mulls_ctx *ctx, mulls_submaps *S, uint32_t first, uint32_t n, const double *poses, int update_bbx)
	try
	{
		if (!ctx || !S || (n && !poses))
			return MULLS_E_INVALID;
		if (int rc = check_store(ctx, S, "mulls_submaps_set_poses"))
			return rc;
		if ((uint64_t)first + n > S->subs.size())
		{
			ctx->err = "mulls_submaps_set_poses: first + n beyond the submaps";
			return MULLS_E_INVALID;
		}
		if (!n)
			return MULLS_OK;
		std::vector<double> out;
		if (update_bbx)
		{
			// one upload, one launch set, one download; the store's records change only once all of it has succeeded
			std::vector<double> rows((size_t)n * 12u);
			for (uint32_t k = 0; k < n; k++)
				rows12_of(poses + (size_t)k * 16u, rows.data() + (size_t)k * 12u);
			out.resize((size_t)n * 6u);
			HIPCHK(ctx, hipSetDevice(ctx->device));
			hipStream_t st = ctx->stream;
			mulls::StreamDrain drain{st};
			HIPCHK(ctx, hipMemcpyAsync(S->d_poses, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st));
			SubmapBoundsArgs a;
			a.recs = S->arena, a.sub_off = S->d_sub_off, a.job_first = S->d_job_first, a.poses = S->d_poses, a.keys = S->d_keys, a.out = S->d_out;
			a.first = first, a.n = n, a.with_local = 0;
			launch_submap_bounds(st, a, S->job_first[first + n] - S->job_first[first]);
			HIPCHK(ctx, hipGetLastError());
			HIPCHK(ctx, hipMemcpyAsync(out.data(), S->d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
			HIPCHK(ctx, hipStreamSynchronize(st));
		}
		for (uint32_t k = 0; k < n; k++)
		{
			mulls_submap_info &I = S->subs[first + k];
			std::memcpy(I.pose_lo, poses + (size_t)k * 16u, sizeof(I.pose_lo));
			if (update_bbx)
				std::memcpy(I.bound, out.data() + (size_t)k * 6u, sizeof(I.bound));
		}
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_submaps_find_overlap(mulls_ctx *ctx, const mulls_submaps *S, uint32_t query_id, const mulls_overlap_params *params, mulls_submap_edge *edges,
								   uint32_t cap, uint32_t *n_edges)
	try
	{
		if (!ctx || !S || !params || !n_edges || (cap && !edges))
			return MULLS_E_INVALID;
		if (int rc = check_view(ctx, S, query_id, 0, "mulls_submaps_find_overlap"))
			return rc;
		if (!std::isfinite(params->neighbor_search_dist) || !std::isfinite(params->min_iou_thre) || params->adjacent_id_thre < 0)
		{
			ctx->err = "mulls_submaps_find_overlap: a search radius or IoU threshold that is not finite, or a negative adjacent_id_thre";
			return MULLS_E_INVALID;
		}
		const std::vector<mulls_submap_edge> found = mulls::submaps::find_overlap(S->subs.data(), query_id, *params);
		*n_edges = (uint32_t)found.size();
		for (uint32_t k = 0; k < std::min<uint32_t>(cap, *n_edges); k++)
			edges[k] = found[k];
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}

	int mulls_submaps_pairs(mulls_ctx *ctx, const mulls_submaps *S, const mulls_submap_edge *edges, uint32_t n, mulls_pair *pairs)
	try
	{
		if (!ctx || !S || (n && (!edges || !pairs)))
			return MULLS_E_INVALID;
		if (int rc = check_store(ctx, S, "mulls_submaps_pairs"))
			return rc;
		for (uint32_t k = 0; k < n; k++)
			if (edges[k].tgt_id < 0 || edges[k].src_id < 0 || (size_t)edges[k].tgt_id >= S->subs.size() || (size_t)edges[k].src_id >= S->subs.size())
			{
				ctx->err = "mulls_submaps_pairs: an edge names a submap the store does not hold";
				return MULLS_E_INVALID;
			}
		for (uint32_t k = 0; k < n; k++)
		{
			mulls_pair &P = pairs[k];
			std::memset(&P, 0, sizeof(P));
			for (int c = 0; c < MULLS_NCLASS; c++)
			{
				(void)mulls_submaps_cloud(ctx, S, (uint32_t)edges[k].tgt_id, c, &P.tgt[c]);
				(void)mulls_submaps_cloud(ctx, S, (uint32_t)edges[k].src_id, c, &P.src[c]);
			}
			std::memcpy(P.tgt_bound, S->subs[(size_t)edges[k].tgt_id].local_bound, sizeof(P.tgt_bound));
			std::memcpy(P.init_guess, edges[k].Trans1_2, sizeof(P.init_guess));
		}
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
	}
}
