// map_batch.cpp — mulls_map_update and mulls_map_update_batch (include/mulls_hip.h): MapManager::update_local_map (src/map_manager.cpp:18-140) and map-based
// dynamic-object removal (:149-268) in nine steps, for a group of maps in lock step; mulls_map_update is a group of one.  Every device step is one table-driven
// launch (k_map_batch.hip; the compactions: launch_map_compact_batch) over a flat job list the host builds from the sizes it knows at every phase, every wait
// happens once per group, and the host arithmetic between the waits is map_internal.h's.  As everywhere in this library there is no CPU fallback: the only
// host-side arithmetic is the pose algebra, the kept-point counts and the seeded selection masks.
//
//   phase A  steps 1-2   the frames' clouds into the maps' frame buffers (host sources wait in the pinned staging, read by the copy launch), moved to the map frame
//   phase B  step 3      dynamic removal of the items whose gate opens: fill `best`, nearest tree point, verdict, ONE compaction           -> wait (counts)
//   phase C  steps 4-6   append, the maps to their frames' coordinates, dist_filter                                                       -> wait (counts)
//   phase D  step 7      the thinning masks of every map (thin_mask, on the host pool), one upload, ONE compaction                        (sizes known: no wait)
//   phase E  steps 8-9   bounds and the pillar / beam refresh (both classes, one launch), ONE compaction                                 -> wait (keys, counts)
//
// Each map keeps its own buffers; the batch owns a pinned staging buffer and its device twin (tables up, counts and keys down).  A buffer that has to grow is
// replaced at once and the old one freed behind the phase's wait (kernels already queued may still read it), so growth never costs a wait of its own.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdio>

#include "batch.h"
#include "map_internal.h"
#include "subbatch.h"

using namespace mulls_mapi;

struct mulls_mapb_scratch
{
	unsigned char *pin = nullptr, *pin_d = nullptr, *dev = nullptr; // the same offsets in both; pin is host-mapped (pin_d: its device address)
	size_t cap = 0, off = 0;
	std::vector<void *> trash_dev, trash_pin;
};

namespace
{
void drain_trash(mulls_mapb_scratch *S)
{
	for (void *p : S->trash_dev)
		(void)hipFree(p);
	for (void *p : S->trash_pin)
		(void)hipHostFree(p);
	S->trash_dev.clear(), S->trash_pin.clear();
}
} // namespace

void mulls_mapb_release(mulls_ctx *ctx)
{
	mulls_mapb_scratch *S = ctx->mapb;
	if (!S)
		return;
	drain_trash(S);
	if (S->dev)
		(void)hipFree(S->dev);
	if (S->pin)
		(void)hipHostFree(S->pin);
	delete S;
	ctx->mapb = nullptr;
}

namespace
{
#define MBCHK(call)                                                                      \
	do                                                                                   \
	{                                                                                    \
		hipError_t e_ = (call);                                                          \
		if (e_ != hipSuccess)                                                            \
		{                                                                                \
			ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                \
			return MULLS_E_HIP;                                                          \
		}                                                                                \
	} while (0)

struct Item
{
	uint32_t idx;
	mulls_map *m;
	const mulls_cloud *fd;
	const double *pose;
	const mulls_map_params *P;
	mulls_map_report *rep;
	UpdatePoses poses;
	RemovalPlan plan;
	int kept[MULLS_NC];
	size_t mask_total;
	uint32_t newn[MULLS_NC];
	bool refresh[2];
	uint32_t keep_first[2];
};

// where a phase's tables and results lie in the staging: take() while the sizes are counted, place() once, then at() / dev() for the addresses
struct Layout
{
	size_t total = 0, base = 0;
	size_t take(size_t bytes)
	{
		const size_t at = total;
		total += up256(bytes);
		return at;
	}
};

struct Group
{
	mulls_ctx *ctx;
	mulls_mapb_scratch *S;
	hipStream_t st;
	mulls_map_batch_stats *stats;
	std::vector<Item> &it;

	int place(Layout &L)
	{
		const size_t need = up256(L.total) + 256;
		if (S->off + need > S->cap)
		{
			const size_t want = std::max<size_t>(2 * need, (size_t)1 << 20);
			if (S->dev)
				S->trash_dev.push_back(S->dev);
			if (S->pin)
				S->trash_pin.push_back(S->pin);
			S->dev = S->pin = S->pin_d = nullptr, S->cap = 0, S->off = 0;
			MBCHK(hipMalloc((void **)&S->dev, want));
			MBCHK(hipHostMalloc((void **)&S->pin, want, hipHostMallocMapped));
			MBCHK(hipHostGetDevicePointer((void **)&S->pin_d, S->pin, 0));
			S->cap = want;
		}
		L.base = S->off;
		S->off += need;
		return MULLS_OK;
	}
	template <typename T>
	T *host(const Layout &L, size_t at) { return reinterpret_cast<T *>(S->pin + L.base + at); }
	template <typename T>
	T *dev(const Layout &L, size_t at) { return reinterpret_cast<T *>(S->dev + L.base + at); }
	template <typename T>
	void put(const Layout &L, size_t at, const std::vector<T> &v)
	{
		if (!v.empty())
			std::memcpy(S->pin + L.base + at, v.data(), v.size() * sizeof(T));
	}
	int upload(const Layout &L, size_t bytes) // the first `bytes` of the phase's region, in one copy
	{
		if (bytes)
			MBCHK(hipMemcpyAsync(S->dev + L.base, S->pin + L.base, bytes, hipMemcpyHostToDevice, st));
		return MULLS_OK;
	}
	int download(const Layout &L, size_t at, size_t bytes)
	{
		if (bytes)
			MBCHK(hipMemcpyAsync(S->pin + L.base + at, S->dev + L.base + at, bytes, hipMemcpyDeviceToHost, st));
		return MULLS_OK;
	}
	int wait()
	{
		MBCHK(hipStreamSynchronize(st));
		stats->n_syncs++;
		drain_trash(S);
		return MULLS_OK;
	}

	// capacity in records, grown by half as map.cpp's reserve() does.  The old buffer (returned through `old` when its contents are to be kept) is freed behind
	// the next wait.
	int reserve_rec(float4 **p, size_t *cap, size_t need, float4 **old = nullptr)
	{
		if (old)
			*old = nullptr;
		if (*p && *cap >= need)
			return MULLS_OK;
		const size_t want = std::max<size_t>(need + need / 2, 1024);
		float4 *q = nullptr;
		MBCHK(hipMalloc((void **)&q, want * REC));
		if (*p)
		{
			S->trash_dev.push_back(*p);
			if (old)
				*old = *p;
		}
		*p = q;
		*cap = want;
		return MULLS_OK;
	}
	int reserve_best(mulls_map *m, size_t total)
	{
		if (m->cap_best >= total)
			return MULLS_OK;
		if (m->best)
			S->trash_dev.push_back(m->best);
		if (m->keep)
			S->trash_dev.push_back(m->keep);
		m->best = nullptr, m->keep = nullptr, m->cap_best = 0;
		if (dmalloc(ctx, &m->best, total * 2) != MULLS_OK || dmalloc(ctx, &m->keep, total * 2) != MULLS_OK)
			return MULLS_E_HIP;
		m->cap_best = total * 2;
		return MULLS_OK;
	}
	int reserve_seg(mulls_map *m, const MapCompactArgs &a)
	{
		const size_t need = (size_t)map_compact_segments(a) + 8;
		if (m->cap_seg >= need)
			return MULLS_OK;
		if (m->seg)
			S->trash_dev.push_back(m->seg);
		m->seg = nullptr, m->cap_seg = 0;
		if (dmalloc(ctx, &m->seg, need * 2) != MULLS_OK)
			return MULLS_E_HIP;
		m->cap_seg = need * 2;
		return MULLS_OK;
	}
	static void add_copy(std::vector<MapbCopyEnt> &ce, std::vector<MapbJob> &cj, const void *dst, const void *src, size_t bytes)
	{
		const size_t piece = (size_t)0xffffc000u; // (a 32-bit size per entry: a range of 4 GiB or more goes in as several, each a multiple of the block)
		for (size_t off = 0; off < bytes; off += piece)
		{
			const size_t b = std::min(piece, bytes - off);
			ce.push_back({(unsigned long long)(uintptr_t)dst + off, (unsigned long long)(uintptr_t)src + off, (uint32_t)b, 0u});
			for (size_t k = 0; k < b; k += MAPB_COPY_BLOCK)
				cj.push_back({(uint32_t)ce.size() - 1u, (uint32_t)(k / MAPB_COPY_BLOCK), 0u, 0u});
		}
	}
	static void add_blocks(std::vector<MapbJob> &jobs, uint32_t ent, uint32_t n, uint32_t per)
	{
		for (uint32_t b = 0; b < (n + per - 1u) / per; b++)
			jobs.push_back({ent, b, 0u, 0u});
	}

	// ---- phase A: steps 1 and 2 -------------------------------------------------------------------------------------------------------------------------
	int phase_frames()
	{
		std::vector<MapbCopyEnt> ce;
		std::vector<MapbJob> cj, xj;
		std::vector<MapbXformEnt> xe;
		struct HostSrc
		{
			size_t ent, at;
			const mulls_cloud *cl;
		};
		std::vector<HostSrc> hs;
		size_t host_bytes = 0;
		for (Item &I : it)
		{
			mulls_map *m = I.m;
			std::memset(I.rep, 0, sizeof(*I.rep));
			m->has_bounds = false; // (until step 8 of this update)
			for (int c = 0; c < MULLS_NC; c++)
			{
				const mulls_cloud &cl = I.fd[c];
				const int rc = reserve_rec(&m->frame[c], &m->cap_frame[c], cl.n);
				if (rc != MULLS_OK)
					return rc;
				m->frame_n[c] = cl.n;
				if (!cl.n)
					continue;
				const size_t bytes = (size_t)cl.n * REC;
				if (cl.stride == REC && mulls_is_map_memory(ctx, cl.pts, bytes))
					add_copy(ce, cj, m->frame[c], cl.pts, bytes);
				else
				{
					hs.push_back({ce.size(), host_bytes, &cl});
					add_copy(ce, cj, m->frame[c], nullptr, bytes); // (src: once the staging is placed)
					host_bytes += up256(bytes);
				}
			}
			update_poses(m->pose, I.pose, &I.poses);
			for (int c = 0; c < 5; c++)
				if (m->frame_n[c])
				{
					MapbXformEnt e;
					e.recs = m->frame[c], e.n = m->frame_n[c], e.pad_ = 0;
					std::memcpy(e.T, I.poses.frame_to_map, sizeof(e.T));
					xe.push_back(e);
					add_blocks(xj, (uint32_t)xe.size() - 1u, e.n, 256u);
				}
		}
		Layout L;
		const size_t o_ce = L.take(ce.size() * sizeof(MapbCopyEnt)), o_cj = L.take(cj.size() * sizeof(MapbJob)), o_xe = L.take(xe.size() * sizeof(MapbXformEnt)),
					 o_xj = L.take(xj.size() * sizeof(MapbJob));
		const size_t tab_bytes = L.total;
		const size_t o_host = L.take(host_bytes);
		if (place(L) != MULLS_OK)
			return MULLS_E_HIP;
		for (const HostSrc &h : hs)
		{
			const mulls_cloud &cl = *h.cl;
			unsigned char *dst = host<unsigned char>(L, o_host + h.at);
			if (cl.stride == REC)
				std::memcpy(dst, cl.pts, (size_t)cl.n * REC);
			else
				for (uint32_t i = 0; i < cl.n; i++)
					std::memcpy(dst + (size_t)i * REC, (const unsigned char *)cl.pts + (size_t)i * cl.stride, REC);
			// (the entries of one cloud follow each other, one per piece)
			size_t e = h.ent, off = 0;
			const size_t bytes = (size_t)cl.n * REC;
			while (off < bytes)
			{
				ce[e].src = (unsigned long long)(uintptr_t)(S->pin_d + L.base + o_host + h.at) + off;
				off += ce[e].bytes;
				e++;
			}
		}
		put(L, o_ce, ce), put(L, o_cj, cj), put(L, o_xe, xe), put(L, o_xj, xj);
		if (upload(L, tab_bytes) != MULLS_OK)
			return MULLS_E_HIP;
		stats->n_kernel_launches += (uint32_t)launch_mapb_copy(st, dev<MapbCopyEnt>(L, o_ce), dev<MapbJob>(L, o_cj), (uint32_t)cj.size());
		stats->n_kernel_launches += (uint32_t)launch_mapb_transform(st, dev<MapbXformEnt>(L, o_xe), dev<MapbJob>(L, o_xj), (uint32_t)xj.size());
		MBCHK(hipGetLastError());
		return MULLS_OK;
	}

	// ---- phase B: step 3 --------------------------------------------------------------------------------------------------------------------------------
	int phase_removal()
	{
		std::vector<MapbRemEnt> re;
		std::vector<MapbJob> pj, nj; // per frame block; per (frame block, tree chunk)
		std::vector<MapCompactJob> cj;
		std::vector<Item *> who;
		const int *order = removal_order();
		for (Item &I : it)
		{
			mulls_map *m = I.m;
			const mulls_map_params *P = I.P;
			I.plan = removal_plan(m, P);
			if (!I.plan.ran)
				continue;
			I.rep->dynamic_removal_ran = 1;
			if (!I.plan.total)
				continue;
			if (reserve_best(m, I.plan.total) != MULLS_OK)
				return MULLS_E_HIP;
			const float dmax = removal_dmax(P);
			MapCompactJob job;
			std::memset(&job, 0, sizeof(job));
			for (int k = 0; k < 3; k++)
			{
				if (!I.plan.run[k])
					continue;
				const int c = order[k];
				const uint32_t nf = m->frame_n[c];
				const int rc = reserve_rec(&m->frame_alt[c], &m->cap_frame_alt[c], nf);
				if (rc != MULLS_OK)
					return rc;
				MapbRemEnt e;
				std::memset(&e, 0, sizeof(e));
				e.frame = m->frame[c], e.tree = m->rec[c], e.best = m->best + I.plan.first[k], e.keep = m->keep + I.plan.first[k];
				e.n_frame = nf, e.n_tree = m->n[c], e.use_box = P->tree_mode == 2;
				e.center_radius = P->dynamic_removal_center_radius, e.dmin = P->dynamic_dist_thre_min, e.dmax = dmax, e.near_ = P->near_dist_thre;
				std::memcpy(e.box, P->tree_box, sizeof(e.box));
				re.push_back(e);
				const uint32_t ent = (uint32_t)re.size() - 1u;
				add_blocks(pj, ent, nf, 256u);
				const uint32_t nchunk = (e.n_tree + MAP_NN_CHUNK - 1u) / MAP_NN_CHUNK;
				for (uint32_t b = 0; b < (nf + 255u) / 256u; b++)
					for (uint32_t t = 0; t < nchunk; t++)
						nj.push_back({ent, b, t, 0u});
				job.a.cloud[k].in = m->frame[c];
				job.a.cloud[k].out = m->frame_alt[c];
				job.a.cloud[k].mask = e.keep;
				job.a.cloud[k].n = nf;
			}
			job.a.mode = 0;
			if (reserve_seg(m, job.a) != MULLS_OK)
				return MULLS_E_HIP;
			job.seg = m->seg;
			cj.push_back(job);
			who.push_back(&I);
		}
		if (!who.empty())
		{
			Layout L;
			const size_t o_re = L.take(re.size() * sizeof(MapbRemEnt)), o_pj = L.take(pj.size() * sizeof(MapbJob)), o_nj = L.take(nj.size() * sizeof(MapbJob)),
						 o_cj = L.take(cj.size() * sizeof(MapCompactJob));
			const size_t tab_bytes = L.total;
			const size_t o_cnt = L.take(who.size() * 6 * sizeof(uint32_t));
			if (place(L) != MULLS_OK)
				return MULLS_E_HIP;
			for (size_t k = 0; k < cj.size(); k++)
				cj[k].a.out_n = dev<uint32_t>(L, o_cnt) + k * 6;
			put(L, o_re, re), put(L, o_pj, pj), put(L, o_nj, nj), put(L, o_cj, cj);
			if (upload(L, tab_bytes) != MULLS_OK)
				return MULLS_E_HIP;
			const MapbRemEnt *re_d = dev<MapbRemEnt>(L, o_re);
			stats->n_kernel_launches += (uint32_t)launch_mapb_fill_best(st, re_d, dev<MapbJob>(L, o_pj), (uint32_t)pj.size());
			stats->n_kernel_launches += (uint32_t)launch_mapb_nn(st, re_d, dev<MapbJob>(L, o_nj), (uint32_t)nj.size());
			stats->n_kernel_launches += (uint32_t)launch_mapb_keep(st, re_d, dev<MapbJob>(L, o_pj), (uint32_t)pj.size());
			stats->n_kernel_launches += (uint32_t)launch_map_compact_batch(st, dev<MapCompactJob>(L, o_cj), cj.data(), (uint32_t)cj.size());
			MBCHK(hipGetLastError());
			if (download(L, o_cnt, who.size() * 6 * sizeof(uint32_t)) != MULLS_OK || wait() != MULLS_OK)
				return MULLS_E_HIP;
			const uint32_t *cnt = host<uint32_t>(L, o_cnt);
			for (size_t w = 0; w < who.size(); w++)
			{
				mulls_map *m = who[w]->m;
				for (int k = 0; k < 3; k++)
					if (who[w]->plan.run[k])
					{
						const int c = order[k];
						std::swap(m->frame[c], m->frame_alt[c]);
						std::swap(m->cap_frame[c], m->cap_frame_alt[c]);
						m->frame_n[c] = cnt[w * 6 + k];
					}
			}
		}
		for (Item &I : it)
			for (int c = 0; c < MULLS_NC; c++)
				I.rep->frame_n[c] = I.m->frame_n[c];
		return MULLS_OK;
	}

	// ---- phase C: steps 4, 5 and 6 ----------------------------------------------------------------------------------------------------------------------
	int phase_merge()
	{
		std::vector<MapbCopyEnt> ce;
		std::vector<MapbJob> pj, xj;
		std::vector<MapbXformEnt> xe;
		std::vector<MapCompactJob> cj(it.size());
		std::memset(cj.data(), 0, cj.size() * sizeof(MapCompactJob));
		for (size_t w = 0; w < it.size(); w++)
		{
			Item &I = it[w];
			mulls_map *m = I.m;
			const mulls_map_params *P = I.P;
			// 4. append_feature(last_target, true, used) (:54): the vertex cloud always
			for (int c = 0; c < MULLS_NC; c++)
				if ((c == MULLS_VERTEX || P->used_feature_type[c] == '1') && m->frame_n[c])
				{
					float4 *old = nullptr;
					const int rc = reserve_rec(&m->rec[c], &m->cap[c], (size_t)m->n[c] + m->frame_n[c], &old);
					if (rc != MULLS_OK)
						return rc;
					if (old && m->n[c])
						add_copy(ce, pj, m->rec[c], old, (size_t)m->n[c] * REC);
					add_copy(ce, pj, m->rec[c] + (size_t)m->n[c] * 3, m->frame[c], (size_t)m->frame_n[c] * REC);
					m->n[c] += m->frame_n[c];
				}
			// 5. the map moves to the frame's coordinates (:57-59)
			for (int c = 0; c < MULLS_NC; c++)
				if (m->n[c])
				{
					MapbXformEnt e;
					e.recs = m->rec[c], e.n = m->n[c], e.pad_ = 0;
					std::memcpy(e.T, I.poses.map_to_frame, sizeof(e.T));
					xe.push_back(e);
					add_blocks(xj, (uint32_t)xe.size() - 1u, e.n, 256u);
				}
			std::memcpy(m->pose, I.pose, sizeof(m->pose));
			// 6. dist_filter(cloud, local_map_radius) on all six (:62-67)
			MapCompactJob &job = cj[w];
			for (int c = 0; c < MULLS_NC; c++)
			{
				const int rc = reserve_rec(&m->alt[c], &m->cap_alt[c], m->n[c]);
				if (rc != MULLS_OK)
					return rc;
				job.a.cloud[c].in = m->rec[c];
				job.a.cloud[c].out = m->alt[c];
				job.a.cloud[c].n = m->n[c];
			}
			job.a.mode = 1;
			job.a.radius = (double)P->local_map_radius;
			if (reserve_seg(m, job.a) != MULLS_OK)
				return MULLS_E_HIP;
			job.seg = m->seg;
		}
		Layout L;
		const size_t o_ce = L.take(ce.size() * sizeof(MapbCopyEnt)), o_pj = L.take(pj.size() * sizeof(MapbJob)), o_xe = L.take(xe.size() * sizeof(MapbXformEnt)),
					 o_xj = L.take(xj.size() * sizeof(MapbJob)), o_cj = L.take(cj.size() * sizeof(MapCompactJob));
		const size_t tab_bytes = L.total;
		const size_t o_cnt = L.take(it.size() * 6 * sizeof(uint32_t));
		if (place(L) != MULLS_OK)
			return MULLS_E_HIP;
		for (size_t w = 0; w < cj.size(); w++)
			cj[w].a.out_n = dev<uint32_t>(L, o_cnt) + w * 6;
		put(L, o_ce, ce), put(L, o_pj, pj), put(L, o_xe, xe), put(L, o_xj, xj), put(L, o_cj, cj);
		if (upload(L, tab_bytes) != MULLS_OK)
			return MULLS_E_HIP;
		stats->n_kernel_launches += (uint32_t)launch_mapb_copy(st, dev<MapbCopyEnt>(L, o_ce), dev<MapbJob>(L, o_pj), (uint32_t)pj.size());
		stats->n_kernel_launches += (uint32_t)launch_mapb_transform(st, dev<MapbXformEnt>(L, o_xe), dev<MapbJob>(L, o_xj), (uint32_t)xj.size());
		stats->n_kernel_launches += (uint32_t)launch_map_compact_batch(st, dev<MapCompactJob>(L, o_cj), cj.data(), (uint32_t)cj.size());
		MBCHK(hipGetLastError());
		if (download(L, o_cnt, it.size() * 6 * sizeof(uint32_t)) != MULLS_OK || wait() != MULLS_OK)
			return MULLS_E_HIP;
		const uint32_t *cnt = host<uint32_t>(L, o_cnt);
		for (size_t w = 0; w < it.size(); w++)
		{
			mulls_map *m = it[w].m;
			for (int c = 0; c < MULLS_NC; c++)
			{
				std::swap(m->rec[c], m->alt[c]);
				std::swap(m->cap[c], m->cap_alt[c]);
				m->n[c] = cnt[w * 6 + c];
			}
		}
		return MULLS_OK;
	}

	// ---- phase D: step 7 --------------------------------------------------------------------------------------------------------------------------------
	int phase_thin()
	{
		// 7. random_downsample_pcl to the per-class share of max_num_pts (:70-86), seeded selection sampling: every map's masks after the one read above
		std::vector<Item *> who;
		size_t mask_bytes = 0;
		for (Item &I : it)
		{
			I.mask_total = thinning_plan(I.m->n, I.P, I.kept);
			if (I.mask_total)
			{
				who.push_back(&I);
				mask_bytes += up256(I.mask_total);
			}
		}
		if (who.empty())
			return MULLS_OK;
		std::vector<MapCompactJob> cj(who.size());
		std::memset(cj.data(), 0, cj.size() * sizeof(MapCompactJob));
		Layout L;
		const size_t o_cj = L.take(cj.size() * sizeof(MapCompactJob)), o_mask = L.take(mask_bytes);
		const size_t tab_bytes = L.total;
		const size_t o_cnt = L.take(who.size() * 6 * sizeof(uint32_t)); // (the scan writes them; the host knows the sizes already)
		if (place(L) != MULLS_OK)
			return MULLS_E_HIP;
		struct Unit
		{
			Item *I;
			int c;
			uint8_t *mask;
		};
		std::vector<Unit> units;
		size_t at = 0;
		for (size_t w = 0; w < who.size(); w++)
		{
			Item &I = *who[w];
			mulls_map *m = I.m;
			MapCompactJob &job = cj[w];
			size_t off = 0;
			for (int c = 0; c < MULLS_NC; c++)
			{
				I.newn[c] = m->n[c];
				if ((long)m->n[c] <= (long)I.kept[c])
					continue; // slot stays an empty cloud: nothing to do
				units.push_back({&I, c, host<uint8_t>(L, o_mask + at + off)});
				job.a.cloud[c].in = m->rec[c];
				job.a.cloud[c].out = m->alt[c]; // capacity >= the pre-filter size
				job.a.cloud[c].mask = dev<uint8_t>(L, o_mask + at + off);
				job.a.cloud[c].n = m->n[c];
				off += m->n[c];
			}
			at += up256(I.mask_total);
			job.a.out_n = dev<uint32_t>(L, o_cnt) + w * 6;
			job.a.mode = 0;
			if (reserve_seg(m, job.a) != MULLS_OK)
				return MULLS_E_HIP;
			job.seg = m->seg;
		}
		const std::function<void(long)> one = [&](long u) {
			const Unit &U = units[(size_t)u];
			U.I->newn[U.c] = thin_mask(U.mask, U.I->m->n[U.c], U.I->kept[U.c], U.I->P->rng_seed, 20 + U.c);
		};
		shared_host_pool().parallel_for(0, (long)units.size(), 1, one);
		put(L, o_cj, cj);
		if (upload(L, tab_bytes) != MULLS_OK)
			return MULLS_E_HIP;
		stats->n_kernel_launches += (uint32_t)launch_map_compact_batch(st, dev<MapCompactJob>(L, o_cj), cj.data(), (uint32_t)cj.size());
		MBCHK(hipGetLastError());
		for (Item *I : who)
			for (int c = 0; c < MULLS_NC; c++)
				if ((long)I->m->n[c] > (long)I->kept[c])
				{
					std::swap(I->m->rec[c], I->m->alt[c]);
					std::swap(I->m->cap[c], I->m->cap_alt[c]);
					I->m->n[c] = I->newn[c];
				}
		return MULLS_OK;
	}

	// ---- phase E: steps 8 and 9 -------------------------------------------------------------------------------------------------------------------------
	int phase_bounds_refresh()
	{
		std::vector<MapbBoxEnt> be;
		std::vector<MapbJob> bj, qj;
		std::vector<MapPcaArgs> pe;
		std::vector<MapCompactJob> cj;
		std::vector<Item *> who; // the items of cj
		const int *cls = refresh_classes();
		for (size_t w = 0; w < it.size(); w++)
		{
			Item &I = it[w];
			mulls_map *m = I.m;
			// 8. bounds of the merged cloud, local and posed (:88-94)
			for (int c = 0; c < MULLS_NC; c++)
				if (m->n[c])
				{
					MapbBoxEnt e;
					e.recs = m->rec[c], e.keys = nullptr, e.n = m->n[c], e.pad_ = (uint32_t)w; // (keys: once the staging is placed)
					std::memcpy(e.pose, I.poses.frame_pose, sizeof(e.pose));
					be.push_back(e);
					add_blocks(bj, (uint32_t)be.size() - 1u, e.n, MAPB_BOX_TILE);
				}
			// 9. recalculate_feature_on (:98-118): principal directions of the pillar and beam clouds from their own neighbourhoods
			uint32_t total = 0;
			for (int k = 0; k < 2; k++)
			{
				I.refresh[k] = refresh_runs(m, I.P, k);
				I.keep_first[k] = total;
				if (I.refresh[k])
					total += (m->n[cls[k]] + 3u) & ~3u;
			}
			if (!total)
				continue;
			if (reserve_best(m, total) != MULLS_OK)
				return MULLS_E_HIP;
			MapCompactJob job;
			std::memset(&job, 0, sizeof(job));
			for (int k = 0; k < 2; k++)
			{
				if (!I.refresh[k])
					continue;
				const int c = cls[k];
				const uint32_t nc = m->n[c];
				MapPcaArgs pa;
				refresh_args(k, m->rec[c], nc, m->keep + I.keep_first[k], &pa);
				pe.push_back(pa);
				add_blocks(qj, (uint32_t)pe.size() - 1u, nc, 256u);
				const int rc = reserve_rec(&m->alt[c], &m->cap_alt[c], nc);
				if (rc != MULLS_OK)
					return rc;
				job.a.cloud[k].in = m->rec[c];
				job.a.cloud[k].out = m->alt[c];
				job.a.cloud[k].mask = pa.keep;
				job.a.cloud[k].n = nc;
			}
			job.a.mode = 0;
			if (reserve_seg(m, job.a) != MULLS_OK)
				return MULLS_E_HIP;
			job.seg = m->seg;
			cj.push_back(job);
			who.push_back(&I);
		}
		Layout L;
		const size_t o_keys = L.take(it.size() * 12 * sizeof(uint32_t)); // (first: they go up initialised and come down with the counts behind them)
		const size_t o_cnt = L.take(who.size() * 6 * sizeof(uint32_t));
		const size_t down_bytes = L.total;
		const size_t o_be = L.take(be.size() * sizeof(MapbBoxEnt)), o_bj = L.take(bj.size() * sizeof(MapbJob)), o_pe = L.take(pe.size() * sizeof(MapPcaArgs)),
					 o_qj = L.take(qj.size() * sizeof(MapbJob)), o_cj = L.take(cj.size() * sizeof(MapCompactJob));
		if (place(L) != MULLS_OK)
			return MULLS_E_HIP;
		for (size_t w = 0; w < it.size(); w++)
			bound_keys_init(host<uint32_t>(L, o_keys) + w * 12);
		std::memset(host<uint32_t>(L, o_cnt), 0, who.size() * 6 * sizeof(uint32_t));
		for (MapbBoxEnt &e : be)
		{
			e.keys = dev<uint32_t>(L, o_keys) + (size_t)e.pad_ * 12;
			e.pad_ = 0;
		}
		for (size_t k = 0; k < cj.size(); k++)
			cj[k].a.out_n = dev<uint32_t>(L, o_cnt) + k * 6;
		put(L, o_be, be), put(L, o_bj, bj), put(L, o_pe, pe), put(L, o_qj, qj), put(L, o_cj, cj);
		if (upload(L, L.total) != MULLS_OK)
			return MULLS_E_HIP;
		stats->n_kernel_launches += (uint32_t)launch_mapb_bbox(st, dev<MapbBoxEnt>(L, o_be), dev<MapbJob>(L, o_bj), (uint32_t)bj.size());
		stats->n_kernel_launches += (uint32_t)launch_mapb_pca(st, dev<MapPcaArgs>(L, o_pe), dev<MapbJob>(L, o_qj), (uint32_t)qj.size());
		stats->n_kernel_launches += (uint32_t)launch_map_compact_batch(st, dev<MapCompactJob>(L, o_cj), cj.data(), (uint32_t)cj.size());
		MBCHK(hipGetLastError());
		if (download(L, 0, down_bytes) != MULLS_OK || wait() != MULLS_OK)
			return MULLS_E_HIP;
		for (size_t w = 0; w < it.size(); w++)
			bound_keys_decode(host<uint32_t>(L, o_keys) + w * 12, it[w].m, it[w].rep);
		const uint32_t *cnt = host<uint32_t>(L, o_cnt);
		for (size_t k = 0; k < who.size(); k++)
		{
			mulls_map *m = who[k]->m;
			for (int q = 0; q < 2; q++)
				if (who[k]->refresh[q])
				{
					const int c = cls[q];
					std::swap(m->rec[c], m->alt[c]);
					std::swap(m->cap[c], m->cap_alt[c]);
					m->n[c] = cnt[k * 6 + q];
				}
		}
		for (Item &I : it)
			report_sizes(I.m, I.rep);
		return MULLS_OK;
	}

	int run()
	{
		S->off = 0; // (the stream is idle: every group ends on a wait)
		int rc = phase_frames();
		if (rc == MULLS_OK)
			rc = phase_removal();
		if (rc == MULLS_OK)
			rc = phase_merge();
		if (rc == MULLS_OK)
			rc = phase_thin();
		if (rc == MULLS_OK)
			rc = phase_bounds_refresh();
		if (rc != MULLS_OK)
		{
			(void)hipStreamSynchronize(st); // (the staging and the retired buffers go back to their owners idle)
			drain_trash(S);
		}
		return rc;
	}
};

// why an item is refused before its map is touched (NULL frame, short strings, a cloud with points but no pointer or a stride below a record)
int precheck(const mulls_map_update_item &I, const mulls_map_params *P, std::string *why)
{
	if (!I.frame_down)
	{
		*why = "frame_down is NULL";
		return MULLS_E_INVALID;
	}
	if (std::strlen(P->used_feature_type) < 6 || std::strlen(P->tree_used) < 6)
	{
		*why = "used_feature_type and tree_used need 6 characters";
		return MULLS_E_INVALID;
	}
	for (int c = 0; c < MULLS_NC; c++)
		if (I.frame_down[c].n && (!I.frame_down[c].pts || I.frame_down[c].stride < REC))
		{
			*why = "cloud with points but null pointer or stride < 48";
			return MULLS_E_INVALID;
		}
	return MULLS_OK;
}

// The items as lock-step groups of at most `max_lockstep` (0: 64).  An item precheck refuses gets its status and stays out of its group; results[i].status and
// errs[i] say how item i fared.  Returns MULLS_E_HIP only where nothing was written (the device could not be selected).
int run_items(mulls_ctx *ctx, const mulls_map_update_item *items, uint32_t n_items, const mulls_map_params *shared_params, uint32_t max_lockstep,
			  mulls_map_batch_result *results, mulls_map_batch_stats *stats, std::vector<std::string> &errs)
{
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (!ctx->mapb)
		ctx->mapb = new mulls_mapb_scratch();
	const uint32_t per_group = max_lockstep ? max_lockstep : 64u;
	errs.assign(n_items, std::string());
	const auto fail = [&](uint32_t i, int rc, const std::string &why) {
		results[i].status = rc;
		errs[i] = why;
	};
	std::vector<Item> group;
	for (uint32_t g0 = 0; g0 < n_items; g0 += per_group)
	{
		const uint32_t g1 = std::min<uint64_t>((uint64_t)g0 + per_group, n_items);
		group.clear();
		for (uint32_t i = g0; i < g1; i++)
		{
			std::memset(&results[i], 0, sizeof(results[i]));
			const mulls_map_params *P = items[i].params ? items[i].params : shared_params;
			std::string why;
			const int rc = precheck(items[i], P, &why);
			if (rc != MULLS_OK)
			{
				fail(i, rc, why);
				continue;
			}
			Item I;
			std::memset(&I, 0, sizeof(I));
			I.idx = i, I.m = items[i].map, I.fd = items[i].frame_down, I.pose = items[i].frame_pose_lo, I.P = P, I.rep = &results[i].report;
			group.push_back(I);
		}
		stats->n_groups++;
		if (group.empty())
			continue;
		const auto wall0 = std::chrono::steady_clock::now();
		Group G{ctx, ctx->mapb, ctx->stream, stats, group};
		const int rc = G.run();
		const float ms = (float)(std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count() * 1e3);
		const std::string why = rc == MULLS_OK ? std::string() : ctx->err;
		for (const Item &I : group)
		{
			results[I.idx].report.ms_total = ms; // (the group's wall time: the items ran together)
			if (rc != MULLS_OK)
				fail(I.idx, rc, why);
		}
		stats->n_lockstep += (uint32_t)group.size();
		if (rc == MULLS_E_HIP)
		{
			for (uint32_t i = g1; i < n_items; i++) // (the device is not asked again)
			{
				std::memset(&results[i], 0, sizeof(results[i]));
				fail(i, MULLS_E_HIP, "not run: an earlier group failed on the device");
			}
			break;
		}
	}
	return MULLS_OK;
}
} // namespace

// One map: a batch of one, without the batch's own refusals (a frame cloud may lie in device memory of this or another map, the map is taken as given).
// Refused for a bad cloud, the call has zeroed `rep` and left the map as it was.
extern "C" int mulls_map_update(mulls_ctx *ctx, mulls_map *m, const mulls_cloud frame_down[6], const double frame_pose_lo[16], const mulls_map_params *P,
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
	const auto wall0 = std::chrono::steady_clock::now();
	mulls_map_update_item item;
	item.map = m, item.frame_down = frame_down, item.params = P;
	std::memcpy(item.frame_pose_lo, frame_pose_lo, sizeof(item.frame_pose_lo));
	mulls_map_batch_result res;
	mulls_map_batch_stats stats;
	std::memset(&stats, 0, sizeof(stats));
	std::vector<std::string> errs;
	const int rc = run_items(ctx, &item, 1, nullptr, 1, &res, &stats, errs);
	if (rc != MULLS_OK)
		return rc;
	*rep = res.report;
	if (res.status != MULLS_OK)
	{
		ctx->err = errs[0];
		return res.status;
	}
	rep->ms_total = (float)(std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count() * 1e3);
	return MULLS_OK;
}
catch (...)
{
	return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
}

extern "C" int mulls_map_update_batch(mulls_ctx *ctx, const mulls_map_update_item *items, uint32_t n_items, const mulls_map_params *shared_params,
									  uint32_t max_lockstep, mulls_map_batch_result *results, mulls_map_batch_stats *stats)
try
{
	if (!ctx)
		return MULLS_E_INVALID;
	mulls_map_batch_stats local;
	std::memset(&local, 0, sizeof(local));
	if (n_items == 0)
	{
		if (stats)
			*stats = local;
		return MULLS_OK;
	}
	// ---- refused before anything is written ----
	if (!items || !results)
	{
		ctx->err = "mulls_map_update_batch: items and results must not be NULL";
		return MULLS_E_INVALID;
	}
	for (uint32_t i = 0; i < n_items; i++)
	{
		const mulls_map *m = items[i].map;
		if (!m || std::find(ctx->maps.begin(), ctx->maps.end(), m) == ctx->maps.end())
		{
			ctx->err = "mulls_map_update_batch: item " + std::to_string(i) + ": map is NULL or not this context's";
			return MULLS_E_INVALID;
		}
		for (uint32_t j = 0; j < i; j++)
			if (items[j].map == m)
			{
				ctx->err = "mulls_map_update_batch: items " + std::to_string(j) + " and " + std::to_string(i) + " name the same map";
				return MULLS_E_INVALID;
			}
		if (!items[i].params && !shared_params)
		{
			ctx->err = "mulls_map_update_batch: item " + std::to_string(i) + " has no params and shared_params is NULL";
			return MULLS_E_INVALID;
		}
	}
	for (uint32_t i = 0; i < n_items; i++)
	{
		if (!items[i].frame_down)
			continue;
		for (int c = 0; c < MULLS_NC; c++)
		{
			const mulls_cloud &cl = items[i].frame_down[c];
			if (!cl.n || !cl.pts)
				continue;
			const char *q = (const char *)cl.pts;
			for (uint32_t j = 0; j < n_items; j++)
				for (int d = 0; d < MULLS_NC; d++)
				{
					const char *lo = (const char *)items[j].map->rec[d];
					if (lo && q >= lo && q < lo + items[j].map->cap[d] * REC)
					{
						ctx->err = "mulls_map_update_batch: item " + std::to_string(i) + ": a frame cloud lies in the memory of a map this batch updates (item " +
								   std::to_string(j) + ")";
						return MULLS_E_INVALID;
					}
				}
		}
	}
	std::vector<std::string> errs;
	const int rc = run_items(ctx, items, n_items, shared_params, max_lockstep, results, &local, errs);
	if (rc != MULLS_OK)
		return rc;
	if (stats)
		*stats = local;
	for (uint32_t i = 0; i < n_items; i++) // the lowest-index item that is not MULLS_OK
		if (results[i].status != MULLS_OK)
		{
			ctx->err = "mulls_map_update_batch: item " + std::to_string(i) + ": " + errs[i];
			return results[i].status;
		}
	return MULLS_OK;
}
catch (...)
{
	return mulls::abi_caught(const_cast<mulls_ctx *>(ctx)); // nothing is thrown across the ABI
}
