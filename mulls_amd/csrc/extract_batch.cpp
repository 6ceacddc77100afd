// extract_batch.cpp — the host chain of the feature stage (include/mulls_hip.h): extract_semantic_pts' scanner / distance filter ->
// voxel_downsample -> fast_ground_filter -> classify_nground_pts for many scans per call, and every single call as a batch of one (mulls_extract_features,
// mulls_extract_features_resident, mulls_ground_filter, mulls_classify_nground: the whole chain or one stage of it).  A sub-batch's scans lie side by side in
// one arena (extract_batch.h: a ground region and a classify region per scan); every device step is ONE launch over a table with one entry per scan (the
// *_batch launchers of k_ground.hip, k_classify.hip, map_kernels.hip), every copy or fill per array is one range of a k_ex_segs launch, and every host wait
// happens once per sub-batch:
//   1 sizes after the pre-filter   2 GfOut   3 (thinning masks up)   4 promotion rounds   5 class counts, non-finite flag   6 keys down, orders up
//   7 suppression rounds           8 *_down sizes (and the clouds the host thins)          9 block placement
// What the host decides per scan — thin_mask, std::sort's visiting orders, the sector samplers — sees that scan's data only.  The two steps without a table
// form (vox_run, launch_ground_normals) run scan-locally in sub-batches of one scan.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mulls_hip.h"
#include "classify_launch.h"
#include "ctx.h"
#include "extract_batch.h"
#include "extract_internal.h"
#include "extract_launch.h"
#include "ground_launch.h"
#include "map_launch.h"
#include "nms_host.h"
#include "rounds.h"

using namespace mulls_ex;

namespace
{
const size_t REC = MULLS_POINT_BYTES;
typedef std::vector<unsigned char> Bytes;

struct ScanState
{
	uint32_t n_in = 0, n = 0; // points handed in; after the pre-filter
	int status = MULLS_OK;
	std::string err;
	bool live = false; // still part of the lock step
	GfArena a;
	unsigned char *gf = nullptr, *cl = nullptr, *cur = nullptr, *other = nullptr, *ug = nullptr; // the two regions; the scan ahead of the ground filter; the non-ground cloud
	GfOut go = {};
	uint32_t n_ug = 0, n_cl = 0; // non-ground points; those the classification works on
	bool classify = false;		 // n_cl > 0
	std::vector<uint8_t> in_mask;
	Layout L = {};
	uint32_t ncls[4] = {}, ndown[4] = {}, nvertex = 0;
	float4 *cls[4] = {};
	bool nms_c[4] = {};
	Bytes host[MULLS_CL_COUNT];
	bool on_host[MULLS_CL_COUNT] = {};
	std::vector<uint32_t> gd_idx;
	// the nine clouds of the classification in MULLS_CL_* order: where the kernels left them (host[k] instead where on_host[k]) and their sizes
	void clouds(const float4 *dev[MULLS_CL_COUNT], uint32_t cnt[MULLS_CL_COUNT]) const
	{
		for (int c = 0; c < 4; c++)
			dev[c] = cls[c], cnt[c] = ncls[c], dev[4 + c] = L.down[c], cnt[4 + c] = ndown[c];
		dev[MULLS_CL_VERTEX] = L.vertex, cnt[MULLS_CL_VERTEX] = nvertex;
	}
};

#define EXCHK(call)            \
	do                         \
	{                          \
		const int rc_ = (call); \
		if (rc_ != MULLS_OK)   \
			return rc_;        \
	} while (0)

// the tables and byte ranges of one sub-batch on their way to the device, and the statistics
struct Run
{
	mulls_ctx *ctx;
	hipStream_t st;
	mulls_extract_batch_stats *S;
	const char *who; // the entry point's name for its messages (the round loops of a single call are mulls_classify_nground's)
	unsigned char *tab_dev = nullptr; // device table area (inside the arena), mirrored by ctx->exb_tab_pin
	size_t tab_cap = 0, tab_off = 0;
	unsigned char *pin_dev = nullptr; // device address of ctx->exb_pin
	size_t pin_off = 0;
	std::vector<ExSeg> segs;
	uint32_t seg_max = 0;

	const char *msg(const char *what)
	{
		text = std::string(who) + ": " + what;
		return text.c_str();
	}
	std::string text;
	// a table to the device (one copy command); nullptr: failed
	template <typename T>
	const T *upload(const std::vector<T> &v)
	{
		const size_t bytes = v.size() * sizeof(T);
		tab_off = (tab_off + 63u) & ~(size_t)63u;
		if (tab_off + bytes > tab_cap)
		{
			ctx->err = msg("table area exhausted");
			return nullptr;
		}
		std::memcpy(ctx->exb_tab_pin + tab_off, v.data(), bytes);
		if (hipMemcpyAsync(tab_dev + tab_off, ctx->exb_tab_pin + tab_off, bytes, hipMemcpyHostToDevice, st) != hipSuccess)
		{
			ctx->err = msg("table upload failed");
			return nullptr;
		}
		const T *p = reinterpret_cast<const T *>(tab_dev + tab_off);
		tab_off += bytes;
		return p;
	}
	// the pinned scratch holds `bytes` from its start (called with the stream idle)
	int pin_reserve(size_t bytes)
	{
		EXCHK(grow_pinned(ctx, &ctx->exb_pin, &ctx->exb_pin_cap, bytes, hipHostMallocMapped));
		HIPCHK(ctx, hipHostGetDevicePointer((void **)&pin_dev, ctx->exb_pin, 0));
		return MULLS_OK;
	}
	// `bytes` of the pinned scratch (16-byte aligned): host address; dev(): the same bytes as the kernels address them
	unsigned char *pin_take(size_t bytes)
	{
		pin_off = (pin_off + 15u) & ~(size_t)15u;
		unsigned char *p = ctx->exb_pin + pin_off;
		pin_off += bytes;
		return p;
	}
	unsigned char *dev(const void *pinned) const { return pin_dev + (static_cast<const unsigned char *>(pinned) - ctx->exb_pin); }
	void seg(const void *dst, const void *src, size_t bytes)
	{
		bytes = (bytes + 3u) & ~(size_t)3u;
		if (!bytes)
			return;
		segs.push_back({(unsigned long long)(uintptr_t)dst, (unsigned long long)(uintptr_t)src, (uint32_t)bytes, 0u});
		seg_max = std::max(seg_max, (uint32_t)bytes);
	}
	int flush()
	{
		if (segs.empty())
			return MULLS_OK;
		const ExSeg *t = upload(segs);
		if (!t)
			return MULLS_E_HIP;
		S->n_kernel_launches += (uint32_t)launch_ex_segs(st, t, (uint32_t)segs.size(), seg_max);
		segs.clear(), seg_max = 0;
		return MULLS_OK;
	}
	int sync()
	{
		HIPCHK(ctx, hipStreamSynchronize(st));
		S->n_syncs++;
		return MULLS_OK;
	}
};

// which part of the chain a run of the core covers
enum Part
{
	EX_ALL,		// scans -> blocks (mulls_extract_features_batch, mulls_extract_features, mulls_extract_features_resident)
	EX_GROUND,	// scan -> ground / non-ground in the scan's region (mulls_ground_filter)
	EX_CLASSIFY // a cloud in the scan's region -> its class clouds, where the kernels leave them (mulls_classify_nground)
};
// where a one-scan run leaves the two clouds no block keeps (mulls_extract_features)
struct HostSinks
{
	void *raw, *down;
	uint32_t cap_raw, cap_down;
};

// voxel_downsample (vox_run: a host sort) and the ground normals of methods 1 and 2 (their own neighbour grid and error word) have no table form
bool scan_local_steps(const mulls_extract_params *X, const mulls_ground_params *P)
{
	return (X && !(X->vf_downsample_resolution < 0.001)) || (P && (P->estimate_ground_normal_method == 1 || P->estimate_ground_normal_method == 2));
}

// The lock step: the scans of `sc` whose `live` is set, one sub-batch after the other.  The checks of a scan's size and parameters are the entry point's.
struct Core
{
	Run R;
	Part part;
	const mulls_cloud *scans;
	const mulls_extract_params *X; // EX_ALL only
	const mulls_ground_params *P;
	const mulls_classify_params *C;
	mulls_block *const *blocks;
	mulls_extract_batch_result *results;
	std::vector<ScanState> &sc;
	const HostSinks *sinks; // one scan only, or null
	mulls_ctx *ctx;
	hipStream_t st;
	mulls_extract_batch_stats &S;
	bool scanner, dist, prefilter, voxels;
	bool alone; // every scan a sub-batch of its own: the two steps without a table form run scan-locally
	// of the sub-batch under way
	uint32_t first = 0, last = 0, m = 0;
	unsigned char *arena = nullptr;
	uint32_t *d_round = nullptr; // 64 counters of the round loops, shared by the scans
	size_t words_bytes = 0;		 // a row of 64 words per scan: what every wait reads

	Core(mulls_ctx *c, const char *who, mulls_extract_batch_stats *stats, Part part_, const mulls_cloud *scans_, const mulls_extract_params *X_, const mulls_ground_params *P_,
		 const mulls_classify_params *C_, mulls_block *const *blocks_, mulls_extract_batch_result *results_, std::vector<ScanState> &sc_, const HostSinks *sinks_ = nullptr)
		: R{c, c->stream, stats, who}, part(part_), scans(scans_), X(X_), P(P_), C(C_), blocks(blocks_), results(results_), sc(sc_), sinks(sinks_), ctx(c), st(c->stream), S(*stats)
	{
		scanner = X && X->apply_scanner_filter != 0, dist = X && X->apply_dist_filter != 0, prefilter = scanner || dist;
		voxels = X && !(X->vf_downsample_resolution < 0.001); // voxel_downsample hands the cloud on below 0.001 m (:90-97)
		alone = scan_local_steps(X, P);
	}
	uint32_t *words_of(uint32_t s) const { return reinterpret_cast<uint32_t *>(ctx->exb_pin) + (size_t)(s - first) * 64; }
	int method() const { return P ? P->estimate_ground_normal_method : 0; }

	int begin(uint32_t first_, uint32_t last_, uint64_t arena_bytes, uint64_t limit);
	int upload(const ScanRegion *reg);
	int prefilter_stage();
	int ground_stage();
	int classify_stage();
	int place();
	int run(uint32_t n_scans, uint64_t limit);
};

// ---- the arena and the tables -----------------------------------------------------------------------------------------------------------
int Core::begin(uint32_t first_, uint32_t last_, uint64_t arena_bytes, uint64_t limit)
{
	first = first_, last = last_, m = last - first;
	EXCHK(ex_arena_reserve(ctx, arena_bytes, limit));
	arena = static_cast<unsigned char *>(ctx->exb_buf);
	d_round = reinterpret_cast<uint32_t *>(arena);
	R.tab_dev = arena + MULLS_EXB_HEAD_BYTES, R.tab_cap = (size_t)MULLS_EXB_TABLE_BYTES * m, R.tab_off = 0;
	if (grow_pinned(ctx, &ctx->exb_tab_pin, &ctx->exb_tab_pin_cap, R.tab_cap, hipHostMallocDefault) != MULLS_OK)
		return MULLS_E_HIP;
	words_bytes = (size_t)m * 256;
	EXCHK(R.pin_reserve(words_bytes + 64));
	R.pin_off = words_bytes;
	if (method() == 3 && gf_rnd_table(ctx) != MULLS_OK)
		return MULLS_E_HIP;
	return MULLS_OK;
}

// ---- the scans go up (pageable ones of a MB and more through the context's pinned scratch; a caller's pinned buffer goes up as it is) ----------------
// A pageable scan of a few MB is pinned and unpinned by the runtime around its copy (0.15 ms in front of a 0.1 ms transfer on the frame path): the
// process's host pool moves it into the context's pinned scratch instead, and the transfer starts from there.
int Core::upload(const ScanRegion *reg)
{
	{
		std::vector<uint8_t> stage(m, 0), on_dev(m, 0);
		size_t pin_need = 0;
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live)
				continue;
			Z.gf = arena + reg[s].o_gf, Z.cl = arena + reg[s].o_cl;
			if (part == EX_CLASSIFY)
			{
				// the region holds the cloud and nothing else: it is the non-ground cloud of a scan whose ground stage has run
				Z.cur = Z.ug = Z.gf;
				Z.go.n_unground = Z.n_in;
			}
			else
			{
				// two scan-sized buffers (gf, alt): every stage ahead of the ground filter reads one and writes the other, and the last one writes gf
				Z.a = gf_layout(Z.n_in, prefilter, voxels, method());
				Z.cur = (prefilter != voxels) ? Z.gf + Z.a.o_alt : Z.gf, Z.other = (prefilter != voxels) ? Z.gf : Z.gf + Z.a.o_alt;
				Z.ug = Z.gf + Z.a.o_unground;
			}
			hipPointerAttribute_t at;
			const hipError_t qe = hipPointerGetAttributes(&at, scans[s].pts);
			const bool pageable = qe != hipSuccess || at.type == hipMemoryTypeUnregistered;
			if (qe != hipSuccess)
				(void)hipGetLastError(); // not an error of this call
			else
				on_dev[s - first] = at.type == hipMemoryTypeDevice;
			// (the stage-alone calls send their cloud as it is: staged, mulls_ground_filter measured 0.06 ms slower on a 121 k-return scan)
			if (part == EX_ALL && scans[s].stride == REC && pageable && (size_t)Z.n_in * REC >= ((size_t)1 << 20))
				stage[s - first] = 1, pin_need += ((size_t)Z.n_in * REC + 255u) & ~(size_t)255u;
		}
		if (pin_need && grow_pinned(ctx, &ctx->scan_pin, &ctx->scan_pin_cap, pin_need, hipHostMallocDefault) != MULLS_OK)
			return MULLS_E_HIP;
		size_t pin_at = 0;
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live)
				continue;
			const size_t rec_in = (size_t)Z.n_in * REC;
			const hipMemcpyKind kind = on_dev[s - first] ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
			if (scans[s].stride != REC)
			{
				HIPCHK(ctx, hipMemcpy2DAsync(Z.cur, REC, scans[s].pts, scans[s].stride, REC, Z.n_in, kind, st));
				continue;
			}
			const void *up = scans[s].pts;
			if (stage[s - first])
			{
				const size_t chunk = (size_t)256 << 10;
				const long nchunk = (long)((rec_in + chunk - 1) / chunk);
				unsigned char *dst = ctx->scan_pin + pin_at;
				const unsigned char *srcb = static_cast<const unsigned char *>(scans[s].pts);
				const std::function<void(long)> move = [&](long k) {
					const size_t o = (size_t)k * chunk;
					std::memcpy(dst + o, srcb + o, std::min(chunk, rec_in - o));
				};
				shared_host_pool().parallel_for(0, nchunk, 1, move);
				up = dst;
				pin_at += (rec_in + 255u) & ~(size_t)255u;
			}
			HIPCHK(ctx, hipMemcpyAsync(Z.cur, up, rec_in, kind, st));
		}
	}
	return MULLS_OK;
}

// ---- dist_filter, scanner_filter: one mask launch, one compaction, one look at the sizes (wait 1); voxel_downsample behind them, scan-locally --------
int Core::prefilter_stage()
{
	if (prefilter)
	{
		std::vector<RawMaskJob> mj(m);
		std::vector<MapCompactJob> cj(m);
		std::memset(cj.data(), 0, cj.size() * sizeof(MapCompactJob));
		uint32_t n_max = 0;
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			RawMaskJob &j = mj[s - first];
			j.pts = nullptr, j.mask = nullptr, j.n = 0, j.pad_ = 0;
			if (!Z.live)
				continue;
			uint32_t *counts = reinterpret_cast<uint32_t *>(Z.gf + Z.a.o_seg);
			j.pts = reinterpret_cast<const float4 *>(Z.cur), j.mask = Z.gf + Z.a.o_mask, j.n = Z.n_in;
			MapCompactJob &c = cj[s - first];
			c.a.cloud[0].in = reinterpret_cast<const float4 *>(Z.cur);
			c.a.cloud[0].out = reinterpret_cast<float4 *>(Z.other);
			c.a.cloud[0].mask = Z.gf + Z.a.o_mask;
			c.a.cloud[0].n = Z.n_in;
			c.a.out_n = counts;
			c.a.mode = 0;
			c.seg = counts + 8;
			n_max = std::max(n_max, Z.n_in);
			R.seg(R.dev(words_of(s)), counts, 32);
		}
		if (n_max)
		{
			RawMaskArgs ma;
			std::memset(&ma, 0, sizeof(ma));
			ma.dist_on = dist, ma.scanner_on = scanner;
			ma.dist_min_sq = X->min_dist_used * X->min_dist_used, ma.dist_max_sq = X->max_dist_used * X->max_dist_used;
			ma.self_radius = X->self_ring_radius, ma.ghost_radius = X->ghost_radius, ma.z_min_ghost = X->z_min, ma.z_min_global = X->z_min_min;
			const RawMaskJob *mj_d = R.upload(mj);
			const MapCompactJob *cj_d = R.upload(cj);
			if (!mj_d || !cj_d)
				return MULLS_E_HIP;
			launch_raw_mask_batch(st, mj_d, m, n_max, ma);
			S.n_kernel_launches += 1u + (uint32_t)launch_map_compact_batch(st, cj_d, cj.data(), m);
			EXCHK(R.flush());
			EXCHK(R.sync());
			for (uint32_t s = first; s < last; s++)
				if (sc[s].live)
				{
					sc[s].n = words_of(s)[0];
					std::swap(sc[s].cur, sc[s].other);
				}
		}
	}
	for (uint32_t s = first; s < last; s++)
	{
		ScanState &Z = sc[s];
		if (!Z.live)
			continue;
		results[s].n_out[MULLS_EX_RAW] = results[s].n_out[MULLS_EX_DOWN] = Z.n;
		if (Z.n == 0)
		{
			Z.live = false; // an empty block, MULLS_OK
			continue;
		}
		if (sinks && std::min(Z.n, sinks->cap_raw))
			HIPCHK(ctx, hipMemcpyAsync(sinks->raw, Z.cur, (size_t)std::min(Z.n, sinks->cap_raw) * REC, hipMemcpyDeviceToHost, st));
		if (voxels)
		{
			// (a sub-batch of one: vox_run waits for its bounding box and its keys, and sorts on the host)
			uint32_t nd = 0;
			const int rcv = vox_run(ctx, Z.gf, Z.a, reinterpret_cast<const float4 *>(Z.cur), Z.n, X->vf_downsample_resolution, reinterpret_cast<float4 *>(Z.other), &nd);
			if (rcv == MULLS_E_HIP)
				return rcv;
			if (rcv != MULLS_OK)
			{
				Z.err = ctx->err, Z.status = rcv, Z.live = false;
				continue;
			}
			std::swap(Z.cur, Z.other);
			results[s].n_out[MULLS_EX_DOWN] = Z.n = nd;
		}
		if (sinks && std::min(Z.n, sinks->cap_down))
			HIPCHK(ctx, hipMemcpyAsync(sinks->down, Z.cur, (size_t)std::min(Z.n, sinks->cap_down) * REC, hipMemcpyDeviceToHost, st));
	}
	return MULLS_OK;
}

// ---- fast_ground_filter: GfOut of every scan in one look (wait 2); the normals of methods 1 and 2 behind it, scan-locally ------------------------------------
int Core::ground_stage()
{
	{
		std::vector<GfScan> gt(m);
		std::memset(gt.data(), 0, gt.size() * sizeof(GfScan));
		bool any = false;
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live)
				continue;
			GfScan &g = gt[s - first];
			g.pts = reinterpret_cast<const float4 *>(Z.cur), g.n = Z.n;
			g.ids = reinterpret_cast<uint32_t *>(Z.gf + Z.a.o_ids), g.cellof = reinterpret_cast<uint16_t *>(Z.gf + Z.a.o_cell), g.code = Z.gf + Z.a.o_code;
			g.d3v = reinterpret_cast<float *>(Z.gf + Z.a.o_d3);
			g.ground = reinterpret_cast<float4 *>(Z.gf + Z.a.o_ground), g.unground = reinterpret_cast<float4 *>(Z.gf + Z.a.o_unground);
			g.aux = Z.gf + Z.a.o_aux;
			if (P->estimate_ground_normal_method == 3)
				g.R = gf_ransac_at(Z.gf, Z.a, Z.n, ctx->gf_rnd);
			R.seg(R.dev(words_of(s)), Z.gf + Z.a.o_aux, sizeof(GfOut));
			any = true;
		}
		if (any)
		{
			const GfScan *gt_d = R.upload(gt);
			if (!gt_d)
				return MULLS_E_HIP;
			S.n_kernel_launches += (uint32_t)launch_ground_filter_batch(st, gt_d, gt.data(), m, *P);
			EXCHK(R.flush());
			EXCHK(R.sync());
		}
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live)
				continue;
			std::memcpy(&Z.go, words_of(s), sizeof(GfOut));
			if (Z.go.error)
			{
				Z.err = "mulls_ground_filter: the grid has too many cells (more than 65536, or more than 64 M table entries: grid_resolution too fine for this scan's extent)";
				Z.status = MULLS_E_UNSUPPORTED, Z.live = false;
				continue;
			}
			if ((method() == 1 || method() == 2) && Z.go.n_ground)
			{
				// normals of cloud_ground from its own neighbourhoods (:1943-1954); the error word of the state reports a neighbourhood beyond the buffer
				uint32_t *err_word = reinterpret_cast<uint32_t *>(Z.gf + Z.a.o_aux) + 3;
				launch_ground_normals(st, reinterpret_cast<float4 *>(Z.gf + Z.a.o_ground), Z.go.n_ground, method() == 1 ? P->normal_estimation_radius : 0.0f, 2 * P->min_grid_pt_num,
									  Z.gf + Z.a.o_normals, err_word);
				uint32_t e = 0;
				HIPCHK(ctx, hipMemcpyAsync(&e, err_word, sizeof(e), hipMemcpyDeviceToHost, st));
				HIPCHK(ctx, hipStreamSynchronize(st));
				if (e)
				{
					Z.err = "mulls_ground_filter: more than 1024 ground points within normal_estimation_radius of one point";
					Z.status = MULLS_E_UNSUPPORTED, Z.live = false;
				}
			}
		}
	}
	return MULLS_OK;
}

// ---- classify_nground_pts ----------------------------------------------------------------------------------------------------------------------------------
int Core::classify_stage()
{
	// (a whole-chain call reaches the classification's own refusal here, behind the ground filter's)
	if (mulls_classify_check(ctx, C) != MULLS_OK)
	{
		for (uint32_t s = first; s < last; s++)
			if (sc[s].live)
				sc[s].err = ctx->err, sc[s].status = MULLS_E_INVALID, sc[s].live = false;
		return MULLS_OK;
	}
	ClParams Q;
	mulls_classify_kernel_params(C, &Q);
	const uint32_t K = Q.K;
	std::vector<ClScan> ct(m);
	std::memset(ct.data(), 0, ct.size() * sizeof(ClScan));
	uint32_t ncl_max = 0;
	{
		// random_downsample_pcl(cloud_in, unground_down_fixed_num) (:2088-2089): the masks of the scans that need it, all in one upload (wait 3 is none: the masks
		// wait in pinned memory until the next look)
		size_t mask_bytes = 64;
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live)
				continue;
			Z.n_ug = Z.go.n_unground;
			Z.n_cl = Z.n_ug;
			if (C->fixed_num_downsampling && (long)Z.n_ug > (long)C->unground_down_fixed_num)
			{
				Z.in_mask.resize(Z.n_ug);
				Z.n_cl = thin_mask(Z.in_mask.data(), Z.n_ug, C->unground_down_fixed_num, C->rng_seed, 30);
				mask_bytes += ((size_t)Z.n_ug + 31u) & ~(size_t)15u;
			}
			results[s].n_out[MULLS_EX_UNGROUND] = Z.n_cl;
			Z.classify = Z.n_cl > 0;
			ncl_max = std::max(ncl_max, Z.n_cl);
		}
		EXCHK(R.pin_reserve(words_bytes + mask_bytes + 64));
		R.pin_off = words_bytes;
		uint32_t *init_keys = reinterpret_cast<uint32_t *>(R.pin_take(32));
		static const uint32_t keys0[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u};
		std::memcpy(init_keys, keys0, sizeof(keys0));
		std::vector<MapCompactJob> tj(m);
		std::memset(tj.data(), 0, tj.size() * sizeof(MapCompactJob));
		bool any_thin = false;
		R.seg(d_round, nullptr, 256);
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live || !Z.classify)
				continue;
			Z.L = carve(Z.cl, Z.n_cl, K, Z.n_ug);
			const ClArrays &A = Z.L.A;
			ct[s - first].A = A, ct[s - first].n = Z.n_cl;
			const unsigned char *src = Z.ug;
			if (Z.in_mask.empty())
				R.seg(A.recs, src, (size_t)Z.n_cl * REC);
			else
			{
				unsigned char *pm = R.pin_take(Z.n_ug);
				std::memcpy(pm, Z.in_mask.data(), Z.n_ug);
				R.seg(A.mask, R.dev(pm), Z.n_ug);
				MapCompactJob &c = tj[s - first];
				c.a.cloud[0].in = reinterpret_cast<const float4 *>(src);
				c.a.cloud[0].out = A.recs;
				c.a.cloud[0].mask = A.mask;
				c.a.cloud[0].n = Z.n_ug;
				c.a.out_n = Z.L.counts;
				c.a.mode = 0;
				c.seg = Z.L.seg;
				any_thin = true;
			}
			// features of points that are not queried (pca_down_rate > 1) are pca_feature_t's zeros; the grid's start keys; its zeroed cell counters
			R.seg(A.closebits, nullptr, (size_t)(reinterpret_cast<unsigned char *>(A.f_nd + Z.n_cl) - reinterpret_cast<unsigned char *>(A.closebits)));
			R.seg(A.grid, R.dev(init_keys), 7 * sizeof(uint32_t));
			R.seg(A.cell_start, nullptr, (size_t)MULLS_CL_MAX_CELLS * sizeof(uint32_t));
			R.seg(A.cell_start + MULLS_CL_MAX_CELLS, nullptr, sizeof(uint32_t));
		}
		if (ncl_max)
		{
			EXCHK(R.flush());
			if (any_thin)
			{
				const MapCompactJob *tj_d = R.upload(tj);
				if (!tj_d)
					return MULLS_E_HIP;
				S.n_kernel_launches += (uint32_t)launch_map_compact_batch(st, tj_d, tj.data(), m);
			}
		}
	}
	if (ncl_max)
	{
		const ClScan *ct_d = R.upload(ct);
		if (!ct_d)
			return MULLS_E_HIP;
		S.n_kernel_launches += (uint32_t)launch_cl_grid_batch(st, ct_d, m, ncl_max, Q);
		S.n_kernel_launches += (uint32_t)launch_cl_pca_batch(st, ct_d, m, ncl_max, Q);
		S.n_kernel_launches += (uint32_t)launch_cl_label_batch(st, ct_d, m, ncl_max, Q);
		if (Q.vertex_method == 2)
		{
			// the promotion rounds in lock step (wait 4): every scan's undecided candidates add into the same counter, the loop ends when none is left anywhere
			const int rcr = run_rounds(
				ctx, st, d_round, 4u, &ctx->exb_rounds_hint[0],
				[&](uint32_t slot) {
					S.n_kernel_launches += (uint32_t)launch_cl_promote_round_batch(st, ct_d, m, ncl_max, Q, d_round + slot);
					S.promote_rounds++;
				},
				R.msg("the promotion loop did not settle"), &S.n_syncs);
			if (rcr != MULLS_OK)
				return rcr;
		}
		S.n_kernel_launches += (uint32_t)launch_cl_encode_batch(st, ct_d, m, ncl_max, Q);
		// stable compactions: the class clouds (first-pass members, then promoted ones), the key points, the *_down clouds of sharpen_with_nms = 0
		std::vector<MapCompactJob> ja(m), jb(m);
		std::memset(ja.data(), 0, ja.size() * sizeof(MapCompactJob));
		std::memset(jb.data(), 0, jb.size() * sizeof(MapCompactJob));
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live || !Z.classify)
				continue;
			const ClArrays &A = Z.L.A;
			const uint32_t n = Z.n_cl;
			MapCompactJob &a = ja[s - first], &b = jb[s - first];
			for (int k = 0; k < 6; k++)
			{
				a.a.cloud[k].in = A.recs;
				a.a.cloud[k].out = Z.L.cls_a[k];
				a.a.cloud[k].mask = A.mask + (size_t)k * n;
				a.a.cloud[k].n = n;
			}
			a.a.out_n = Z.L.counts, a.a.mode = 0, a.seg = Z.L.seg;
			b.a.cloud[0].in = A.vtx;
			b.a.cloud[0].out = Z.L.vertex;
			b.a.cloud[0].mask = A.mask + (size_t)6 * n;
			b.a.cloud[0].n = n;
			if (!Q.nms)
				for (int k = 0; k < 4; k++)
				{
					b.a.cloud[1 + k].in = A.recs;
					b.a.cloud[1 + k].out = Z.L.down[k];
					b.a.cloud[1 + k].mask = A.mask + (size_t)(7 + k) * n;
					b.a.cloud[1 + k].n = n;
				}
			b.a.out_n = Z.L.counts + 6, b.a.mode = 0, b.seg = Z.L.seg;
			R.seg(R.dev(words_of(s)), Z.L.counts, 48);
			R.seg(R.dev(words_of(s) + 16), A.grid, sizeof(ClGrid));
		}
		const MapCompactJob *ja_d = R.upload(ja), *jb_d = R.upload(jb);
		if (!ja_d || !jb_d)
			return MULLS_E_HIP;
		S.n_kernel_launches += (uint32_t)launch_map_compact_batch(st, ja_d, ja.data(), m);
		S.n_kernel_launches += (uint32_t)launch_map_compact_batch(st, jb_d, jb.data(), m);
		EXCHK(R.flush());
		EXCHK(R.sync()); // wait 5: class counts and the grid's non-finite flag
		const int fixed_num[4] = {C->pillar_down_fixed_num, C->beam_down_fixed_num, C->facade_down_fixed_num, C->roof_down_fixed_num};
		bool any_nms = false;
		size_t key_bytes = 64;
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live || !Z.classify)
				continue;
			const uint32_t *cnt = words_of(s);
			ClGrid grid;
			std::memcpy(&grid, words_of(s) + 16, sizeof(grid));
			if (grid.nonfinite)
			{
				Z.err = "mulls_classify_nground: the cloud has non-finite coordinates";
				Z.status = MULLS_E_INVALID, Z.live = false;
				continue;
			}
			// class clouds: pillar = [first pass | promoted], beam likewise (the promotion loop pushes after the first loop has finished)
			Z.ncls[0] = cnt[0] + cnt[1], Z.ncls[1] = cnt[2] + cnt[3], Z.ncls[2] = cnt[4], Z.ncls[3] = cnt[5];
			Z.cls[0] = Z.L.cls_a[0], Z.cls[1] = Z.L.cls_a[2], Z.cls[2] = Z.L.cls_a[4], Z.cls[3] = Z.L.cls_a[5];
			if (cnt[1])
				R.seg(Z.L.cls_a[0] + (size_t)cnt[0] * 3, Z.L.cls_a[1], (size_t)cnt[1] * REC);
			if (cnt[3])
				R.seg(Z.L.cls_a[2] + (size_t)cnt[2] * 3, Z.L.cls_a[3], (size_t)cnt[3] * REC);
			Z.ndown[0] = cnt[7], Z.ndown[1] = cnt[8], Z.ndown[2] = cnt[9], Z.ndown[3] = cnt[10];
			Z.nvertex = cnt[6];
			if (Q.nms)
				for (int c = 0; c < 4; c++)
				{
					Z.ndown[c] = 0;
					Z.nms_c[c] = fixed_num[c] > 0 && Z.ncls[c] >= 10;
					if (Z.nms_c[c])
						any_nms = true, key_bytes += (size_t)Z.ncls[c] * 8 + 32;
				}
		}
		EXCHK(R.flush()); // the promoted members behind the first pass's
		if (any_nms)
		{
			// non_max_suppress(cloud, cloud_down, 0.25 * radius) for the classes whose *_down_fixed_num is positive and that have 10 points: keys down,
			// visiting orders up (wait 6), through the pinned scratch; every (scan, class) sort on the host pool at once
			EXCHK(R.pin_reserve(words_bytes + key_bytes));
			R.pin_off = words_bytes;
			struct SortJob
			{
				float *keys;
				uint32_t *perm;
				uint32_t n;
			};
			std::vector<SortJob> sj;
			std::vector<ClRecJob> kj, gj;
			uint32_t nmax = 0;
			for (uint32_t s = first; s < last; s++)
			{
				ScanState &Z = sc[s];
				if (!Z.live || !Z.classify)
					continue;
				for (int c = 0; c < 4; c++)
				{
					if (!Z.nms_c[c])
						continue;
					const uint32_t n = Z.n_cl, nc = Z.ncls[c];
					float *hk = reinterpret_cast<float *>(R.pin_take((size_t)nc * 4));
					uint32_t *hp = reinterpret_cast<uint32_t *>(R.pin_take((size_t)nc * 4));
					sj.push_back({hk, hp, nc});
					ClRecJob j;
					std::memset(&j, 0, sizeof(j));
					j.in = Z.cls[c], j.keys = Z.L.keys + (size_t)c * n, j.n = nc;
					kj.push_back(j);
					j.perm = Z.L.perm + (size_t)c * n, j.out = Z.L.cls_sorted[c];
					gj.push_back(j);
					R.seg(R.dev(hk), Z.L.keys + (size_t)c * n, (size_t)nc * 4);
					nmax = std::max(nmax, nc);
				}
			}
			const ClRecJob *kj_d = R.upload(kj), *gj_d = R.upload(gj);
			if (!kj_d || !gj_d)
				return MULLS_E_HIP;
			S.n_kernel_launches += (uint32_t)launch_cl_keys_batch(st, kj_d, (uint32_t)kj.size(), nmax);
			EXCHK(R.flush());
			EXCHK(R.sync());
			// the comparator of cfilter.hpp:1255; the permutation std::sort leaves depends on keys and count only (nms_host.h)
			const std::function<void(long)> sort_class = [&](long k) { nms_visiting_order(sj[k].keys, sj[k].n, sj[k].perm); };
			shared_host_pool().parallel_for(0, (long)sj.size(), 1, sort_class);
			const float nms_radius = (float)(0.25 * C->neighbor_searching_radius);
			std::vector<ClNmsArgs> nt(m);
			std::memset(nt.data(), 0, nt.size() * sizeof(ClNmsArgs));
			std::vector<MapCompactJob> jd(m);
			std::memset(jd.data(), 0, jd.size() * sizeof(MapCompactJob));
			std::vector<uint32_t> with_nms;
			size_t k = 0;
			for (uint32_t s = first; s < last; s++)
			{
				ScanState &Z = sc[s];
				ClNmsArgs &na = nt[s - first];
				na.r2 = (float)((double)nms_radius * (double)nms_radius);
				// (a scan outside the suppression still owns a pool cursor for k_cl_nms_init to reset: its own arena's, or the head's spare word)
				na.pool_used = reinterpret_cast<unsigned long long *>(arena + 512);
				if (!Z.live || !Z.classify)
					continue;
				na.pool = Z.L.nms_pool, na.pool_used = Z.L.nms_pool_used, na.pool_cap = Z.L.nms_pool_cap;
				MapCompactJob &d = jd[s - first];
				d.a.out_n = Z.L.counts, d.a.mode = 0, d.seg = Z.L.seg;
				bool any = false;
				for (int c = 0; c < 4; c++)
				{
					if (!Z.nms_c[c])
						continue;
					any = true;
					R.seg(Z.L.perm + (size_t)c * Z.n_cl, R.dev(sj[k].perm), (size_t)Z.ncls[c] * 4);
					k++;
					Z.cls[c] = Z.L.cls_sorted[c]; // std::sort works on cloud_in itself: the class cloud stays in this order
					na.recs[c] = Z.L.cls_sorted[c];
					na.n[c] = Z.ncls[c];
					na.keep[c] = Z.L.keep[c];
					na.list[c] = Z.L.nms_list[c];
					na.cnt[c] = Z.L.nms_cnt[c];
					na.off[c] = Z.L.nms_off[c];
					na.wcur[c] = Z.L.nms_wcur[c];
					d.a.cloud[c].in = na.recs[c];
					d.a.cloud[c].out = Z.L.down[c];
					d.a.cloud[c].mask = na.keep[c];
					d.a.cloud[c].n = na.n[c];
				}
				if (any)
					with_nms.push_back(s);
			}
			const ClNmsArgs *nt_d = R.upload(nt);
			const MapCompactJob *jd_d = R.upload(jd);
			if (!nt_d || !jd_d)
				return MULLS_E_HIP;
			EXCHK(R.flush());
			S.n_kernel_launches += (uint32_t)launch_cl_gather_batch(st, gj_d, (uint32_t)gj.size(), nmax);
			S.n_kernel_launches += (uint32_t)launch_cl_nms_lists_batch(st, nt_d, m, nmax, d_round); // (zeroes the pool cursors and the round counters)
			const int rcn = run_rounds(
				ctx, st, d_round, 8u, &ctx->exb_rounds_hint[1],
				[&](uint32_t slot) {
					S.n_kernel_launches += (uint32_t)launch_cl_nms_round_batch(st, nt_d, m, nmax, d_round + slot);
					S.nms_rounds++;
				},
				R.msg("the suppression rounds did not settle"), &S.n_syncs); // wait 7
			if (rcn != MULLS_OK)
				return rcn;
			S.n_kernel_launches += (uint32_t)launch_map_compact_batch(st, jd_d, jd.data(), m);
			for (uint32_t s : with_nms)
				R.seg(R.dev(words_of(s)), sc[s].L.counts, 16);
			EXCHK(R.flush());
			EXCHK(R.sync()); // wait 8: the *_down sizes
			for (uint32_t s : with_nms)
				for (int c = 0; c < 4; c++)
					sc[s].ndown[c] = words_of(s)[c];
		}
		// the *_down clouds the fixed-number samplers thin come to the host in one launch, are thinned by the single path's samplers, and go back with the placement
		if (C->fixed_num_downsampling)
		{
			size_t bytes = 64;
			for (uint32_t s = first; s < last; s++)
				if (sc[s].live && sc[s].classify)
					for (int c = 0; c < 4; c++)
						bytes += (size_t)sc[s].ndown[c] * REC + 16;
			EXCHK(R.pin_reserve(words_bytes + bytes));
			R.pin_off = words_bytes;
			std::vector<unsigned char *> where((size_t)m * 4, nullptr);
			for (uint32_t s = first; s < last; s++)
			{
				ScanState &Z = sc[s];
				if (!Z.live || !Z.classify)
					continue;
				for (int c = 0; c < 4; c++)
					if (Z.ndown[c])
					{
						where[(size_t)(s - first) * 4 + c] = R.pin_take((size_t)Z.ndown[c] * REC);
						R.seg(R.dev(where[(size_t)(s - first) * 4 + c]), Z.L.down[c], (size_t)Z.ndown[c] * REC);
					}
			}
			if (!R.segs.empty())
			{
				EXCHK(R.flush());
				EXCHK(R.sync());
			}
			const std::function<void(long)> thin = [&](long i) {
				ScanState &Z = sc[first + (uint32_t)i];
				if (!Z.live || !Z.classify)
					return;
				for (int c = 0; c < 4; c++)
				{
					Bytes &h = Z.host[MULLS_CL_PILLAR_DOWN + c];
					h.clear();
					if (Z.ndown[c])
						h.assign(where[(size_t)i * 4 + c], where[(size_t)i * 4 + c] + (size_t)Z.ndown[c] * REC);
				}
				mulls_classify_thin_down(Z.host, C);
				for (int c = 0; c < 4; c++)
					Z.ndown[c] = (uint32_t)(Z.host[MULLS_CL_PILLAR_DOWN + c].size() / REC), Z.on_host[MULLS_CL_PILLAR_DOWN + c] = true;
			};
			shared_host_pool().parallel_for(0, (long)m, 1, thin);
		}
	}
	return MULLS_OK;
}

// ---- block placement (wait 9): every block sized first and grown at most once, then all clouds of all scans in one launch ---------------------------------
int Core::place()
{
	{
		size_t bytes = 64;
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live)
				continue;
			gf_ground_down_indices(P, Z.go.n_ground, Z.gd_idx);
			bytes += Z.gd_idx.size() * 4 + 16;
			for (int k = MULLS_CL_PILLAR_DOWN; k <= MULLS_CL_ROOF_DOWN; k++)
				bytes += Z.host[k].size() + 16;
		}
		EXCHK(R.pin_reserve(words_bytes + bytes));
		R.pin_off = words_bytes;
		std::vector<ClRecJob> gj;
		uint32_t gmax = 0;
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live)
				continue;
			mulls_block *blk = blocks[s];
			uint32_t *n_out = results[s].n_out;
			uint32_t cntk[MULLS_CL_COUNT];
			const float4 *dev[MULLS_CL_COUNT];
			Z.clouds(dev, cntk);
			uint32_t cnt[MULLS_EX_COUNT] = {};
			cnt[MULLS_EX_GROUND] = Z.go.n_ground, cnt[MULLS_EX_GROUND_DOWN] = (uint32_t)Z.gd_idx.size(), cnt[MULLS_EX_UNGROUND] = Z.n_cl;
			for (int k = 0; k < MULLS_CL_COUNT; k++)
				cnt[MULLS_EX_PILLAR + k] = Z.classify ? cntk[k] : 0u, n_out[MULLS_EX_PILLAR + k] = cnt[MULLS_EX_PILLAR + k];
			n_out[MULLS_EX_GROUND] = cnt[MULLS_EX_GROUND], n_out[MULLS_EX_GROUND_DOWN] = cnt[MULLS_EX_GROUND_DOWN];
			const BlockLayout bl = block_layout(cnt, Z.gd_idx.size());
			const size_t need = bl.need, *off = bl.off;
			if (blk->cap < need)
			{
				if (blk->buf)
					(void)hipFree(blk->buf);
				blk->buf = nullptr, blk->cap = 0;
				HIPCHK(ctx, hipMalloc((void **)&blk->buf, need + need / 4));
				blk->cap = need + need / 4;
			}
			R.seg(blk->buf + off[MULLS_EX_GROUND], Z.gf + Z.a.o_ground, (size_t)cnt[MULLS_EX_GROUND] * REC);
			if (!Z.gd_idx.empty())
			{
				uint32_t *d_idx = reinterpret_cast<uint32_t *>(blk->buf + bl.o_idx);
				unsigned char *hp = R.pin_take(Z.gd_idx.size() * 4);
				std::memcpy(hp, Z.gd_idx.data(), Z.gd_idx.size() * 4);
				R.seg(d_idx, R.dev(hp), Z.gd_idx.size() * 4);
				ClRecJob j;
				std::memset(&j, 0, sizeof(j));
				j.in = reinterpret_cast<const float4 *>(Z.gf + Z.a.o_ground), j.perm = d_idx, j.out = reinterpret_cast<float4 *>(blk->buf + off[MULLS_EX_GROUND_DOWN]);
				j.n = (uint32_t)Z.gd_idx.size();
				gj.push_back(j);
				gmax = std::max(gmax, j.n);
			}
			if (Z.classify)
			{
				R.seg(blk->buf + off[MULLS_EX_UNGROUND], Z.L.A.recs, (size_t)Z.n_cl * REC);
				for (int k = 0; k < MULLS_CL_COUNT; k++)
				{
					if (!cnt[MULLS_EX_PILLAR + k])
						continue;
					if (Z.on_host[k])
					{
						unsigned char *hp = R.pin_take(Z.host[k].size());
						std::memcpy(hp, Z.host[k].data(), Z.host[k].size());
						R.seg(blk->buf + off[MULLS_EX_PILLAR + k], R.dev(hp), Z.host[k].size());
					}
					else
						R.seg(blk->buf + off[MULLS_EX_PILLAR + k], dev[k], (size_t)cnt[MULLS_EX_PILLAR + k] * REC);
				}
			}
			for (int k = 0; k < MULLS_EX_COUNT; k++)
				blk->off[k] = off[k], blk->n[k] = cnt[k];
		}
		if (!R.segs.empty() || !gj.empty())
		{
			EXCHK(R.flush());
			if (!gj.empty())
			{
				const ClRecJob *gj_d = R.upload(gj);
				if (!gj_d)
					return MULLS_E_HIP;
				S.n_kernel_launches += (uint32_t)launch_cl_gather_batch(st, gj_d, (uint32_t)gj.size(), gmax);
			}
			EXCHK(R.sync()); // the arena and the pinned scratch the launch reads are the next sub-batch's
		}
	}
	return MULLS_OK;
}

// plan the sub-batches and run them
int Core::run(uint32_t n_scans, uint64_t limit)
{
	// (a neighbor_k the classification refuses sizes nothing: classify_stage turns those scans away)
	const uint32_t K = C && C->neighbor_k >= 1 && C->neighbor_k <= (int)MULLS_CL_MAX_K ? (uint32_t)C->neighbor_k : 1u;
	std::vector<ScanCost> cost(n_scans);
	std::vector<uint64_t> bytes(n_scans);
	for (uint32_t s = 0; s < n_scans; s++)
	{
		const uint32_t n = sc[s].live ? sc[s].n_in : 0u;
		if (part == EX_ALL)
			cost[s] = extract_batch_scan_cost(n, prefilter, method(), C->fixed_num_downsampling != 0, C->unground_down_fixed_num, K, voxels);
		else
		{
			// one stage's region: the ground arena alone, or the cloud and the classify arena of its work points
			cost[s].gf = !n ? 0u : part == EX_GROUND ? up256(gf_layout(n, false, false, method()).total) : up256((uint64_t)n * REC);
			cost[s].cl = !n || part == EX_GROUND ? 0u : up256(carve(nullptr, classify_work_points(n, C->fixed_num_downsampling != 0, C->unground_down_fixed_num), K, n).total);
			cost[s].total = cost[s].gf + cost[s].cl + MULLS_EXB_TABLE_BYTES;
		}
		bytes[s] = cost[s].total;
	}
	std::vector<uint32_t> cuts;
	extract_batch_cuts(bytes.data(), n_scans, limit, &cuts, alone ? 1u : MULLS_EXB_MAX_SCANS);
	std::vector<ScanRegion> reg(n_scans);
	for (size_t k = 0; k + 1 < cuts.size(); k++)
	{
		const uint64_t arena_bytes = extract_batch_offsets(cost.data(), cuts[k], cuts[k + 1], reg.data());
		S.n_subbatches++;
		EXCHK(begin(cuts[k], cuts[k + 1], arena_bytes, limit));
		EXCHK(upload(reg.data()));
		if (part == EX_ALL)
			EXCHK(prefilter_stage());
		if (part != EX_CLASSIFY)
			EXCHK(ground_stage());
		if (part != EX_GROUND)
			EXCHK(classify_stage());
		if (part == EX_ALL && blocks[first])
			EXCHK(place()); // (a one-scan run without a block: mulls_extract_features takes the clouds from where they are)
	}
	return MULLS_OK;
}

// a single call: one scan, one sub-batch, the scan's own status and message
int run_one(mulls_ctx *ctx, Part part, const char *who, const void *pts, uint32_t n, uint32_t stride, const mulls_extract_params *X, const mulls_ground_params *P,
			const mulls_classify_params *C, mulls_block *blk, const HostSinks *sinks, uint32_t *n_out, std::vector<ScanState> &sc)
{
	const mulls_cloud cloud = {pts, n, stride};
	mulls_extract_batch_result res;
	mulls_extract_batch_stats stats;
	std::memset(&res, 0, sizeof(res));
	std::memset(&stats, 0, sizeof(stats));
	sc.assign(1, ScanState());
	sc[0].n_in = sc[0].n = n, sc[0].live = true;
	Core K(ctx, who, &stats, part, &cloud, X, P, C, &blk, &res, sc, sinks);
	const int rc = K.run(1, MULLS_EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES);
	if (n_out)
		std::memcpy(n_out, res.n_out, sizeof(res.n_out));
	if (rc == MULLS_OK && sc[0].status != MULLS_OK)
		ctx->err = sc[0].err;
	return rc != MULLS_OK ? rc : sc[0].status;
}

// cloud_ground (n_ground records in the scan's region) and cloud_ground_down, taken from it on the host, cut to the capacities; waits for the stream
int ground_clouds_down(mulls_ctx *ctx, const mulls_ground_params *P, const ScanState &Z, void *ground, uint32_t cap_ground, void *ground_down, uint32_t cap_ground_down,
					   uint32_t *n_ground, uint32_t *n_ground_down)
{
	const uint32_t ng = Z.go.n_ground;
	std::vector<unsigned char> g((size_t)ng * REC);
	if (ng)
		HIPCHK(ctx, hipMemcpyAsync(g.data(), Z.gf + Z.a.o_ground, g.size(), hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	if (std::min(ng, cap_ground))
		std::memcpy(ground, g.data(), (size_t)std::min(ng, cap_ground) * REC);
	std::vector<uint32_t> idx;
	gf_ground_down_indices(P, ng, idx);
	for (size_t k = 0; k < idx.size() && k < cap_ground_down; k++)
		std::memcpy(static_cast<unsigned char *>(ground_down) + k * REC, g.data() + (size_t)idx[k] * REC, REC);
	*n_ground = ng, *n_ground_down = (uint32_t)idx.size();
	return MULLS_OK;
}
// the nine clouds of the classification from where the kernels (or the host's samplers) left them, cut to the capacities, and cloud_in as the stage leaves it
// (whole, or not at all: cloud_in null); queued on the stream
int class_clouds_down(mulls_ctx *ctx, const ScanState &Z, void *const out[MULLS_CL_COUNT], const uint32_t cap[MULLS_CL_COUNT], uint32_t n_out[MULLS_CL_COUNT], void *cloud_in)
{
	if (!Z.classify)
		return MULLS_OK;
	const float4 *dev[MULLS_CL_COUNT];
	uint32_t cnt[MULLS_CL_COUNT];
	Z.clouds(dev, cnt);
	for (int k = 0; k < MULLS_CL_COUNT; k++)
	{
		n_out[k] = cnt[k];
		const size_t want = std::min(cnt[k], cap[k]);
		if (!want)
			continue;
		if (Z.on_host[k])
			std::memcpy(out[k], Z.host[k].data(), want * REC);
		else
			HIPCHK(ctx, hipMemcpyAsync(out[k], dev[k], want * REC, hipMemcpyDeviceToHost, ctx->stream));
	}
	if (cloud_in)
		HIPCHK(ctx, hipMemcpyAsync(cloud_in, Z.L.A.recs, (size_t)Z.n_cl * REC, hipMemcpyDeviceToHost, ctx->stream));
	return MULLS_OK;
}
} // namespace

extern "C"
{
	// the feature stage's one device arena holds `need` bytes: grown by a quarter (frames whose sizes creep upward do not reallocate at every new
	// maximum), but not beyond the limit a batch was given unless one scan needs it
	MULLS_HIDDEN int ex_arena_reserve(mulls_ctx *ctx, uint64_t need, uint64_t limit)
	{
		if (ctx->exb_buf && ctx->exb_cap >= need)
			return MULLS_OK;
		if (ctx->exb_buf)
			(void)hipFree(ctx->exb_buf);
		ctx->exb_buf = nullptr, ctx->exb_cap = 0;
		const uint64_t want = std::max<uint64_t>(std::min(need + need / 4, std::max(need, limit)), 64);
		HIPCHK(ctx, hipMalloc(&ctx->exb_buf, want));
		ctx->exb_cap = want;
		return MULLS_OK;
	}

	int mulls_extract_features_batch(mulls_ctx *ctx, const mulls_cloud *scans, uint32_t n_scans, const mulls_extract_params *X, mulls_block *const *blocks,
									 uint64_t scratch_limit_bytes, mulls_extract_batch_result *results, mulls_extract_batch_stats *stats)
	try
	{
		if (!ctx || !X)
			return MULLS_E_INVALID;
		if (stats)
			std::memset(stats, 0, sizeof(*stats));
		if (n_scans == 0)
			return MULLS_OK;
		if (!scans || !blocks || !results)
			return MULLS_E_INVALID;
		for (uint32_t s = 0; s < n_scans; s++)
		{
			if (!blocks[s] || std::find(ctx->blocks.begin(), ctx->blocks.end(), blocks[s]) == ctx->blocks.end() || (scans[s].n && !scans[s].pts) ||
				scans[s].stride < MULLS_POINT_BYTES)
				return MULLS_E_INVALID;
			for (uint32_t t = 0; t < s; t++)
				if (blocks[t] == blocks[s])
					return MULLS_E_INVALID;
		}
		mulls_extract_batch_stats local, unseen;
		std::memset(&local, 0, sizeof(local));
		std::memset(&unseen, 0, sizeof(unseen));
		mulls_extract_batch_stats &S = stats ? *stats : local;
		std::memset(results, 0, sizeof(*results) * n_scans);
		const mulls_ground_params *P = &X->ground;
		HIPCHK(ctx, hipSetDevice(ctx->device));
		const mulls::StreamDrain drain{ctx->stream};
		std::vector<ScanState> sc(n_scans);
		// the statistics count the lock step: scans that run alone (path = 1) are counted as such and nothing else
		// (parameters every single call would refuse: each scan says how, as a scan that ran alone)
		const bool alone = scan_local_steps(X, P) || gf_check(ctx, P, 0) != MULLS_OK || mulls_classify_check(ctx, &X->classify) != MULLS_OK;
		Core K(ctx, "mulls_extract_features_batch", alone ? &unseen : &S, EX_ALL, scans, X, P, &X->classify, blocks, results, sc);
		K.alone = alone;
		for (uint32_t s = 0; s < n_scans; s++)
		{
			for (int k = 0; k < MULLS_EX_COUNT; k++)
				blocks[s]->n[k] = 0;
			sc[s].n_in = sc[s].n = scans[s].n;
			sc[s].status = gf_check(ctx, P, scans[s].n);
			if (sc[s].status != MULLS_OK)
				sc[s].err = ctx->err;
			sc[s].live = sc[s].status == MULLS_OK && scans[s].n > 0;
			results[s].path = alone ? 1u : 0u;
			(alone ? S.n_single_path : S.n_lockstep)++;
		}
		const int rc = K.run(n_scans, scratch_limit_bytes ? scratch_limit_bytes : MULLS_EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES);
		if (rc != MULLS_OK)
		{
			// the device or the runtime failed: no scan's result stands
			const std::string why = ctx->err;
			for (uint32_t s = 0; s < n_scans; s++)
			{
				results[s].status = rc;
				for (int k = 0; k < MULLS_EX_COUNT; k++)
					blocks[s]->n[k] = 0;
			}
			ctx->err = why;
			return rc;
		}
		for (uint32_t s = 0; s < n_scans; s++)
		{
			results[s].status = sc[s].status;
			if (sc[s].status != MULLS_OK)
				for (int k = 0; k < MULLS_EX_COUNT; k++)
					blocks[s]->n[k] = 0;
		}
		for (uint32_t s = 0; s < n_scans; s++)
			if (results[s].status != MULLS_OK)
			{
				ctx->err = "mulls_extract_features_batch: scan " + std::to_string(s) + ": " + sc[s].err;
				return (int)results[s].status;
			}
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	// ---- the single calls: a batch of one -------------------------------------------------------------------------------------------------
	// (the round loops' messages are mulls_classify_nground's in a single call, whichever entry point it is)
	int mulls_extract_features_resident(mulls_ctx *ctx, const void *scan, uint32_t n, uint32_t stride, const mulls_extract_params *X, mulls_block *block,
										uint32_t n_out[MULLS_EX_COUNT])
	try
	{
		if (!block || !ctx || !X || !n_out || (n && !scan) || stride < MULLS_POINT_BYTES)
			return MULLS_E_INVALID;
		for (int k = 0; k < MULLS_EX_COUNT; k++)
			block->n[k] = 0, n_out[k] = 0;
		const int chk = gf_check(ctx, &X->ground, n);
		if (chk != MULLS_OK || n == 0)
			return chk;
		HIPCHK(ctx, hipSetDevice(ctx->device));
		const mulls::StreamDrain drain{ctx->stream};
		std::vector<ScanState> sc;
		const int rc = run_one(ctx, EX_ALL, "mulls_classify_nground", scan, n, stride, X, &X->ground, &X->classify, block, nullptr, n_out, sc);
		if (rc != MULLS_OK)
			for (int k = 0; k < MULLS_EX_COUNT; k++)
				block->n[k] = 0;
		return rc;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	// the whole chain without a block: the clouds come down from where the stages leave them, cut to the capacities
	int mulls_extract_features(mulls_ctx *ctx, const void *scan, uint32_t n_in, uint32_t stride, const mulls_extract_params *X, void *const out[MULLS_EX_COUNT],
							   const uint32_t cap[MULLS_EX_COUNT], uint32_t n_out[MULLS_EX_COUNT])
	try
	{
		if (!ctx || !X || !out || !cap || !n_out || (n_in && !scan) || stride < MULLS_POINT_BYTES)
			return MULLS_E_INVALID;
		for (int k = 0; k < MULLS_EX_COUNT; k++)
		{
			n_out[k] = 0;
			if (cap[k] && !out[k])
				return MULLS_E_INVALID;
		}
		const int chk = gf_check(ctx, &X->ground, n_in);
		if (chk != MULLS_OK || n_in == 0)
			return chk;
		HIPCHK(ctx, hipSetDevice(ctx->device));
		const mulls::StreamDrain drain{ctx->stream}; // error returns leave copies into out[] queued
		const HostSinks sinks = {out[MULLS_EX_RAW], out[MULLS_EX_DOWN], cap[MULLS_EX_RAW], cap[MULLS_EX_DOWN]};
		std::vector<ScanState> sc;
		const int rc = run_one(ctx, EX_ALL, "mulls_classify_nground", scan, n_in, stride, X, &X->ground, &X->classify, nullptr, &sinks, n_out, sc);
		if (rc != MULLS_OK)
			return rc;
		const ScanState &Z = sc[0];
		// (cloud_in comes back only whole: a capacity below the non-ground cloud's size ahead of its thinning leaves the buffer alone)
		EXCHK(class_clouds_down(ctx, Z, out + MULLS_EX_PILLAR, cap + MULLS_EX_PILLAR, n_out + MULLS_EX_PILLAR, cap[MULLS_EX_UNGROUND] >= Z.go.n_unground ? out[MULLS_EX_UNGROUND] : nullptr));
		return ground_clouds_down(ctx, &X->ground, Z, out[MULLS_EX_GROUND], cap[MULLS_EX_GROUND], out[MULLS_EX_GROUND_DOWN], cap[MULLS_EX_GROUND_DOWN], &n_out[MULLS_EX_GROUND],
								  &n_out[MULLS_EX_GROUND_DOWN]);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	// the ground stage alone; cloud_ground_down is taken on the host from the downloaded cloud
	int mulls_ground_filter(mulls_ctx *ctx, const void *pts, uint32_t n, uint32_t stride, const mulls_ground_params *P, void *ground, uint32_t cap_ground,
							void *ground_down, uint32_t cap_ground_down, void *unground, uint32_t cap_unground, uint32_t n_out[3])
	try
	{
		if (!ctx || !P || !n_out || (n && !pts) || stride < MULLS_POINT_BYTES || (cap_ground && !ground) || (cap_ground_down && !ground_down) ||
			(cap_unground && !unground))
			return MULLS_E_INVALID;
		n_out[0] = n_out[1] = n_out[2] = 0;
		const int chk = gf_check(ctx, P, n);
		if (chk != MULLS_OK)
			return chk;
		if (n == 0)
			return MULLS_OK; // (the reference divides by a zero sample count here)
		HIPCHK(ctx, hipSetDevice(ctx->device));
		hipStream_t st = ctx->stream;
		const mulls::StreamDrain drain{st}; // error returns below leave copies into `unground` / `g` queued
		std::vector<ScanState> sc;
		const int rc = run_one(ctx, EX_GROUND, "mulls_ground_filter", pts, n, stride, nullptr, P, nullptr, nullptr, nullptr, nullptr, sc);
		if (rc != MULLS_OK)
			return rc;
		const ScanState &Z = sc[0];
		const uint32_t ku = std::min(Z.go.n_unground, cap_unground);
		if (ku)
			HIPCHK(ctx, hipMemcpyAsync(unground, Z.ug, (size_t)ku * REC, hipMemcpyDeviceToHost, st));
		EXCHK(ground_clouds_down(ctx, P, Z, ground, cap_ground, ground_down, cap_ground_down, &n_out[0], &n_out[1]));
		n_out[2] = Z.go.n_unground;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	// the host cloud into the scan's region, the classification stage alone, the clouds down from where the kernels (or the host's samplers) left them
	int mulls_classify_nground(mulls_ctx *ctx, const void *pts, uint32_t n_in, uint32_t stride, const mulls_classify_params *P, void *const out[MULLS_CL_COUNT],
							   const uint32_t cap[MULLS_CL_COUNT], uint32_t n_out[MULLS_CL_COUNT], void *cloud_in_after, uint32_t *n_cloud_in_after)
	try
	{
		if (!ctx || !P || !out || !cap || !n_out || (n_in && !pts) || stride < MULLS_POINT_BYTES)
			return MULLS_E_INVALID;
		for (int k = 0; k < MULLS_CL_COUNT; k++)
		{
			n_out[k] = 0;
			if (cap[k] && !out[k])
				return MULLS_E_INVALID;
		}
		if (mulls_classify_check(ctx, P) != MULLS_OK)
			return MULLS_E_INVALID;
		if (n_in > 2000000u)
		{
			ctx->err = "mulls_classify_nground: more than 2000000 points in one cloud";
			return MULLS_E_UNSUPPORTED;
		}
		// random_downsample_pcl(cloud_in, unground_down_fixed_num) (:2088-2089) leaves this many
		const uint32_t n = classify_work_points(n_in, P->fixed_num_downsampling != 0, P->unground_down_fixed_num);
		if (n_cloud_in_after)
			*n_cloud_in_after = n;
		if (n == 0)
			return MULLS_OK;
		HIPCHK(ctx, hipSetDevice(ctx->device));
		hipStream_t st = ctx->stream;
		const mulls::StreamDrain drain{st};
		std::vector<ScanState> sc;
		const int rc = run_one(ctx, EX_CLASSIFY, "mulls_classify_nground", pts, n_in, stride, nullptr, nullptr, P, nullptr, nullptr, nullptr, sc);
		if (rc != MULLS_OK)
			return rc;
		EXCHK(class_clouds_down(ctx, sc[0], out, cap, n_out, cloud_in_after));
		HIPCHK(ctx, hipStreamSynchronize(st));
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}
}
