// extract_batch.cpp — host side of mulls_extract_features_batch (include/mulls_hip.h): extract_impl's chain (ground.cpp) and
// mulls_classify_impl's (classify.cpp) for many scans per call.  A sub-batch's scans lie side by side in one arena (extract_batch.h: every scan gets the
// regions its single call carves); every device step is ONE launch over a table with one entry per scan (the *_batch launchers of k_ground.hip,
// k_classify.hip, map_kernels.hip), every copy or fill the single path issues per array is one range of a k_ex_segs launch, and every host wait of the
// single path happens once per sub-batch:
//   1 sizes after the pre-filter   2 GfOut   3 (thinning masks up)   4 promotion rounds   5 class counts, non-finite flag   6 keys down, orders up
//   7 suppression rounds           8 *_down sizes (and the clouds the host thins)          9 block placement
// What the host decides per scan — thin_mask, std::sort's visiting orders, the sector samplers — is the single path's code on the single path's inputs.
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
	unsigned char *gf = nullptr, *cl = nullptr, *cur = nullptr, *other = nullptr;
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
};

// the tables and byte ranges of one sub-batch on their way to the device, and the statistics
struct Run
{
	mulls_ctx *ctx;
	hipStream_t st;
	mulls_extract_batch_stats *S;
	unsigned char *tab_dev = nullptr; // device table area (inside the arena), mirrored by ctx->exb_tab_pin
	size_t tab_cap = 0, tab_off = 0;
	unsigned char *pin_dev = nullptr; // device address of ctx->exb_pin
	size_t pin_off = 0;
	std::vector<ExSeg> segs;
	uint32_t seg_max = 0;

	// a table to the device (one copy command); nullptr: failed
	template <typename T>
	const T *upload(const std::vector<T> &v)
	{
		const size_t bytes = v.size() * sizeof(T);
		tab_off = (tab_off + 63u) & ~(size_t)63u;
		if (tab_off + bytes > tab_cap)
		{
			ctx->err = "mulls_extract_features_batch: table area exhausted";
			return nullptr;
		}
		std::memcpy(ctx->exb_tab_pin + tab_off, v.data(), bytes);
		if (hipMemcpyAsync(tab_dev + tab_off, ctx->exb_tab_pin + tab_off, bytes, hipMemcpyHostToDevice, st) != hipSuccess)
		{
			ctx->err = "mulls_extract_features_batch: table upload failed";
			return nullptr;
		}
		const T *p = reinterpret_cast<const T *>(tab_dev + tab_off);
		tab_off += bytes;
		return p;
	}
	// the pinned scratch holds `bytes` from its start (called with the stream idle)
	int pin_reserve(size_t bytes)
	{
		if (ctx->exb_pin_cap < bytes)
		{
			if (ctx->exb_pin)
				(void)hipHostFree(ctx->exb_pin);
			ctx->exb_pin = nullptr, ctx->exb_pin_cap = 0;
			const size_t want = bytes + bytes / 4 + 4096;
			HIPCHK(ctx, hipHostMalloc((void **)&ctx->exb_pin, want, hipHostMallocMapped));
			ctx->exb_pin_cap = want;
		}
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

#define EXCHK(call)            \
	do                         \
	{                          \
		const int rc_ = (call); \
		if (rc_ != MULLS_OK)   \
			return rc_;        \
	} while (0)

// one sub-batch: the scans first .. last of `sc` whose `live` is set, in lock step
int run_subbatch(Run &R, const mulls_cloud *scans, const mulls_extract_params *X, mulls_block *const *blocks, mulls_extract_batch_result *results, std::vector<ScanState> &sc,
				 uint32_t first, uint32_t last, const ScanRegion *reg, uint64_t arena_bytes)
{
	mulls_ctx *ctx = R.ctx;
	hipStream_t st = R.st;
	mulls_extract_batch_stats &S = *R.S;
	const mulls_ground_params *P = &X->ground;
	const mulls_classify_params *C = &X->classify;
	const uint32_t m = last - first;
	const bool scanner = X->apply_scanner_filter != 0, dist = X->apply_dist_filter != 0, prefilter = scanner || dist;
	// ---- the arena and the tables -----------------------------------------------------------------------------------------------------------
	if (ctx->exb_cap < arena_bytes)
	{
		if (ctx->exb_buf)
			(void)hipFree(ctx->exb_buf);
		ctx->exb_buf = nullptr, ctx->exb_cap = 0;
		HIPCHK(ctx, hipMalloc(&ctx->exb_buf, arena_bytes));
		ctx->exb_cap = arena_bytes;
	}
	unsigned char *arena = static_cast<unsigned char *>(ctx->exb_buf);
	uint32_t *d_round = reinterpret_cast<uint32_t *>(arena); // 64 counters of the round loops, shared by the scans
	R.tab_dev = arena + MULLS_EXB_HEAD_BYTES, R.tab_cap = (size_t)MULLS_EXB_TABLE_BYTES * m, R.tab_off = 0;
	if (grow_pinned(ctx, &ctx->exb_tab_pin, &ctx->exb_tab_pin_cap, R.tab_cap, hipHostMallocDefault) != MULLS_OK)
		return MULLS_E_HIP;
	const size_t words_bytes = (size_t)m * 256; // a row of 64 words per scan: what every wait reads
	auto words_of = [&](uint32_t s) { return reinterpret_cast<uint32_t *>(ctx->exb_pin) + (size_t)(s - first) * 64; };
	EXCHK(R.pin_reserve(words_bytes + 64));
	R.pin_off = words_bytes;
	if (P->estimate_ground_normal_method == 3 && gf_rnd_table(ctx) != MULLS_OK)
		return MULLS_E_HIP;

	// ---- the scans go up (pageable ones of a MB and more through the context's pinned scratch, as a single call's) ---------------------------------
	{
		std::vector<uint8_t> stage(m, 0), on_dev(m, 0);
		size_t pin_need = 0;
		for (uint32_t s = first; s < last; s++)
		{
			ScanState &Z = sc[s];
			if (!Z.live)
				continue;
			Z.a = gf_layout(Z.n_in, prefilter, false, P->estimate_ground_normal_method);
			Z.gf = arena + reg[s].o_gf, Z.cl = arena + reg[s].o_cl;
			Z.cur = prefilter ? Z.gf + Z.a.o_alt : Z.gf, Z.other = prefilter ? Z.gf : Z.gf + Z.a.o_alt;
			hipPointerAttribute_t at;
			const hipError_t qe = hipPointerGetAttributes(&at, scans[s].pts);
			const bool pageable = qe != hipSuccess || at.type == hipMemoryTypeUnregistered;
			if (qe != hipSuccess)
				(void)hipGetLastError(); // not an error of this call
			else
				on_dev[s - first] = at.type == hipMemoryTypeDevice;
			if (scans[s].stride == REC && pageable && (size_t)Z.n_in * REC >= ((size_t)1 << 20))
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

	// ---- dist_filter, scanner_filter: one mask launch, one compaction, one look at the sizes (wait 1) ---------------------------------------------------
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
			Z.live = false; // an empty block, MULLS_OK
	}

	// ---- fast_ground_filter: GfOut of every scan in one look (wait 2) ----------------------------------------------------------------------------------------
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
			}
		}
	}

	// ---- classify_nground_pts ----------------------------------------------------------------------------------------------------------------------------------
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
			const unsigned char *src = Z.gf + Z.a.o_unground;
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
				"mulls_extract_features_batch: the promotion loop did not settle", &S.n_syncs);
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
				"mulls_extract_features_batch: the suppression rounds did not settle", &S.n_syncs); // wait 7
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

	// ---- block placement (wait 9): every block sized first and grown at most once, then all clouds of all scans in one launch ---------------------------------
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
			const uint32_t cntk[MULLS_CL_COUNT] = {Z.ncls[0], Z.ncls[1], Z.ncls[2], Z.ncls[3], Z.ndown[0], Z.ndown[1], Z.ndown[2], Z.ndown[3], Z.nvertex};
			const float4 *dev[MULLS_CL_COUNT] = {Z.cls[0], Z.cls[1], Z.cls[2], Z.cls[3], Z.L.down[0], Z.L.down[1], Z.L.down[2], Z.L.down[3], Z.L.vertex};
			uint32_t cnt[MULLS_EX_COUNT] = {};
			cnt[MULLS_EX_GROUND] = Z.go.n_ground, cnt[MULLS_EX_GROUND_DOWN] = (uint32_t)Z.gd_idx.size(), cnt[MULLS_EX_UNGROUND] = Z.n_cl;
			for (int k = 0; k < MULLS_CL_COUNT; k++)
				cnt[MULLS_EX_PILLAR + k] = Z.classify ? cntk[k] : 0u, n_out[MULLS_EX_PILLAR + k] = cnt[MULLS_EX_PILLAR + k];
			n_out[MULLS_EX_GROUND] = cnt[MULLS_EX_GROUND], n_out[MULLS_EX_GROUND_DOWN] = cnt[MULLS_EX_GROUND_DOWN];
			size_t need = 0, off[MULLS_EX_COUNT];
			for (int k = 0; k < MULLS_EX_COUNT; k++)
			{
				off[k] = need;
				need += ((size_t)cnt[k] * REC + 255) & ~(size_t)255;
			}
			need += Z.gd_idx.size() * 4 + 256; // the selection indices ride at the end
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
				uint32_t *d_idx = reinterpret_cast<uint32_t *>(blk->buf + need - (Z.gd_idx.size() * 4 + 128));
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
} // namespace

extern "C"
{
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
		mulls_extract_batch_stats local;
		std::memset(&local, 0, sizeof(local));
		mulls_extract_batch_stats &S = stats ? *stats : local;
		std::memset(results, 0, sizeof(*results) * n_scans);
		const mulls_ground_params *P = &X->ground;
		auto finish = [&](const std::vector<std::string> &errs) {
			for (uint32_t s = 0; s < n_scans; s++)
				if (results[s].status != MULLS_OK)
				{
					ctx->err = "mulls_extract_features_batch: scan " + std::to_string(s) + ": " + errs[s];
					return (int)results[s].status;
				}
			return (int)MULLS_OK;
		};
		std::vector<std::string> errs(n_scans);
		// the two parameter points of the single-scan path (and parameters every single call would refuse: it says how)
		const bool voxels = !(X->vf_downsample_resolution < 0.001);
		const int method = P->estimate_ground_normal_method;
		const bool refused = gf_check(ctx, P, 0) != MULLS_OK || mulls_classify_check(ctx, &X->classify) != MULLS_OK;
		if (voxels || method == 1 || method == 2 || refused)
		{
			void *no_out[MULLS_EX_COUNT] = {};
			uint32_t no_cap[MULLS_EX_COUNT] = {};
			for (uint32_t s = 0; s < n_scans; s++)
			{
				results[s].path = 1;
				results[s].status = extract_impl(ctx, scans[s].pts, scans[s].n, scans[s].stride, X, no_out, no_cap, results[s].n_out, blocks[s]);
				if (results[s].status != MULLS_OK)
				{
					errs[s] = ctx->err;
					for (int k = 0; k < MULLS_EX_COUNT; k++)
						blocks[s]->n[k] = 0;
				}
				S.n_single_path++;
			}
			return finish(errs);
		}
		HIPCHK(ctx, hipSetDevice(ctx->device));
		const mulls::StreamDrain drain{ctx->stream};
		const bool prefilter = X->apply_scanner_filter != 0 || X->apply_dist_filter != 0;
		std::vector<ScanState> sc(n_scans);
		std::vector<ScanCost> cost(n_scans);
		std::vector<uint64_t> bytes(n_scans);
		for (uint32_t s = 0; s < n_scans; s++)
		{
			for (int k = 0; k < MULLS_EX_COUNT; k++)
				blocks[s]->n[k] = 0;
			sc[s].n_in = sc[s].n = scans[s].n;
			sc[s].status = gf_check(ctx, P, scans[s].n);
			if (sc[s].status != MULLS_OK)
				sc[s].err = ctx->err;
			sc[s].live = sc[s].status == MULLS_OK && scans[s].n > 0;
			cost[s] = extract_batch_scan_cost(sc[s].live ? scans[s].n : 0u, prefilter, method, X->classify.fixed_num_downsampling != 0, X->classify.unground_down_fixed_num,
											  (uint32_t)X->classify.neighbor_k);
			bytes[s] = cost[s].total;
			S.n_lockstep++;
		}
		std::vector<uint32_t> cuts;
		extract_batch_cuts(bytes.data(), n_scans, scratch_limit_bytes ? scratch_limit_bytes : MULLS_EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES, &cuts);
		std::vector<ScanRegion> reg(n_scans);
		Run R{ctx, ctx->stream, &S};
		int rc = MULLS_OK;
		for (size_t k = 0; k + 1 < cuts.size() && rc == MULLS_OK; k++)
		{
			const uint64_t arena_bytes = extract_batch_offsets(cost.data(), cuts[k], cuts[k + 1], reg.data());
			S.n_subbatches++;
			rc = run_subbatch(R, scans, X, blocks, results, sc, cuts[k], cuts[k + 1], reg.data(), arena_bytes);
		}
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
			errs[s] = sc[s].err;
			if (sc[s].status != MULLS_OK)
				for (int k = 0; k < MULLS_EX_COUNT; k++)
					blocks[s]->n[k] = 0;
		}
		return finish(errs);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}
}
