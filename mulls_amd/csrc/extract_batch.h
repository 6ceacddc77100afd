// extract_batch.h — arena arithmetic of the feature stage and the planner of mulls_extract_features_batch (include/mulls_hip.h).
// Host code only (no kernel, no runtime call), so that tests/extract_batch_harness.cpp can hold it on the CPU.  gf_layout and carve are the formulas of a
// scan's two regions, whichever entry point runs it (a single call is a batch of one): the scans of a sub-batch lie side by side,
//   arena = tables (EXB_TABLE_BYTES per scan, behind EXB_HEAD_BYTES of shared words) | scan 0: ground region, classify region | scan 1: ... | ...
// and the batch is cut into consecutive sub-batches whose arenas stay at or below the caller's limit; a scan larger than the limit runs alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "classify_launch.h"
#include "ground_launch.h"
#include "subbatch.h"

namespace mulls_ex
{
struct GfArena // one device arena: scan | ground | unground | ids | d3v | cellof | code | state, counters, per-cell tables | (filters / voxels ahead:) scan copy, mask, scratch, voxel keys, order
{
	size_t o_ground, o_unground, o_ids, o_d3, o_cell, o_code, o_aux, o_alt, o_mask, o_seg, o_keys, o_perm, o_ransac, o_normals, total;
};
// prefilter: dist_filter / scanner_filter ahead of the ground filter; voxels: voxel_downsample ahead of it (either needs a second scan-sized buffer)
inline GfArena gf_layout(uint32_t n, bool prefilter, bool voxels, int normal_method = 0)
{
	GfArena a;
	const size_t rec = (size_t)n * MULLS_POINT_BYTES;
	a.o_ground = rec, a.o_unground = 2 * rec, a.o_ids = 3 * rec, a.o_d3 = a.o_ids + (size_t)n * 4, a.o_cell = a.o_d3 + (size_t)n * 4;
	a.o_code = a.o_cell + (size_t)n * 2;
	a.o_aux = (a.o_code + n + 255) & ~(size_t)255;
	a.o_alt = (a.o_aux + ground_filter_aux_bytes(n) + 255) & ~(size_t)255;
	a.o_mask = a.o_alt + (prefilter || voxels ? rec : 0);
	a.o_seg = (a.o_mask + (prefilter ? n : 0) + 255) & ~(size_t)255;
	a.o_keys = (a.o_seg + (prefilter ? ((size_t)n / 4096 + 32) * 4 * 8 : 0) + 255) & ~(size_t)255;
	a.o_perm = a.o_keys + (voxels ? (size_t)n * 8 + 256 : 0);
	// normal method 3: gg | perm | inl (uint32 each) | gxyz (float4) | cell_nrm (float4 per cell); methods 1 / 2: the neighbour grid of the ground cloud
	a.o_ransac = (a.o_perm + (voxels ? (size_t)n * 4 : 0) + 255) & ~(size_t)255;
	a.o_normals = a.o_ransac + (normal_method == 3 ? (size_t)n * 28 + (size_t)MULLS_GF_MAXCELLS * 16 + 256 : 0);
	a.total = a.o_normals + ((normal_method == 1 || normal_method == 2) ? ground_normals_bytes(n) : 0);
	return a;
}
// the plane RANSAC's scratch inside a ground arena at `base` (normal method 3); rnd: the context's sample table
inline GfRansac gf_ransac_at(unsigned char *base, const GfArena &a, uint32_t n, const void *rnd)
{
	GfRansac R = {};
	unsigned char *r = base + a.o_ransac;
	R.gg = reinterpret_cast<uint32_t *>(r);
	R.perm = R.gg + n;
	R.inl = R.perm + n;
	R.gxyz = reinterpret_cast<float4 *>((reinterpret_cast<uintptr_t>(R.inl + n) + 15) & ~(uintptr_t)15);
	R.cell_nrm = R.gxyz + n;
	R.rnd = static_cast<const uint32_t *>(rnd);
	return R;
}

struct Bump // carve device arrays out of one arena
{
	unsigned char *base;
	size_t off;
	template <typename T>
	T *take(size_t count)
	{
		off = (off + 255u) & ~(size_t)255u;
		T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
		off += count * sizeof(T);
		return p;
	}
};

struct Layout
{
	ClArrays A;
	float4 *cls_a[6];	  // pillar, pillar (promoted), beam, beam (promoted), facade, roof: compaction targets, pillar / beam become the class clouds
	float4 *cls_sorted[4]; // class clouds in visiting order
	float4 *down[4], *vertex;
	uint32_t *nms_list[4], *nms_cnt[4], *nms_off[4], *nms_wcur[4], *nms_pool;
	unsigned long long *nms_pool_used;
	uint32_t nms_pool_cap;
	uint8_t *keep[4];
	float *keys;	// [4][n]
	uint32_t *perm; // [4][n]
	uint32_t *counts; // [16]
	uint32_t *seg;	  // compaction scratch
	size_t seg_cap;
	size_t total;
};

// n: points the passes work on; n_in >= n: points of the cloud as handed in (the device-side thinning needs a mask and compaction scratch of that size)
inline Layout carve(unsigned char *base, uint32_t n, uint32_t K, uint32_t n_in)
{
	Layout L;
	Bump b{base, 0};
	ClArrays &A = L.A;
	A.recs = b.take<float4>((size_t)n * 3);
	A.sorted = b.take<float4>(n);
	A.cellof = b.take<uint32_t>(n);
	A.cell_start = b.take<uint32_t>((size_t)MULLS_CL_MAX_CELLS + 1u);
	A.cell_fill = b.take<uint32_t>((size_t)MULLS_CL_MAX_CELLS + 1u);
	A.seg_sum = b.take<uint32_t>(1032);
	A.nbr = b.take<uint32_t>((size_t)n * K);
	A.closebits = b.take<unsigned long long>(n);
	A.f_cnt = b.take<int32_t>(n);
	A.cov = b.take<float>((size_t)n * 6);
	A.f_curv = b.take<double>(n);
	A.f_lin = b.take<double>(n);
	A.f_pla = b.take<double>(n);
	A.f_pd = b.take<float4>(n);
	A.f_nd = b.take<float4>(n);
	A.lab = b.take<uint8_t>(n);
	A.plab = b.take<uint8_t>(n);
	A.cstate = b.take<uint8_t>(n);
	A.cand = b.take<uint8_t>(n);
	A.down = b.take<uint8_t>(n);
	A.mask = b.take<uint8_t>(std::max<size_t>((size_t)n * 11, n_in));
	A.vtx = b.take<float4>((size_t)n * 3);
	A.round_cnt = b.take<uint32_t>(64);
	A.grid = b.take<ClGrid>(1);
	for (int k = 0; k < 6; k++)
		L.cls_a[k] = b.take<float4>((size_t)n * 3);
	for (int k = 0; k < 4; k++)
	{
		L.cls_sorted[k] = b.take<float4>((size_t)n * 3);
		L.down[k] = b.take<float4>((size_t)n * 3);
		L.nms_list[k] = b.take<uint32_t>((size_t)n * MULLS_CL_NMS_CAP);
		L.nms_cnt[k] = b.take<uint32_t>(n);
		L.nms_off[k] = b.take<uint32_t>(n);
		L.nms_wcur[k] = b.take<uint32_t>(n);
		L.keep[k] = b.take<uint8_t>(n);
	}
	L.vertex = b.take<float4>((size_t)n * 3);
	L.nms_pool_cap = (uint32_t)std::min<size_t>((size_t)n * 64u, 0x7fffffffu);
	L.nms_pool = b.take<uint32_t>(L.nms_pool_cap);
	L.nms_pool_used = b.take<unsigned long long>(1);
	L.keys = b.take<float>((size_t)n * 4);
	L.perm = b.take<uint32_t>((size_t)n * 4);
	L.counts = b.take<uint32_t>(16);
	L.seg_cap = (size_t)6 * ((std::max(n, n_in) + 4095u) / 4096u + 1u) + 16;
	L.seg = b.take<uint32_t>(L.seg_cap);
	L.total = b.off + 256;
	return L;
}

// ---- the planner -----------------------------------------------------------------------------------------------------------------------
#define MULLS_EXB_TABLE_BYTES 8192u // a scan's entries in the tables the lock-step kernels read, and its words in the collection rows
#define MULLS_EXB_HEAD_BYTES 4096u	// the round counters and other words the scans of a sub-batch share
#define MULLS_EXB_MAX_SCANS 4096u	// scans of one sub-batch: a grid axis

// how many points of a non-ground cloud of n_in the classification works on (random_downsample_pcl(cloud_in, unground_down_fixed_num), classify.cpp)
inline uint32_t classify_work_points(uint32_t n_in, bool fixed_num, int unground_down_fixed_num)
{
	if (fixed_num && unground_down_fixed_num >= 0 && (long)n_in > (long)unground_down_fixed_num)
		return (uint32_t)unground_down_fixed_num;
	return n_in;
}

struct ScanCost
{
	uint64_t gf, cl, total; // the ground region, the classify region, both with the scan's share of the tables
};
// What a scan of n points may need: its ground arena, and the classify arena of the largest non-ground cloud it can leave (all n points).
// A scan without points takes its table row only.
inline ScanCost extract_batch_scan_cost(uint32_t n, bool prefilter, int normal_method, bool fixed_num, int unground_down_fixed_num, uint32_t K, bool voxels = false)
{
	ScanCost c = {0, 0, MULLS_EXB_TABLE_BYTES};
	if (!n)
		return c;
	c.gf = up256(gf_layout(n, prefilter, voxels, normal_method).total);
	c.cl = up256(carve(nullptr, classify_work_points(n, fixed_num, unground_down_fixed_num), K, n).total);
	c.total = c.gf + c.cl + MULLS_EXB_TABLE_BYTES;
	return c;
}

// the cut rule of subbatch.h: every sub-batch starts from the head.  max_scans = 1: every scan a sub-batch of its own, whatever the limit (the steps
// without a table form run scan-locally)
inline void extract_batch_cuts(const uint64_t *bytes, uint32_t count, uint64_t limit, std::vector<uint32_t> *cuts, uint32_t max_scans = MULLS_EXB_MAX_SCANS)
{
	sub_batch_cuts(bytes, count, limit, max_scans, cuts, MULLS_EXB_HEAD_BYTES);
}

struct ScanRegion
{
	uint64_t o_gf, o_cl; // byte offsets of the scan's two regions in the sub-batch's arena, multiples of 256
};
// the arena of the scans [first, last): head, tables, then every scan's regions in order.  Returns the arena's bytes (the sum the cuts counted).
inline uint64_t extract_batch_offsets(const ScanCost *cost, uint32_t first, uint32_t last, ScanRegion *out)
{
	uint64_t off = MULLS_EXB_HEAD_BYTES + (uint64_t)MULLS_EXB_TABLE_BYTES * (last - first);
	for (uint32_t b = first; b < last; b++)
	{
		out[b].o_gf = off, off += cost[b].gf;
		out[b].o_cl = off, off += cost[b].cl;
	}
	return off;
}

// a feature block's buffer: the clouds of MULLS_EX_* in order, every offset a multiple of 256, and behind them the n_idx selection indices of
// cloud_ground_down (the gather that fills it reads them from the block)
struct BlockLayout
{
	size_t off[MULLS_EX_COUNT], o_idx, need;
};
inline BlockLayout block_layout(const uint32_t cnt[MULLS_EX_COUNT], size_t n_idx)
{
	BlockLayout b;
	size_t at = 0;
	for (int k = 0; k < MULLS_EX_COUNT; k++)
	{
		b.off[k] = at;
		at += up256((uint64_t)cnt[k] * MULLS_POINT_BYTES);
	}
	b.o_idx = at + 128;
	b.need = at + n_idx * 4 + 256;
	return b;
}
} // namespace mulls_ex
