// ncc_batch.h — mulls_ncc_correspond_batch (include/mulls_hip.h): the per-problem record the kernels of k_ncc_batch.hip read, the
// planner that cuts a batch into sub-batches and lays a sub-batch out in the device arena, and the launchers.  A sub-batch's arena begins with its
// head — the records, then the three prefix tables — followed by the staged host clouds (head and clouds go up in one copy), the per-problem working
// arrays, and the `out` region, which comes down in one copy.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <cmath>
#include <map>
#include <tuple>
#include <vector>

#include "ncc_launch.h"
#include "subbatch.h"

// one problem of a sub-batch as the device sees it.  Offsets are bytes from the arena's base, multiples of 256.
struct NccBatchDesc
{
	uint64_t in_t, in_s;	   // ext_t / ext_s == 0: arena offset of the staged live floats (MULLS_NCC_LIVE per key point; a cloud that several problems name
							   // is staged once, and they share the offset); else the device address of the caller's 48-byte records
	uint64_t desc_t, desc_s;   // n_t / n_s descriptors of three float4
	uint64_t rowkey, colkey;   // n_t / n_s 64-bit keys
	uint64_t mm;			   // intensity_min, intensity_max
	uint64_t out;			   // nearest-neighbour modes: 2 + 2 n_t words (ncc_recip_compact's out); fixed-number mode: 1 + K keys (cand)
	uint64_t sel, hist;		   // fixed-number mode: the NccSel record and the MULLS_NCC_HIST_LEVELS x MULLS_NCC_HIST_BUCKETS words behind it
	uint32_t n_t, n_s, K;	   // K: min(corr_num, n_t * n_s), fixed-number mode only
	uint32_t ext_t, ext_s;	   // the cloud is device-resident
	uint32_t chunk, chunk_swap; // columns per workgroup of a table pass with the targets as rows, and with the roles swapped (the reciprocal test's pass)
	uint32_t wg, wg_swap;	   // the problem's first workgroup of those two passes
	uint32_t blk;			   // ... and its first block of 256 key points of the descriptor launch
};

#define MULLS_NCC_BATCH_MAX_PROBLEMS 16384u	 // problems of one sub-batch
#define MULLS_NCC_BATCH_MAX_WGS (1u << 30)	 // workgroups of one launch (gridDim.x)

struct NccBatchShape // what the planner needs of a problem
{
	uint32_t n_t, n_s, K;
	const void *key_t, *key_s; // host clouds: the pointer, which with n and the stride identifies a cloud for staging once; NULL: device-resident
	uint32_t stride_t, stride_s;
	uint32_t stage_t, stage_s; // index of the staged cloud this side reads (set by ncc_batch_layout), or ~0u
};

struct NccBatchLayout
{
	std::vector<NccBatchDesc> desc;
	std::vector<uint32_t> wg, wg_swap, blk; // the prefix tables, count + 1 entries each: the last is the launch's grid
	std::vector<uint32_t> staged_owner;		// staged cloud k is side (owner & 1: source) of problem (owner >> 1), the first that named it
	std::vector<uint64_t> staged_at;		// ... and lies at this arena offset
	uint64_t o_desc = 0, o_wg = 0, o_wg_swap = 0, o_blk = 0, o_in = 0, up_bytes = 0; // the head and the staged clouds: arena offsets 0 .. up_bytes go up
	uint64_t o_sel = 0, sel_bytes = 0;												 // the records and histograms of all problems: cleared in one go
	uint64_t o_out = 0, out_bytes = 0;												 // comes down in one copy
	uint64_t dev_bytes = 0;
};

inline uint64_t ncc_batch_out_bytes(uint32_t n_t, bool fixed, uint32_t K) { return fixed ? (uint64_t)(1u + K) * 8u : (2u + 2u * (uint64_t)n_t) * 4u; }
inline uint64_t ncc_batch_sel_bytes() { return up256(sizeof(NccSel)) + (uint64_t)MULLS_NCC_HIST_LEVELS * MULLS_NCC_HIST_BUCKETS * 4u; }

// the arena bytes of one problem: an upper bound (both clouds counted as staged for this problem alone; its share of the head as 512)
inline uint64_t ncc_batch_problem_bytes(uint32_t n_t, uint32_t n_s, bool fixed, uint32_t K)
{
	const uint64_t live = MULLS_NCC_LIVE * 4u;
	return up256(n_t * live) + up256(n_s * live) + up256((uint64_t)n_t * 48u) + up256((uint64_t)n_s * 48u) +
		   up256((uint64_t)n_t * 8u) + up256((uint64_t)n_s * 8u) + 256u + up256(ncc_batch_out_bytes(n_t, fixed, K)) +
		   (fixed ? up256(ncc_batch_sel_bytes()) : 0u) + 512u;
}

inline uint64_t ncc_batch_row_blocks(uint32_t n_rows) { return ((uint64_t)n_rows + MULLS_NCC_ROWS - 1u) / MULLS_NCC_ROWS; }

// Columns per workgroup of a table pass of n_rows x n_cols for a problem that is to have about `aim` workgroups: the column range is split until row
// blocks x chunks reach `aim`, into chunks of 32 columns at least (a problem that runs alone has aim = MULLS_NCC_WGS; the grid is flat, so no gridDim.y
// bounds the number of chunks).
// THE CHUNK IS WORK SPLIT ONLY: the row minima are merged by a 64-bit atomicMin, the histograms are integer sums and the collected keys are ordered on the
// host, so no result depends on it.
inline uint32_t ncc_batch_chunk(uint32_t n_rows, uint32_t n_cols, uint64_t aim)
{
	const uint64_t rb = ncc_batch_row_blocks(n_rows);
	uint64_t splits = aim / rb;
	splits = splits < 1u ? 1u : splits;
	uint64_t chunk = (n_cols + splits - 1u) / splits;
	return (uint32_t)(chunk < 32u ? 32u : chunk);
}
// the workgroups of that pass: row blocks x column chunks, at most max(row blocks, aim)
inline uint64_t ncc_batch_wgs(uint32_t n_rows, uint32_t n_cols, uint32_t chunk) { return ncc_batch_row_blocks(n_rows) * (((uint64_t)n_cols + chunk - 1u) / chunk); }

// more workgroups than any launch has for this problem (aim <= MULLS_NCC_WGS), the descriptor launch's blocks included: sub_batch_cuts' second budget,
// so that a launch's grid stays below MULLS_NCC_BATCH_MAX_WGS.  (At most 2^23 + 2048 + 2^24 for 2^31 - 1 key points a side: a problem that runs alone,
// which no budget cuts, has its grids far below that too.)
inline uint64_t ncc_batch_wgs_bound(uint32_t n_t, uint32_t n_s)
{
	const uint64_t rt = ncc_batch_row_blocks(n_t), rs = ncc_batch_row_blocks(n_s);
	return (rt > rs ? rt : rs) + MULLS_NCC_WGS + ((uint64_t)n_t + n_s + 255u) / 256u;
}

// the cut rule of subbatch.h; wgs[b]: ncc_batch_wgs_bound of problem b
inline void ncc_batch_cuts(const uint64_t *bytes, const uint64_t *wgs, uint32_t count, uint64_t limit, std::vector<uint32_t> *cuts) { sub_batch_cuts(bytes, count, limit, MULLS_NCC_BATCH_MAX_PROBLEMS, cuts, 0, wgs, MULLS_NCC_BATCH_MAX_WGS); }

// the arena of the problems shape[0 .. count), and their records
inline void ncc_batch_layout(NccBatchShape *shape, uint32_t count, bool fixed, NccBatchLayout *L)
{
	L->desc.assign(count, NccBatchDesc());
	L->wg.assign(count + 1u, 0u), L->wg_swap.assign(count + 1u, 0u), L->blk.assign(count + 1u, 0u);
	L->staged_owner.clear(), L->staged_at.clear();
	uint64_t off = 0;
	auto take = [&](uint64_t bytes) {
		const uint64_t at = off;
		off += up256(bytes);
		return at;
	};
	L->o_desc = take(sizeof(NccBatchDesc) * (uint64_t)count);
	L->o_wg = take(4u * ((uint64_t)count + 1u)), L->o_wg_swap = take(4u * ((uint64_t)count + 1u)), L->o_blk = take(4u * ((uint64_t)count + 1u));
	// staged host clouds, each distinct (pointer, n, stride) once
	L->o_in = off;
	std::map<std::tuple<const void *, uint32_t, uint32_t>, uint32_t> seen;
	for (uint32_t b = 0; b < count; b++)
		for (uint32_t side = 0; side < 2u; side++)
		{
			const void *key = side ? shape[b].key_s : shape[b].key_t;
			const uint32_t n = side ? shape[b].n_s : shape[b].n_t, stride = side ? shape[b].stride_s : shape[b].stride_t;
			uint32_t &slot = side ? shape[b].stage_s : shape[b].stage_t;
			slot = ~0u;
			if (!key)
				continue;
			const auto found = seen.emplace(std::make_tuple(key, n, stride), (uint32_t)seen.size());
			slot = found.first->second;
			if (found.second)
			{
				L->staged_owner.push_back(b * 2u + side);
				L->staged_at.push_back(take((uint64_t)n * MULLS_NCC_LIVE * 4u));
			}
		}
	L->up_bytes = off;
	// the split: a problem's share of the MULLS_NCC_WGS workgroups the single call aims at is its share of the sub-batch's table entries
	double entries = 0.0; // (a share, and work split only: double is exact enough, and 2^31 x 2^31 tables do not overflow it)
	for (uint32_t b = 0; b < count; b++)
		entries += (double)shape[b].n_t * (double)shape[b].n_s;
	uint64_t wg = 0, wg_swap = 0, blk = 0;
	for (uint32_t b = 0; b < count; b++)
	{
		NccBatchDesc &D = L->desc[b];
		const NccBatchShape &P = shape[b];
		D.n_t = P.n_t, D.n_s = P.n_s, D.K = P.K;
		D.ext_t = P.key_t ? 0u : 1u, D.ext_s = P.key_s ? 0u : 1u;
		D.in_t = P.key_t ? L->staged_at[P.stage_t] : 0u, D.in_s = P.key_s ? L->staged_at[P.stage_s] : 0u; // (device addresses: filled by the caller)
		D.desc_t = take((uint64_t)P.n_t * 48u), D.desc_s = take((uint64_t)P.n_s * 48u);
		D.rowkey = take((uint64_t)P.n_t * 8u), D.colkey = take((uint64_t)P.n_s * 8u);
		D.mm = take(8);
		const uint64_t aim = (uint64_t)std::ceil((double)MULLS_NCC_WGS * ((double)P.n_t * (double)P.n_s / entries)); // (entries >= 100: 10 key points a side at least)
		D.chunk = ncc_batch_chunk(P.n_t, P.n_s, aim), D.chunk_swap = ncc_batch_chunk(P.n_s, P.n_t, aim);
		D.wg = (uint32_t)wg, D.wg_swap = (uint32_t)wg_swap, D.blk = (uint32_t)blk;
		L->wg[b] = D.wg, L->wg_swap[b] = D.wg_swap, L->blk[b] = D.blk;
		wg += ncc_batch_wgs(P.n_t, P.n_s, D.chunk), wg_swap += ncc_batch_wgs(P.n_s, P.n_t, D.chunk_swap);
		blk += ((uint64_t)P.n_t + P.n_s + 255u) / 256u;
	}
	L->wg[count] = (uint32_t)wg, L->wg_swap[count] = (uint32_t)wg_swap, L->blk[count] = (uint32_t)blk;
	L->o_sel = off;
	for (uint32_t b = 0; b < count && fixed; b++)
	{
		L->desc[b].sel = take(sizeof(NccSel));
		L->desc[b].hist = take((uint64_t)MULLS_NCC_HIST_LEVELS * MULLS_NCC_HIST_BUCKETS * 4u);
	}
	L->sel_bytes = off - L->o_sel;
	L->o_out = off;
	for (uint32_t b = 0; b < count; b++)
		L->desc[b].out = take(ncc_batch_out_bytes(shape[b].n_t, fixed, shape[b].K));
	L->out_bytes = off - L->o_out;
	L->dev_bytes = off;
}

// ---- launchers (k_ncc_batch.hip).  arena: the base the offsets count from; head: the records and prefix tables inside it, as laid out above; B problems.
// intensity ranges, descriptors, key presets and — fixed-number mode — the zero of cand's counter
hipError_t launch_ncc_batch_describe(hipStream_t st, unsigned char *arena, const NccBatchLayout &L, uint32_t B, int fixed);
// the row minima of every problem, key[r] = min over the columns of (float bits of d(r, c) << 32 | c): the first column with the strictly smallest distance
// below FLT_MAX; swapped: the column minima (the sources as rows)
hipError_t launch_ncc_batch_rowmin(hipStream_t st, unsigned char *arena, const NccBatchLayout &L, uint32_t B, int swapped);
// out[0] = count, out[2 + k] = i, out[2 + n_t + k] = j*(i) of the k-th surviving target in ascending i
hipError_t launch_ncc_batch_recip(hipStream_t st, unsigned char *arena, const NccBatchLayout &L, uint32_t B, int reciprocal);
// the six digit levels in lock-step (histogram + pick each), then the collection of every key up to the rank-K key into cand[1 ...] (at most
// MULLS_NCC_MAX_CORR, unordered), their count in the low word of cand[0]; sel, hist zeroed by the caller
hipError_t launch_ncc_batch_select(hipStream_t st, unsigned char *arena, const NccBatchLayout &L, uint32_t B);
