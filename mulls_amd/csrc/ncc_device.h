// ncc_device.h — key-point descriptor matching: CRegistration<PointT>::find_feature_correspondence_ncc (cregistration.hpp:409-601) for gfx950.  The
// arithmetic of the k_nb_* kernels (k_ncc_batch.hip): the descriptors, d(i, j), a table pass over one (row block, column range), the digit rule of the
// fixed-number selection, and the bodies of the single-workgroup steps.  A kernel only decides which problem, row block and column range a workgroup
// works on; nothing here reads blockIdx.
//
// The reference fills an Nt x Ns table of L1 distances between 11-float "neighbourhood category context" descriptors and then reads it three ways: row minima
// (nearest neighbour), column minima (the reciprocal test), or its corr_num smallest entries (a sort of all Nt * Ns).  Here the table is never stored.  One
// lane owns one row point, its descriptor in registers; the column descriptors are the same for every lane of a wave at the same time, so they come
// through the scalar cache into SGPRs (no LDS, no vector loads in the loop) and an entry costs its 22 VALU operations and nothing else.  d(i, j) is
// recomputed by the same eleven float additions in k order in every pass and with either cloud as the rows (|a - b| == |b - a| bit for bit), which is what lets
// the passes agree on equal distances.  Built with -ffp-contract=off like the rest of the library (there is no multiply in the distance anyway).
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>

#include "ncc_launch.h"

constexpr uint32_t NCC_ROWS = MULLS_NCC_ROWS, NCC_WGS = MULLS_NCC_WGS; // (ncc_launch.h: the planner of ncc_batch.h counts workgroups with the same two)
constexpr uint32_t FLT_MAX_BITS = 0x7f7fffffu;

// (int)x as the reference's x86 build evaluates it: cvttss2si returns INT_MIN for NaN and for values outside the int range (as k_ground.hip)
__device__ __forceinline__ int f2i_x86(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000; }

// live float k (0 data[3], 1 normal[0], 2 normal[1], 3 normal[3], 4 intensity) of key point i
__device__ __forceinline__ float ncc_field(const NccCloudIn &c, uint32_t i, uint32_t k)
{
	return c.packed ? c.p[(size_t)i * MULLS_NCC_LIVE + k] : c.p[(size_t)i * 12u + (k < 3u ? 3u + k : 4u + k)];
}

// intensity_min = min_(intensity_min, cur_i), intensity_max = max_(...) over the target in index order (:433-442), with min_(a, b) = a < b ? a : b.
// Without a NaN that is min(FLT_MAX, all) and max(0, all).  A NaN intensity replaces the running value and is itself replaced by the next one, so the
// loop's result is the plain min / max of the points behind the last NaN (and NaN when the last point is it): reproduced as such.  One workgroup of 1024.
__device__ __forceinline__ void ncc_minmax_fold(NccCloudIn tgt, float *mm)
{
	__shared__ float s_lo[1024], s_hi[1024];
	__shared__ uint32_t s_last[1024];
	const uint32_t t = threadIdx.x;
	uint32_t last = 0;
	for (uint32_t i = t; i < tgt.n; i += 1024u)
	{
		const float v = ncc_field(tgt, i, 4);
		if (v != v)
			last = i + 1u; // i ascends: the last one stays
	}
	s_last[t] = last;
	__syncthreads();
	for (uint32_t w = 512u; w; w >>= 1)
	{
		if (t < w)
			s_last[t] = max(s_last[t], s_last[t + w]);
		__syncthreads();
	}
	const uint32_t first = s_last[0]; // the fold restarts here
	float lo = __builtin_inff(), hi = -__builtin_inff();
	for (uint32_t i = first + t; i < tgt.n; i += 1024u)
	{
		const float v = ncc_field(tgt, i, 4);
		lo = v < lo ? v : lo;
		hi = v > hi ? v : hi;
	}
	s_lo[t] = lo;
	s_hi[t] = hi;
	__syncthreads();
	for (uint32_t w = 512u; w; w >>= 1)
	{
		if (t < w)
		{
			s_lo[t] = s_lo[t + w] < s_lo[t] ? s_lo[t + w] : s_lo[t];
			s_hi[t] = s_hi[t + w] > s_hi[t] ? s_hi[t + w] : s_hi[t];
		}
		__syncthreads();
	}
	if (t == 0)
	{
		lo = s_lo[0];
		hi = s_hi[0];
		if (first == 0u)
		{
			lo = FLT_MAX < lo ? FLT_MAX : lo;
			hi = 0.0f > hi ? 0.0f : hi;
		}
		else if (first >= tgt.n)
			lo = hi = __builtin_nanf("");
		mm[0] = lo;
		mm[1] = hi;
	}
}

// the descriptor of :446-462 / :470-486, entry 11 = 0, of key point g of the target followed by the source (g < tgt.n + src.n), and its key's preset
__device__ __forceinline__ void ncc_describe(NccCloudIn tgt, NccCloudIn src, const float *__restrict__ mm, float4 *desc_t, float4 *desc_s,
											 unsigned long long *rowkey, unsigned long long *colkey, uint32_t g)
{
	const bool is_t = g < tgt.n;
	const NccCloudIn &c = is_t ? tgt : src;
	const uint32_t i = is_t ? g : g - tgt.n;
	const float intensity_min = mm[0], intensity_max = mm[1];
	const int cl = f2i_x86(ncc_field(c, i, 1)), fa = f2i_x86(ncc_field(c, i, 2));
	float4 a, b, d;
	a.x = (float)(cl / 1000000);
	a.y = (float)((cl % 1000000) / 10000);
	a.z = (float)((cl % 10000) / 100);
	a.w = (float)(cl % 100);
	b.x = (float)(fa / 1000000);
	b.y = (float)((fa % 1000000) / 10000);
	b.z = (float)((fa % 10000) / 100);
	b.w = (float)(fa % 100);
	const float cur_i = ncc_field(c, i, 4);
	d.x = (float)((double)((cur_i - intensity_min) / (intensity_max - intensity_min)) * 255.0); // float quotient, double product, narrowed by the store
	d.y = ncc_field(c, i, 3) * 100.0f;
	d.z = ncc_field(c, i, 0) * 30.0f;
	d.w = 0.0f;
	float4 *o = (is_t ? desc_t : desc_s) + (size_t)i * 3u;
	o[0] = a;
	o[1] = b;
	o[2] = d;
	(is_t ? rowkey : colkey)[i] = (unsigned long long)FLT_MAX_BITS << 32; // min_dist_row = FLT_MAX, min_dist_col_index = 0 (:522-523)
}

// d(i, j) of :504-505: a float accumulator from +0, the eleven terms in k order
__device__ __forceinline__ float ncc_dist(const float4 &r0, const float4 &r1, const float4 &r2, const float4 &c0, const float4 &c1, const float4 &c2)
{
	float d = 0.0f;
	d += fabsf(r0.x - c0.x);
	d += fabsf(r0.y - c0.y);
	d += fabsf(r0.z - c0.z);
	d += fabsf(r0.w - c0.w);
	d += fabsf(r1.x - c1.x);
	d += fabsf(r1.y - c1.y);
	d += fabsf(r1.z - c1.z);
	d += fabsf(r1.w - c1.w);
	d += fabsf(r2.x - c2.x);
	d += fabsf(r2.y - c2.y);
	d += fabsf(r2.z - c2.z);
	return d;
}

// One workgroup's part of a table pass: row block `row_block` of NCC_ROWS rows, the columns j0 <= j < min(n_cols, j0 + chunk).  f(row, col, d) for every
// entry of a valid row.  row_block and j0 are the same for every lane of the workgroup.
template <typename F>
__device__ __forceinline__ void ncc_sweep_at(const float4 *__restrict__ rows, uint32_t n_rows, const float4 *__restrict__ cols, uint32_t n_cols, uint32_t row_block,
											 uint32_t j0, uint32_t chunk, F &&f)
{
	const uint32_t row = row_block * NCC_ROWS + threadIdx.x;
	const bool valid = row < n_rows;
	const float4 *rp = rows + (size_t)(valid ? row : n_rows - 1u) * 3u;
	const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
	const uint32_t j1 = min(n_cols, j0 + chunk);
	if (j0 >= j1)
		return;
	// wave-uniform addresses: scalar loads.  Column j + 1 is asked for before column j is used, so that the scalar cache's latency runs under the arithmetic
	const float4 *cp = cols + (size_t)j0 * 3u;
	float4 n0 = cp[0], n1 = cp[1], n2 = cp[2];
	for (uint32_t j = j0; j < j1; j++)
	{
		const float4 c0 = n0, c1 = n1, c2 = n2;
		cp = cols + (size_t)min(j + 1u, j1 - 1u) * 3u;
		n0 = cp[0];
		n1 = cp[1];
		n2 = cp[2];
		const float d = ncc_dist(r0, r1, r2, c0, c1, c2);
		if (valid)
			f(row, j, d);
	}
}

// the loop of :524-531 over this workgroup's columns, merged over the chunks by a 64-bit minimum of (bits of d, column): d >= +0 orders like its bit pattern,
// a NaN or an infinity is never below FLT_MAX and never gets here, and among equal distances the lowest column wins as the strict `<` of :526 has it
__device__ __forceinline__ void ncc_rowmin_at(const float4 *__restrict__ rows, uint32_t n_rows, const float4 *__restrict__ cols, uint32_t n_cols, uint32_t row_block,
											  uint32_t j0, uint32_t chunk, unsigned long long *key)
{
	float best = FLT_MAX;
	uint32_t best_j = 0;
	ncc_sweep_at(rows, n_rows, cols, n_cols, row_block, j0, chunk, [&](uint32_t, uint32_t j, float d) {
		if (d < best)
		{
			best = d;
			best_j = j;
		}
	});
	const uint32_t row = row_block * NCC_ROWS + threadIdx.x;
	if (row < n_rows && best < FLT_MAX)
		atomicMin(&key[row], ((unsigned long long)__float_as_uint(best) << 32) | best_j);
}

// :532-549 — the pair (i, j*) goes unless some target is strictly closer to j* than i is (dist_margin_thre = 0; a NaN drops nothing).  colkey[j] holds
// min(FLT_MAX, min over the targets of d(., j)), and d*(i) <= FLT_MAX, so `d*(i) > colmin` decides exactly what the loop of :535-542 decides.
// One workgroup of 1024, chunks of 1024 targets in ascending order: ballot ranks inside a wave, the waves' counts in LDS, the running total in a register.
__device__ __forceinline__ void ncc_recip_compact(const unsigned long long *__restrict__ rowkey, const unsigned long long *__restrict__ colkey, uint32_t n_t,
												  int reciprocal, uint32_t *out)
{
	__shared__ uint32_t s_wave[16];
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	uint32_t total = 0;
	for (uint32_t base = 0; base < n_t; base += 1024u)
	{
		const uint32_t i = base + t;
		bool keep = false;
		uint32_t j = 0;
		if (i < n_t)
		{
			const unsigned long long k = rowkey[i];
			j = (uint32_t)k;
			keep = true;
			if (reciprocal)
				keep = !(__uint_as_float((uint32_t)(k >> 32)) > __uint_as_float((uint32_t)(colkey[j] >> 32)));
		}
		const unsigned long long m = __ballot(keep);
		if (lane == 0)
			s_wave[wave] = (uint32_t)__popcll(m);
		__syncthreads();
		uint32_t before = 0, all = 0;
		for (uint32_t w = 0; w < 16u; w++)
		{
			const uint32_t c = s_wave[w];
			before += w < wave ? c : 0u;
			all += c;
		}
		if (keep)
		{
			const uint32_t pos = total + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
			out[2u + pos] = i;
			out[2u + n_t + pos] = j;
		}
		total += all;
		__syncthreads();
	}
	if (t == 0)
		out[0] = total;
}

// ---- fixed-number mode: the K smallest (d, flat index) keys without sorting Nt * Ns of them ----------------------------------------------------------
// A radix selection on the 62-bit key (31 bits of d's pattern, 31 bits of i * Ns + j), most significant digit first: digits of 11, 10, 10 bits of d, then — only
// when the K-th distance is shared by more entries than fit — 11, 10, 10 bits of the flat index.  A level = one table pass that counts the entries agreeing
// with the digits found so far into an LDS histogram per workgroup (flushed once), and one small kernel that finds the bucket holding the rank.

template <uint32_t LEVEL>
__device__ __forceinline__ bool ncc_level_bucket(uint32_t db, uint32_t idx, uint32_t thr_d, uint32_t thr_i, uint32_t &bucket)
{
	if constexpr (LEVEL == 0u)
	{
		bucket = db >> 20;
		return db <= 0x7f800000u; // every distance that is not a NaN (d >= +0: no sign bit)
	}
	else if constexpr (LEVEL == 1u)
	{
		bucket = (db >> 10) & 1023u;
		return (db >> 20) == (thr_d >> 20);
	}
	else if constexpr (LEVEL == 2u)
	{
		bucket = db & 1023u;
		return (db >> 10) == (thr_d >> 10);
	}
	else if constexpr (LEVEL == 3u)
	{
		bucket = idx >> 20;
		return db == thr_d;
	}
	else if constexpr (LEVEL == 4u)
	{
		bucket = (idx >> 10) & 1023u;
		return db == thr_d && (idx >> 20) == (thr_i >> 20);
	}
	else
	{
		bucket = idx & 1023u;
		return db == thr_d && (idx >> 10) == (thr_i >> 10);
	}
}

// one workgroup's part of the histogram pass of level LEVEL (the level is a template argument: decided per table entry at run time a pass over
// 16 384 x 12 288 took 201 us instead of 138)
template <uint32_t LEVEL>
__device__ __forceinline__ void ncc_hist_at(const float4 *__restrict__ desc_t, uint32_t n_t, const float4 *__restrict__ desc_s, uint32_t n_s, uint32_t row_block,
											uint32_t j0, uint32_t chunk, const NccSel *__restrict__ sel, uint32_t *hist)
{
	__shared__ uint32_t s_hist[MULLS_NCC_HIST_BUCKETS];
	if (sel->done | sel->none)
		return;
	const uint32_t thr_d = sel->thr_d, thr_i = sel->thr_i;
	for (uint32_t b = threadIdx.x; b < MULLS_NCC_HIST_BUCKETS; b += NCC_ROWS)
		s_hist[b] = 0;
	__syncthreads();
	ncc_sweep_at(desc_t, n_t, desc_s, n_s, row_block, j0, chunk, [&](uint32_t i, uint32_t j, float d) {
		uint32_t bucket;
		if (ncc_level_bucket<LEVEL>(__float_as_uint(d), i * n_s + j, thr_d, thr_i, bucket))
			atomicAdd(&s_hist[bucket], 1u);
	});
	__syncthreads();
	uint32_t *h = hist + LEVEL * MULLS_NCC_HIST_BUCKETS;
	for (uint32_t b = threadIdx.x; b < MULLS_NCC_HIST_BUCKETS; b += NCC_ROWS)
		if (s_hist[b])
			atomicAdd(&h[b], s_hist[b]);
}

// the bucket of level `level` that holds the rank, one workgroup of 256: 8 consecutive buckets per thread
__device__ __forceinline__ void ncc_pick_bucket(uint32_t level, uint32_t K, NccSel *sel, const uint32_t *__restrict__ hist)
{
	__shared__ uint32_t s_sum[256], s_rem;
	if (sel->done | sel->none)
		return;
	const uint32_t t = threadIdx.x;
	const uint32_t *h = hist + level * MULLS_NCC_HIST_BUCKETS;
	uint32_t c[8], mine = 0;
	for (uint32_t k = 0; k < 8u; k++)
	{
		c[k] = h[t * 8u + k];
		mine += c[k];
	}
	s_sum[t] = mine;
	__syncthreads();
	if (t == 0)
	{
		uint32_t run = 0;
		for (uint32_t k = 0; k < 256u; k++)
		{
			const uint32_t v = s_sum[k];
			s_sum[k] = run;
			run += v;
		}
		// level 0 counts every selectable entry: with fewer than K of them all are taken (the sorted table's NaNs come last and are never selected)
		s_rem = level == 0u ? min(K, run) : sel->remaining;
		if (level == 0u && run == 0u)
			sel->none = 1u;
	}
	__syncthreads();
	const uint32_t rem = s_rem;
	if (rem == 0u)
		return;
	uint32_t cum = s_sum[t];
	for (uint32_t k = 0; k < 8u; k++)
	{
		if (cum < rem && rem <= cum + c[k])
		{
			const uint32_t b = t * 8u + k, left = rem - cum;
			sel->remaining = left;
			switch (level)
			{
			case 0:
				sel->thr_d = b << 20;
				break;
			case 1:
				sel->thr_d |= b << 10;
				break;
			case 2:
				sel->thr_d |= b;
				if (left == c[k]) // every entry at the K-th distance is among the K smallest: no need to look at flat indices
				{
					sel->thr_i = 0xffffffffu;
					sel->done = 1u;
				}
				break;
			case 3:
				sel->thr_i = b << 20;
				break;
			case 4:
				sel->thr_i |= b << 10;
				break;
			default:
				sel->thr_i |= b;
				sel->done = 1u;
				break;
			}
		}
		cum += c[k];
	}
}

// one workgroup's part of the collection: every key up to the rank-K key, unordered (the host orders the at most 65 536 of them); slots by one atomic per
// wave and hit
__device__ __forceinline__ void ncc_collect_at(const float4 *__restrict__ desc_t, uint32_t n_t, const float4 *__restrict__ desc_s, uint32_t n_s, uint32_t row_block,
											   uint32_t j0, uint32_t chunk, uint32_t K, const NccSel *__restrict__ sel, unsigned long long *cand)
{
	if (sel->none)
		return;
	const uint32_t thr_d = sel->thr_d, thr_i = sel->thr_i;
	uint32_t *counter = reinterpret_cast<uint32_t *>(cand);
	ncc_sweep_at(desc_t, n_t, desc_s, n_s, row_block, j0, chunk, [&](uint32_t i, uint32_t j, float d) {
		const uint32_t db = __float_as_uint(d), idx = i * n_s + j;
		if (db < thr_d || (db == thr_d && idx <= thr_i))
		{
			const unsigned long long m = __ballot(1);
			const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)m) - 1u;
			uint32_t base = 0;
			if (lane == leader)
				base = atomicAdd(counter, (uint32_t)__popcll(m));
			base = (uint32_t)__shfl((int)base, (int)leader);
			const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
			if (slot < K) // exactly min(K, selectable entries) keys qualify; the bound is the buffer's
				cand[1u + slot] = ((unsigned long long)db << 32) | idx;
		}
	});
}
