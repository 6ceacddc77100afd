// reg_device.h — what the registrations' kernels (k_ndt.hip, k_gicp.hip, k_pcl_icp.hip, k_fpfh.hip, k_reg_table.hip) share, device only: the arena accessor, the
// cell table's probe, claim and 27-cell visitor (reg_table.h), the shell sort of a slot's list, the scan of a table's counts, and the sums: the halving
// tree over MULLS_NDT_TREE strided partials and the count of hits.  Every translation unit expands the same text, so a sum has the same bits in all.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mulls_hip.h"
#include "pcl_icp_math.h"
#include "reg_table.h"

namespace
{
template <typename T>
__device__ inline T *at(unsigned char *arena, uint64_t off)
{
	return reinterpret_cast<T *>(arena + off);
}
constexpr uint64_t EMPTY = 0xffffffffffffffffull;
constexpr uint32_t NO_SLOT = 0xffffffffu;
inline uint32_t blocks_of(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }

// ---- the cell table ----
// does a table take part in a launch?  One that is rebuilt while the problem runs: only while it does
__device__ inline bool table_live(const RegHead &H, const RegTab &T) { return H.status == 0 && T.n_cap != 0 && (!T.rebuilt || (H.running && !H.range)); }
// a table's points: its cloud's count after the crop
__device__ inline uint32_t points_of(const RegHead &H, const RegTab &T)
{
	const uint32_t n = H.n[T.cloud & 1u];
	return n < T.n_cap ? n : T.n_cap;
}
// a point's cell coordinate by the table's rule; *ok = 0 when it does not fit the packed key
__device__ inline int32_t table_coord(const RegTab &T, float x, int *ok)
{
	return T.rule == REG_COORD_VOXEL ? gicp::voxel_coord(x, T.resolution, ok) : pcl_icp::cell_coord(x, T.inv_edge, ok);
}
__device__ inline bool cell_in_range(int32_t x, int32_t y, int32_t z)
{
	return x >= -1048576 && y >= -1048576 && z >= -1048576 && x < 1048576 && y < 1048576 && z < 1048576;
}
// the slot of a key, or NO_SLOT
__device__ inline uint32_t find_slot(const uint64_t *__restrict__ keys, uint64_t key, uint32_t slots, uint32_t shift)
{
	uint32_t h = gicp::home_slot(key, shift);
	for (uint32_t probe = 0; probe < slots; probe++)
	{
		const uint64_t k = keys[h];
		if (k == key)
			return h;
		if (k == EMPTY)
			return NO_SLOT;
		h = (h + 1u) & (slots - 1u);
	}
	return NO_SLOT;
}
// the slot of a key, claimed by compare-and-swap where no point had it yet (NO_SLOT: the table is full, which a table of two slots a point never is)
__device__ inline uint32_t claim_slot(unsigned long long *keys, uint64_t key, uint32_t slots, uint32_t shift)
{
	uint32_t h = gicp::home_slot(key, shift);
	for (uint32_t probe = 0; probe < slots; probe++)
	{
		const unsigned long long was = atomicCAS(&keys[h], (unsigned long long)EMPTY, (unsigned long long)key);
		if (was == EMPTY || was == key)
			return h;
		h = (h + 1u) & (slots - 1u);
	}
	return NO_SLOT;
}
// The cells l0 .. l1 - 1 of the 27 around (cx, cy, cz), cell l = 9 (dz + 1) + 3 (dy + 1) + (dx + 1), so x runs fastest: f(l, slot) for every one
// that is in range and occupied.
template <typename F>
__device__ __forceinline__ void visit_cells(const uint64_t *__restrict__ keys, uint32_t slots, uint32_t shift, int32_t cx, int32_t cy, int32_t cz, int l0, int l1, F f)
{
	for (int l = l0; l < l1; l++)
	{
		const int32_t nx = cx + (l % 3 - 1), ny = cy + (l / 3 % 3 - 1), nz = cz + (l / 9 - 1);
		if (!cell_in_range(nx, ny, nz))
			continue;
		const uint32_t slot = find_slot(keys, gicp::pack_coords(nx, ny, nz), slots, shift);
		if (slot != NO_SLOT)
			f(l, slot);
	}
}
// point i into its slot's list, at the slot's start plus its arrival's turn: -> the position, NO_SLOT for a point without a slot
__device__ inline uint32_t list_point(const uint32_t *__restrict__ cell, const uint32_t *__restrict__ start, uint32_t *fill, uint32_t *list, uint32_t slots, uint32_t cap,
									  uint32_t i)
{
	const uint32_t slot = cell[i];
	if (slot >= slots)
		return NO_SLOT;
	const uint32_t pos = start[slot] + atomicAdd(&fill[slot], 1u);
	if (pos >= cap)
		return NO_SLOT;
	list[pos] = i;
	return pos;
}
// a slot's list ascending (a shell sort: the indices are distinct, so the order does not depend on how they arrived)
__device__ inline void sort_list(uint32_t *L, uint32_t n)
{
	const uint32_t gaps[9] = {1750u, 701u, 301u, 132u, 57u, 23u, 10u, 4u, 1u};
	for (int gi = 0; gi < 9; gi++)
	{
		const uint32_t gap = gaps[gi];
		for (uint32_t i = gap; i < n; i++)
		{
			const uint32_t v = L[i];
			uint32_t k = i;
			for (; k >= gap && L[k - gap] > v; k -= gap)
				L[k] = L[k - gap];
			L[k] = v;
		}
	}
}
// start[slot]: the exclusive sum of the counts, by a workgroup of MULLS_REG_SEG threads; -> the number of occupied slots (thread 0 only)
__device__ inline uint32_t scan_counts(const uint32_t *__restrict__ count, uint32_t *start, uint32_t slots, uint32_t *s_cnt, uint32_t *s_occ)
{
	const uint32_t t = threadIdx.x, seg = slots / MULLS_REG_SEG, b = t * seg;
	uint32_t sum = 0, occ = 0, cells = 0;
	for (uint32_t k = 0; k < seg; k++)
		sum += count[b + k], occ += count[b + k] ? 1u : 0u;
	s_cnt[t] = sum, s_occ[t] = occ;
	__syncthreads();
	if (t == 0)
	{
		uint32_t run = 0;
		for (uint32_t k = 0; k < MULLS_REG_SEG; k++)
		{
			const uint32_t v = s_cnt[k];
			s_cnt[k] = run;
			run += v;
			cells += s_occ[k];
		}
	}
	__syncthreads();
	uint32_t run = s_cnt[t];
	for (uint32_t k = 0; k < seg; k++)
	{
		start[b + k] = run;
		run += count[b + k];
	}
	return cells;
}

// ---- the sums ----
// the pairwise tree over MULLS_NDT_TREE partials held as r[16] per thread of a 256-thread workgroup (r[m] = partial[t + 256 m]); the sum in every thread
__device__ inline double tree_of_partials(double *r, double *s_p)
{
	const uint32_t t = threadIdx.x;
#pragma unroll
	for (int h = 8; h >= 1; h >>= 1) // the levels w = 2048 .. 256: partner l + w of l = t + 256 m is held by the same thread
#pragma unroll
		for (int m = 0; m < h; m++)
			r[m] += r[m + h];
	__syncthreads();
	s_p[t] = r[0];
	__syncthreads();
	for (uint32_t w = 128; w >= 1; w >>= 1)
	{
		if (t < w)
			s_p[t] += s_p[t + w];
		__syncthreads();
	}
	return s_p[0];
}
// s_sum[k], k < K: the tree over row k of the strided partials where use(k) (the same answer in every thread), 0 elsewhere; readable by every thread after
template <typename Use>
__device__ __forceinline__ void tree_of_sums(const double *__restrict__ partial, int K, Use use, double *s_p, double *s_sum)
{
	const uint32_t t = threadIdx.x;
	for (int k = 0; k < K; k++)
	{
		double v = 0.0;
		if (use(k))
		{
			double r[16];
#pragma unroll
			for (int m = 0; m < 16; m++)
				r[m] = partial[(uint32_t)k * MULLS_NDT_TREE + t + 256u * m];
			v = tree_of_partials(r, s_p);
		}
		if (t == 0)
			s_sum[k] = v;
	}
	__syncthreads();
}
// a 256-thread workgroup's sum of one count a thread; the sum in every thread
__device__ inline uint32_t sum_of_counts(uint32_t h, uint32_t *s_hits)
{
	const uint32_t t = threadIdx.x;
	__syncthreads();
	s_hits[t] = h;
	__syncthreads();
	for (uint32_t w = 128; w >= 1; w >>= 1)
	{
		if (t < w)
			s_hits[t] += s_hits[t + w];
		__syncthreads();
	}
	return s_hits[0];
}
// the lanes' counts of hits (MULLS_NDT_TREE of them) added up
__device__ inline uint32_t hits_of(const uint32_t *__restrict__ hits, uint32_t *s_hits)
{
	uint32_t h = 0;
	for (int m = 0; m < 16; m++)
		h += hits[threadIdx.x + 256u * m];
	return sum_of_counts(h, s_hits);
}
} // namespace
