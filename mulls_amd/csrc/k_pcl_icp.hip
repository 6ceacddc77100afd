// k_pcl_icp.hip — the device side of mulls_pcl_icp / mulls_pcl_icp_batch (gfx950).  One launch of each kernel serves every problem of a sub-batch:
// blockIdx.y is the problem for the per-point, per-slot and per-cell kernels, blockIdx.x for those that give a problem one workgroup.  The crop and the
// nearest-neighbour pass of the fitness are k_ndt.hip's.  Setup: hash tables of occupied cells (k_pcl_icp_cells, k_pcl_icp_offsets, k_pcl_icp_scatter,
// as k_gicp.hip's, with the coordinates copied into cell order) and, for Point2Plane, the normals: every cell's list sorted (k_pcl_icp_sort), then one
// workgroup per cell that merges its 27 lists through LDS tiles in ascending index (k_pcl_icp_normals).  A tick: the moved source re-binned when the
// correspondences are reciprocal, k_pcl_icp_search (the hot path: the exact nearest target point within the distance, 27 cells, ties by index),
// k_pcl_icp_recip, k_pcl_icp_accum (and k_pcl_icp_cross for Point2Point: the centroids come first) into strided partials, k_pcl_icp_decide (the tree,
// pcl_icp_math.h's step and stop rules on one lane, then the source moved by the whole workgroup).  Atomics place entries and count; they never decide
// an order of additions.  No kernel waits for another workgroup.  Every loop is bounded by a descriptor field, a launch argument or a constant.
#include <hip/hip_runtime.h>

#include "ndt_tree.h"
#include "pcl_icp_launch.h"

namespace
{
template <typename T>
__device__ inline T *at(unsigned char *arena, uint64_t off)
{
	return reinterpret_cast<T *>(arena + off);
}
constexpr uint64_t EMPTY = 0xffffffffffffffffull;
constexpr uint32_t NO_SLOT = 0xffffffffu, NO_POINT = 0xffffffffu;
constexpr uint32_t TILE = MULLS_PCL_ICP_TILE;

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
__device__ inline bool cell_in_range(int32_t x, int32_t y, int32_t z)
{
	return x >= -1048576 && y >= -1048576 && z >= -1048576 && x < 1048576 && y < 1048576 && z < 1048576;
}
// a table's points: the source for PCL_ICP_TAB_SRC, the target for the others
__device__ inline uint32_t points_of(const PclIcpRec &R, const PclIcpTab &T, int tb)
{
	const uint32_t n = R.n[tb == PCL_ICP_TAB_SRC ? 0 : 1];
	return n < T.n_cap ? n : T.n_cap;
}
// does a table take part in this launch?  The source's is rebuilt while the problem runs
__device__ inline bool table_live(const PclIcpRec &R, const PclIcpTab &T, int tb)
{
	return R.status == PCL_ICP_ST_OK && T.n_cap != 0 && (tb != PCL_ICP_TAB_SRC || (R.S.running && !R.range));
}

__global__ void __launch_bounds__(64) k_pcl_icp_begin(const NdtRec *__restrict__ nrec, PclIcpRec *rec, double *frames, uint32_t P)
{
	const uint32_t p = blockIdx.x * 64u + threadIdx.x;
	if (p >= P)
		return;
	PclIcpRec &R = rec[p]; // (zeroed by the host: range is only ever set)
	R.n[0] = nrec[p].n_src, R.n[1] = nrec[p].n_tgt;
	R.n_fit = 0, R.fitness = 0.0, R.pad = 0;
	int status = PCL_ICP_ST_OK;
	if (nrec[p].status == NDT_ST_NONFINITE)
		status = PCL_ICP_ST_NONFINITE;
	else if (nrec[p].status != NDT_ST_OK || R.n[0] == 0 || R.n[1] == 0)
		status = PCL_ICP_ST_EMPTY;
	R.status = status;
	pcl_icp::State S;
	pcl_icp::begin(S);
	if (status != PCL_ICP_ST_OK)
		S.running = 0;
	R.S = S;
	for (int k = 0; k < 9; k++)
		frames[12u * p + k] = S.R[k];
	for (int k = 0; k < 3; k++)
		frames[12u * p + 9 + k] = S.t[k];
}

// the moved source starts as the cropped source; a source point outside the cells' range refuses the problem
__global__ void __launch_bounds__(256) k_pcl_icp_copy(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec)
{
	const uint32_t p = blockIdx.y;
	PclIcpRec &R = rec[p];
	if (R.status != PCL_ICP_ST_OK)
		return;
	const PclIcpDesc &D = desc[p];
	const uint32_t ns = R.n[0] < D.n_src_cap ? R.n[0] : D.n_src_cap;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ns)
		return;
	const float *S3 = at<const float>(arena, D.o_src);
	float *M3 = at<float>(arena, D.o_mov);
	const float x = S3[3 * i], y = S3[3 * i + 1], z = S3[3 * i + 2];
	M3[3 * i] = x, M3[3 * i + 1] = y, M3[3 * i + 2] = z;
	int ok = 1;
	const double inv = opt.inv_edge[PCL_ICP_TAB_TGT];
	(void)pcl_icp::cell_coord(x, inv, &ok), (void)pcl_icp::cell_coord(y, inv, &ok), (void)pcl_icp::cell_coord(z, inv, &ok);
	if (!ok)
		atomicOr(&R.range, 1u);
}

__global__ void __launch_bounds__(256) k_pcl_icp_clear(const PclIcpDesc *__restrict__ desc, unsigned char *arena, const PclIcpRec *__restrict__ rec, int tb)
{
	const uint32_t p = blockIdx.y;
	const PclIcpTab T = desc[p].tab[tb];
	if (!table_live(rec[p], T, tb))
		return;
	const uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s >= T.slots)
		return;
	at<uint64_t>(arena, T.o_keys)[s] = EMPTY;
	at<uint32_t>(arena, T.o_count)[s] = 0u, at<uint32_t>(arena, T.o_start)[s] = 0u, at<uint32_t>(arena, T.o_fill)[s] = 0u;
}

// every point of a table's cloud: its cell, the cell's slot (claimed by compare-and-swap), the slot's count
__global__ void __launch_bounds__(256) k_pcl_icp_cells(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec, int tb)
{
	const uint32_t p = blockIdx.y;
	PclIcpRec &R = rec[p];
	const PclIcpTab T = desc[p].tab[tb];
	if (!table_live(R, T, tb))
		return;
	const uint32_t n = points_of(R, T, tb);
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n)
		return;
	const float *P3 = at<const float>(arena, T.o_pts);
	const double inv = opt.inv_edge[tb];
	int ok = 1;
	const int32_t c0 = pcl_icp::cell_coord(P3[3 * i], inv, &ok), c1 = pcl_icp::cell_coord(P3[3 * i + 1], inv, &ok), c2 = pcl_icp::cell_coord(P3[3 * i + 2], inv, &ok);
	uint32_t found = NO_SLOT;
	if (ok)
	{
		const uint64_t key = gicp::pack_coords(c0, c1, c2);
		unsigned long long *keys = at<unsigned long long>(arena, T.o_keys);
		uint32_t h = gicp::home_slot(key, T.shift);
		for (uint32_t probe = 0; probe < T.slots; probe++)
		{
			const unsigned long long was = atomicCAS(&keys[h], (unsigned long long)EMPTY, (unsigned long long)key);
			if (was == EMPTY || was == key)
			{
				found = h;
				break;
			}
			h = (h + 1u) & (T.slots - 1u);
		}
	}
	else if (tb != PCL_ICP_TAB_SRC)
		atomicOr(&R.range, 1u); // a target point that does not fit the packed key: refused by the host.  A moved source point that does not takes no part.
	at<uint32_t>(arena, T.o_cell)[i] = found;
	if (found != NO_SLOT)
		atomicAdd(&at<uint32_t>(arena, T.o_count)[found], 1u);
}

// start[slot]: the exclusive sum of the counts
__global__ void __launch_bounds__(MULLS_PCL_ICP_SEG) k_pcl_icp_offsets(const PclIcpDesc *__restrict__ desc, unsigned char *arena, const PclIcpRec *__restrict__ rec, int tb)
{
	__shared__ uint32_t s_cnt[MULLS_PCL_ICP_SEG];
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	const PclIcpTab T = desc[p].tab[tb];
	if (!table_live(rec[p], T, tb))
		return;
	const uint32_t *count = at<const uint32_t>(arena, T.o_count);
	uint32_t *start = at<uint32_t>(arena, T.o_start);
	const uint32_t seg = T.slots / MULLS_PCL_ICP_SEG, b = t * seg;
	uint32_t sum = 0;
	for (uint32_t k = 0; k < seg; k++)
		sum += count[b + k];
	s_cnt[t] = sum;
	__syncthreads();
	if (t == 0)
	{
		uint32_t run = 0;
		for (uint32_t k = 0; k < MULLS_PCL_ICP_SEG; k++)
		{
			const uint32_t v = s_cnt[k];
			s_cnt[k] = run;
			run += v;
		}
	}
	__syncthreads();
	uint32_t run = s_cnt[t];
	for (uint32_t k = 0; k < seg; k++)
	{
		start[b + k] = run;
		run += count[b + k];
	}
}

__global__ void __launch_bounds__(256) k_pcl_icp_scatter(const PclIcpDesc *__restrict__ desc, unsigned char *arena, const PclIcpRec *__restrict__ rec, int tb)
{
	const uint32_t p = blockIdx.y;
	const PclIcpRec &R = rec[p];
	const PclIcpTab T = desc[p].tab[tb];
	if (!table_live(R, T, tb))
		return;
	const uint32_t n = points_of(R, T, tb);
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n)
		return;
	const uint32_t slot = at<const uint32_t>(arena, T.o_cell)[i];
	if (slot >= T.slots)
		return;
	const uint32_t pos = at<const uint32_t>(arena, T.o_start)[slot] + atomicAdd(&at<uint32_t>(arena, T.o_fill)[slot], 1u);
	if (pos >= T.n_cap)
		return;
	const float *P3 = at<const float>(arena, T.o_pts);
	float *Q3 = at<float>(arena, T.o_sorted);
	at<uint32_t>(arena, T.o_list)[pos] = i;
	Q3[3 * pos] = P3[3 * i], Q3[3 * pos + 1] = P3[3 * i + 1], Q3[3 * pos + 2] = P3[3 * i + 2];
}

// one lane per occupied slot of the normals' table: its points' indices ascending (a shell sort: the indices are distinct, so the order does not
// depend on how they arrived)
__global__ void __launch_bounds__(256) k_pcl_icp_sort(const PclIcpDesc *__restrict__ desc, unsigned char *arena, const PclIcpRec *__restrict__ rec)
{
	const uint32_t p = blockIdx.y;
	const PclIcpRec &R = rec[p];
	const PclIcpTab T = desc[p].tab[PCL_ICP_TAB_NRM];
	if (!table_live(R, T, PCL_ICP_TAB_NRM) || R.range)
		return;
	const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
	if (slot >= T.slots)
		return;
	const uint32_t n = at<const uint32_t>(arena, T.o_count)[slot];
	if (!n)
		return;
	const uint32_t first = at<const uint32_t>(arena, T.o_start)[slot];
	if (first >= T.n_cap || n > T.n_cap - first)
		return;
	uint32_t *L = at<uint32_t>(arena, T.o_list) + first;
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

// The normals.  One workgroup per occupied cell; a thread per point of the cell (256 at a time).  The neighbours of those points lie in the 27 cells
// around it, whose sorted lists are merged window by window: a window is TILE consecutive target indices, the lists' entries inside it are flagged,
// compacted in index order into an LDS tile of coordinates, and every thread walks the tile.  So a point adds its neighbours in ascending index
// whatever their number; two passes (the sum, then the scatter about the mean), then pcl_icp_math.h's normal.
__global__ void __launch_bounds__(256) k_pcl_icp_normals(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *__restrict__ rec)
{
	__shared__ uint32_t s_beg[27], s_end[27], s_cur[27], s_lo[27], s_hi[27];
	__shared__ uint32_t s_flag[TILE], s_wave[4];
	__shared__ float s_tile[TILE][3];
	const uint32_t p = blockIdx.y, slot = blockIdx.x, t = threadIdx.x;
	const PclIcpRec &R = rec[p];
	const PclIcpTab T = desc[p].tab[PCL_ICP_TAB_NRM];
	if (!table_live(R, T, PCL_ICP_TAB_NRM) || R.range || slot >= T.slots)
		return;
	const uint32_t n = points_of(R, T, PCL_ICP_TAB_NRM);
	const uint64_t *keys = at<const uint64_t>(arena, T.o_keys);
	const uint32_t *start = at<const uint32_t>(arena, T.o_start), *count = at<const uint32_t>(arena, T.o_count), *list = at<const uint32_t>(arena, T.o_list);
	const uint32_t cnt = count[slot], first = start[slot];
	if (!cnt || first >= n || cnt > n - first)
		return;
	const float *P3 = at<const float>(arena, T.o_pts);
	float *N3 = at<float>(arena, desc[p].o_nrm);
	if (t < 27u)
	{
		const uint64_t key = keys[slot];
		const int32_t cx = (int32_t)(key & 0x1fffffu) - 1048576 + ((int32_t)(t % 3u) - 1), cy = (int32_t)((key >> 21) & 0x1fffffu) - 1048576 + ((int32_t)((t / 3u) % 3u) - 1),
					  cz = (int32_t)((key >> 42) & 0x1fffffu) - 1048576 + ((int32_t)(t / 9u) - 1);
		uint32_t b = 0, e = 0;
		if (cell_in_range(cx, cy, cz))
		{
			const uint32_t s = find_slot(keys, gicp::pack_coords(cx, cy, cz), T.slots, T.shift);
			if (s != NO_SLOT && start[s] < n && count[s] <= n - start[s])
				b = start[s], e = b + count[s];
		}
		s_beg[t] = b, s_end[t] = e;
	}
	__syncthreads();
	for (uint32_t q0 = 0; q0 < cnt; q0 += 256u)
	{
		const bool have = q0 + t < cnt;
		uint32_t qi = have ? list[first + q0 + t] : 0u;
		qi = qi < n ? qi : 0u;
		const float qx = P3[3 * qi], qy = P3[3 * qi + 1], qz = P3[3 * qi + 2];
		double s[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
		uint32_t k = 0;
		for (int pass = 0; pass < 2; pass++)
		{
			if (t < 27u)
				s_cur[t] = s_beg[t];
			__syncthreads();
			for (uint32_t base = 0; base < n; base += TILE)
			{
				if (t < 27u)
				{
					// the first entry of the list at or above the window's end
					uint32_t lo = s_cur[t], hi = s_end[t];
					for (int it = 0; it < 32 && lo < hi; it++)
					{
						const uint32_t mid = lo + (hi - lo) / 2u;
						if (list[mid] < base + TILE)
							lo = mid + 1u;
						else
							hi = mid;
					}
					s_lo[t] = s_cur[t], s_hi[t] = lo, s_cur[t] = lo;
				}
				s_flag[t] = 0u;
				__syncthreads();
				uint32_t total = 0;
				for (int l = 0; l < 27; l++)
					total += s_hi[l] - s_lo[l];
				if (!total)
				{
					__syncthreads();
					continue;
				}
				for (int l = 0; l < 27; l++)
				{
					const uint32_t e = s_lo[l] + t;
					if (e < s_hi[l])
					{
						const uint32_t j = list[e];
						if (j >= base && j - base < TILE)
							s_flag[j - base] = 1u;
					}
				}
				__syncthreads();
				const bool present = s_flag[t] != 0u && base + t < n;
				const unsigned long long mask = __ballot(present);
				if ((t & 63u) == 0u)
					s_wave[t >> 6] = (uint32_t)__popcll(mask);
				__syncthreads();
				uint32_t off = 0, in_tile = 0;
				for (uint32_t w = 0; w < 4u; w++)
				{
					off += w < (t >> 6) ? s_wave[w] : 0u;
					in_tile += s_wave[w];
				}
				if (present)
				{
					const uint32_t pos = off + (uint32_t)__popcll(mask & ((1ull << (t & 63u)) - 1ull)), j = base + t;
					s_tile[pos][0] = P3[3 * j], s_tile[pos][1] = P3[3 * j + 1], s_tile[pos][2] = P3[3 * j + 2];
				}
				__syncthreads();
				for (uint32_t j = 0; j < in_tile && j < TILE; j++)
				{
					const float x = s_tile[j][0], y = s_tile[j][1], z = s_tile[j][2];
					if (!((double)pcl_icp::dist2(x, y, z, qx, qy, qz) <= opt.radius2))
						continue;
					if (pass == 0)
					{
						gicp::sum_add(s, (double)x, (double)y, (double)z);
						k++;
					}
					else
						gicp::scatter_add(S, m, (double)x, (double)y, (double)z);
				}
				__syncthreads();
			}
			if (pass == 0 && k >= 3u)
				gicp::mean_of(s, (int)k, m);
		}
		if (have)
		{
			float nv[3] = {0.577f, 0.577f, 0.577f};
			if (k >= 3u)
				pcl_icp::normal_of_scatter(S, (double)qx, (double)qy, (double)qz, nv);
			N3[3 * qi] = nv[0], N3[3 * qi + 1] = nv[1], N3[3 * qi + 2] = nv[2];
		}
	}
}

// The loop's hot path.  One lane per moved source point: the 27 cells around its own, every target point in them, the smallest by (float d2, index);
// no pair when the distance is above the threshold.
__global__ void __launch_bounds__(256) k_pcl_icp_search(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *__restrict__ rec)
{
	const uint32_t p = blockIdx.y;
	const PclIcpRec &R = rec[p];
	if (!R.S.running || R.range)
		return;
	const PclIcpDesc &D = desc[p];
	const PclIcpTab T = D.tab[PCL_ICP_TAB_TGT];
	const uint32_t ns = R.n[0] < D.n_src_cap ? R.n[0] : D.n_src_cap, nt = points_of(R, T, PCL_ICP_TAB_TGT);
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ns)
		return;
	const float *M3 = at<const float>(arena, D.o_mov), *Q3 = at<const float>(arena, T.o_sorted);
	const float qx = M3[3 * i], qy = M3[3 * i + 1], qz = M3[3 * i + 2];
	const uint64_t *keys = at<const uint64_t>(arena, T.o_keys);
	const uint32_t *start = at<const uint32_t>(arena, T.o_start), *count = at<const uint32_t>(arena, T.o_count), *list = at<const uint32_t>(arena, T.o_list);
	int ok = 1;
	const double inv = opt.inv_edge[PCL_ICP_TAB_TGT];
	const int32_t cx = pcl_icp::cell_coord(qx, inv, &ok), cy = pcl_icp::cell_coord(qy, inv, &ok), cz = pcl_icp::cell_coord(qz, inv, &ok);
	float best = __builtin_huge_valf();
	uint32_t bi = NO_POINT;
	if (ok)
		for (int dz = -1; dz <= 1; dz++)
			for (int dy = -1; dy <= 1; dy++)
				for (int dx = -1; dx <= 1; dx++)
				{
					const int32_t nx = cx + dx, ny = cy + dy, nz = cz + dz;
					if (!cell_in_range(nx, ny, nz))
						continue;
					const uint32_t slot = find_slot(keys, gicp::pack_coords(nx, ny, nz), T.slots, T.shift);
					if (slot == NO_SLOT)
						continue;
					const uint32_t b = start[slot], cnt = count[slot];
					if (b >= nt || cnt > nt - b)
						continue;
					for (uint32_t j = b; j < b + cnt; j++)
					{
						const float d2 = pcl_icp::dist2(qx, qy, qz, Q3[3 * j], Q3[3 * j + 1], Q3[3 * j + 2]);
						const uint32_t m = list[j];
						if (m < nt && pcl_icp::before(d2, m, best, bi))
							best = d2, bi = m;
					}
				}
	if (bi != NO_POINT && (double)best > opt.thr2)
		bi = NO_POINT;
	at<int32_t>(arena, D.o_match)[i] = bi == NO_POINT ? -1 : (int32_t)bi;
	at<float>(arena, D.o_d2)[i] = bi == NO_POINT ? 0.f : best;
}

// The reciprocity test.  A source point that beats i at its target point m lies within d(i, m) <= the threshold of m: the 27 cells of the moved
// source around m's cell decide it.  i keeps its pair only if no moved source point is before it by (d2 to m, index).
__global__ void __launch_bounds__(256) k_pcl_icp_recip(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *__restrict__ rec)
{
	const uint32_t p = blockIdx.y;
	const PclIcpRec &R = rec[p];
	if (!R.S.running || R.range)
		return;
	const PclIcpDesc &D = desc[p];
	const PclIcpTab T = D.tab[PCL_ICP_TAB_SRC];
	if (!T.n_cap)
		return;
	const uint32_t ns = points_of(R, T, PCL_ICP_TAB_SRC), nt = points_of(R, D.tab[PCL_ICP_TAB_TGT], PCL_ICP_TAB_TGT);
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ns)
		return;
	int32_t *match = at<int32_t>(arena, D.o_match);
	const int32_t m = match[i];
	if (m < 0 || (uint32_t)m >= nt)
		return;
	const float di = at<const float>(arena, D.o_d2)[i];
	const float *G3 = at<const float>(arena, D.tab[PCL_ICP_TAB_TGT].o_pts), *Q3 = at<const float>(arena, T.o_sorted);
	const float tx = G3[3 * m], ty = G3[3 * m + 1], tz = G3[3 * m + 2];
	const uint64_t *keys = at<const uint64_t>(arena, T.o_keys);
	const uint32_t *start = at<const uint32_t>(arena, T.o_start), *count = at<const uint32_t>(arena, T.o_count), *list = at<const uint32_t>(arena, T.o_list);
	int ok = 1;
	const double inv = opt.inv_edge[PCL_ICP_TAB_SRC];
	const int32_t cx = pcl_icp::cell_coord(tx, inv, &ok), cy = pcl_icp::cell_coord(ty, inv, &ok), cz = pcl_icp::cell_coord(tz, inv, &ok);
	bool beaten = false;
	if (ok)
		for (int dz = -1; dz <= 1; dz++)
			for (int dy = -1; dy <= 1; dy++)
				for (int dx = -1; dx <= 1; dx++)
				{
					const int32_t nx = cx + dx, ny = cy + dy, nz = cz + dz;
					if (!cell_in_range(nx, ny, nz))
						continue;
					const uint32_t slot = find_slot(keys, gicp::pack_coords(nx, ny, nz), T.slots, T.shift);
					if (slot == NO_SLOT)
						continue;
					const uint32_t b = start[slot], cnt = count[slot];
					if (b >= ns || cnt > ns - b)
						continue;
					for (uint32_t j = b; j < b + cnt; j++)
						if (pcl_icp::before(pcl_icp::dist2(Q3[3 * j], Q3[3 * j + 1], Q3[3 * j + 2], tx, ty, tz), list[j], di, i))
							beaten = true;
				}
	if (beaten)
		match[i] = -1;
}

// Lane l of the problem's MULLS_NDT_TREE lanes takes the source points l, l + MULLS_NDT_TREE, ..: a pair's terms into the lane's sums.  Point2Plane:
// all 28.  Point2Point: the sums of the paired points and of d2; the cross-covariance follows in k_pcl_icp_cross.
__global__ void __launch_bounds__(256) k_pcl_icp_accum(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *__restrict__ rec)
{
	const uint32_t p = blockIdx.y;
	const PclIcpRec &R = rec[p];
	if (!R.S.running || R.range)
		return;
	const PclIcpDesc &D = desc[p];
	const uint32_t ns = R.n[0] < D.n_src_cap ? R.n[0] : D.n_src_cap, nt = R.n[1] < D.n_tgt_cap ? R.n[1] : D.n_tgt_cap;
	const float *M3 = at<const float>(arena, D.o_mov), *G3 = at<const float>(arena, D.tab[PCL_ICP_TAB_TGT].o_pts), *N3 = at<const float>(arena, D.o_nrm);
	const int32_t *match = at<const int32_t>(arena, D.o_match);
	const float *d2 = at<const float>(arena, D.o_d2);
	const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
	double acc[pcl_icp::N_SUMS];
#pragma unroll
	for (int k = 0; k < pcl_icp::N_SUMS; k++)
		acc[k] = 0.0;
	uint32_t hits = 0;
	for (uint32_t i = lane; i < ns; i += MULLS_NDT_TREE)
	{
		const int32_t m = match[i];
		if (m < 0 || (uint32_t)m >= nt)
			continue;
		const double s[3] = {(double)M3[3 * i], (double)M3[3 * i + 1], (double)M3[3 * i + 2]};
		const double g[3] = {(double)G3[3 * m], (double)G3[3 * m + 1], (double)G3[3 * m + 2]};
		if (opt.metric == pcl_icp::POINT2PLANE)
		{
			const double nv[3] = {(double)N3[3 * m], (double)N3[3 * m + 1], (double)N3[3 * m + 2]};
			pcl_icp::plane_term(s, g, nv, acc);
		}
		else
		{
#pragma unroll
			for (int a = 0; a < 3; a++)
				acc[pcl_icp::SUM_S + a] += s[a], acc[pcl_icp::SUM_T + a] += g[a];
		}
		acc[pcl_icp::SUM_D2] += (double)d2[i];
		hits++;
	}
	double *partial = at<double>(arena, D.o_partial);
#pragma unroll
	for (int k = 0; k < pcl_icp::N_SUMS; k++)
		partial[(uint32_t)k * MULLS_NDT_TREE + lane] = acc[k];
	at<uint32_t>(arena, D.o_hits)[lane] = hits;
}

// the number of pairs: the lanes' counts added up by a 256-thread workgroup; the sum in every thread
__device__ inline uint32_t pairs_of(const uint32_t *__restrict__ hits, uint32_t *s_hits)
{
	const uint32_t t = threadIdx.x;
	uint32_t h = 0;
	for (int m = 0; m < 16; m++)
		h += hits[t + 256u * m];
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

// Point2Point's second pass.  Every workgroup takes the tree over the six sums itself (the same text as k_pcl_icp_decide's, so the same centroids),
// then its lanes add the products of the demeaned pairs.
__global__ void __launch_bounds__(256) k_pcl_icp_cross(const PclIcpDesc *__restrict__ desc, unsigned char *arena, const PclIcpRec *__restrict__ rec)
{
	__shared__ double s_p[256];
	__shared__ uint32_t s_hits[256];
	const uint32_t p = blockIdx.y, t = threadIdx.x;
	const PclIcpRec &R = rec[p];
	if (!R.S.running || R.range)
		return;
	const PclIcpDesc &D = desc[p];
	double *partial = at<double>(arena, D.o_partial);
	double c[6];
	for (int k = 0; k < 6; k++)
	{
		double r[16];
#pragma unroll
		for (int m = 0; m < 16; m++)
			r[m] = partial[(uint32_t)k * MULLS_NDT_TREE + t + 256u * m];
		c[k] = tree_of_partials(r, s_p);
	}
	const double dn = (double)pairs_of(at<const uint32_t>(arena, D.o_hits), s_hits);
	for (int k = 0; k < 6; k++)
		c[k] = c[k] / dn;
	const uint32_t ns = R.n[0] < D.n_src_cap ? R.n[0] : D.n_src_cap, nt = R.n[1] < D.n_tgt_cap ? R.n[1] : D.n_tgt_cap;
	const float *M3 = at<const float>(arena, D.o_mov), *G3 = at<const float>(arena, D.tab[PCL_ICP_TAB_TGT].o_pts);
	const int32_t *match = at<const int32_t>(arena, D.o_match);
	const uint32_t lane = blockIdx.x * 256u + t;
	double acc[9];
#pragma unroll
	for (int k = 0; k < 9; k++)
		acc[k] = 0.0;
	for (uint32_t i = lane; i < ns; i += MULLS_NDT_TREE)
	{
		const int32_t m = match[i];
		if (m < 0 || (uint32_t)m >= nt)
			continue;
		const double sd[3] = {(double)M3[3 * i] - c[0], (double)M3[3 * i + 1] - c[1], (double)M3[3 * i + 2] - c[2]};
		const double gd[3] = {(double)G3[3 * m] - c[3], (double)G3[3 * m + 1] - c[4], (double)G3[3 * m + 2] - c[5]};
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int b = 0; b < 3; b++)
				acc[3 * a + b] += sd[a] * gd[b];
	}
#pragma unroll
	for (int k = 0; k < 9; k++)
		partial[(uint32_t)(pcl_icp::SUM_H + k) * MULLS_NDT_TREE + lane] = acc[k];
}

// one workgroup per problem: the tree over the sums, pcl_icp_math.h's advance on one lane, then the stored source moved by the step
__global__ void __launch_bounds__(256) k_pcl_icp_decide(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec, double *frames,
														uint32_t *running, uint32_t *next)
{
	__shared__ double s_p[256];
	__shared__ double s_sum[pcl_icp::N_SUMS];
	__shared__ double s_step[12];
	__shared__ uint32_t s_hits[256];
	__shared__ int s_run, s_moved;
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	if (p == 0 && t == 0)
		*next = 0u; // (the next tick's count starts from 0)
	if (t == 0)
	{
		s_run = rec[p].S.running;
		if (s_run && rec[p].range)
			rec[p].S.running = 0, s_run = 0; // refused by the host
	}
	__syncthreads();
	if (!s_run)
		return;
	const PclIcpDesc &D = desc[p];
	const double *partial = at<const double>(arena, D.o_partial);
	for (int k = 0; k < pcl_icp::N_SUMS; k++)
	{
		if (opt.metric == pcl_icp::POINT2POINT && k >= pcl_icp::SUM_H + 9 && k != pcl_icp::SUM_D2)
		{
			if (t == 0)
				s_sum[k] = 0.0;
			continue;
		}
		double r[16];
#pragma unroll
		for (int m = 0; m < 16; m++)
			r[m] = partial[(uint32_t)k * MULLS_NDT_TREE + t + 256u * m];
		const double v = tree_of_partials(r, s_p);
		if (t == 0)
			s_sum[k] = v;
	}
	const uint32_t n_corr = pairs_of(at<const uint32_t>(arena, D.o_hits), s_hits);
	if (t == 0)
	{
		PclIcpRec &R = rec[p];
		pcl_icp::State S = R.S;
		pcl_icp::advance(S, opt.metric, s_sum, n_corr, opt.max_iter_num, opt.transformation_epsilon, opt.euclidean_fitness_epsilon);
		R.S = S;
		for (int k = 0; k < 9; k++)
			frames[12u * p + k] = S.R[k], s_step[k] = S.Rs[k];
		for (int k = 0; k < 3; k++)
			frames[12u * p + 9 + k] = S.t[k], s_step[9 + k] = S.ts[k];
		s_moved = S.moved && S.running; // (a stopped problem's moved source is read by nobody)
		if (S.running)
			atomicAdd(running, 1u);
	}
	__syncthreads();
	if (!s_moved)
		return;
	const uint32_t ns = rec[p].n[0] < D.n_src_cap ? rec[p].n[0] : D.n_src_cap;
	float *M3 = at<float>(arena, D.o_mov);
	for (uint32_t i = t; i < ns; i += 256u)
		pcl_icp::move_stored(s_step, s_step + 9, M3 + 3 * i);
}

// the fitness: over the source points whose nearest squared distance is within the range, the mean; the strided partials and the tree as every sum here
__global__ void __launch_bounds__(256) k_pcl_icp_fitness(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec)
{
	__shared__ double s_p[256];
	__shared__ uint32_t s_hits[256];
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	PclIcpRec &R = rec[p];
	if (R.status != PCL_ICP_ST_OK)
		return;
	const PclIcpDesc &D = desc[p];
	const uint32_t ns = R.n[0] < D.n_src_cap ? R.n[0] : D.n_src_cap;
	const float *dist = at<const float>(arena, D.o_dist);
	double r[16];
	uint32_t h = 0;
#pragma unroll
	for (int m = 0; m < 16; m++)
	{
		double a = 0.0;
		for (uint32_t i = t + 256u * m; i < ns; i += MULLS_NDT_TREE)
			if ((double)dist[i] <= opt.fit_range)
				a += (double)dist[i], h++;
		r[m] = a;
	}
	const double sum = tree_of_partials(r, s_p);
	s_hits[t] = h;
	__syncthreads();
	for (uint32_t w = 128; w >= 1; w >>= 1)
	{
		if (t < w)
			s_hits[t] += s_hits[t + w];
		__syncthreads();
	}
	if (t == 0)
	{
		R.n_fit = s_hits[0];
		R.fitness = s_hits[0] ? sum / (double)s_hits[0] : DBL_MAX;
	}
}
inline uint32_t blocks_of(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }
} // namespace

hipError_t launch_pcl_icp_begin(hipStream_t st, const PclIcpDesc *desc, uint32_t P, uint32_t n_src_max, unsigned char *arena, PclIcpOpts opt, const NdtRec *nrec,
								PclIcpRec *rec, double *frames)
{
	hipLaunchKernelGGL(k_pcl_icp_begin, dim3(blocks_of(P, 64)), dim3(64), 0, st, nrec, rec, frames, P);
	hipLaunchKernelGGL(k_pcl_icp_copy, dim3(blocks_of(n_src_max, 256), P), dim3(256), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_table(hipStream_t st, const PclIcpDesc *desc, uint32_t P, int tb, uint32_t n_max, uint32_t slots_max, bool clear, unsigned char *arena,
								PclIcpOpts opt, PclIcpRec *rec)
{
	if (clear)
		hipLaunchKernelGGL(k_pcl_icp_clear, dim3(blocks_of(slots_max, 256), P), dim3(256), 0, st, desc, arena, rec, tb);
	hipLaunchKernelGGL(k_pcl_icp_cells, dim3(blocks_of(n_max, 256), P), dim3(256), 0, st, desc, arena, opt, rec, tb);
	hipLaunchKernelGGL(k_pcl_icp_offsets, dim3(P), dim3(MULLS_PCL_ICP_SEG), 0, st, desc, arena, rec, tb);
	hipLaunchKernelGGL(k_pcl_icp_scatter, dim3(blocks_of(n_max, 256), P), dim3(256), 0, st, desc, arena, rec, tb);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_normals(hipStream_t st, const PclIcpDesc *desc, uint32_t P, uint32_t slots_max, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *rec)
{
	hipLaunchKernelGGL(k_pcl_icp_sort, dim3(blocks_of(slots_max, 256), P), dim3(256), 0, st, desc, arena, rec);
	hipLaunchKernelGGL(k_pcl_icp_normals, dim3(slots_max, P), dim3(256), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_search(hipStream_t st, const PclIcpDesc *desc, uint32_t P, uint32_t n_src_max, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *rec)
{
	const dim3 grid(blocks_of(n_src_max, 256), P), block(256);
	hipLaunchKernelGGL(k_pcl_icp_search, grid, block, 0, st, desc, arena, opt, rec);
	if (opt.reciprocal)
		hipLaunchKernelGGL(k_pcl_icp_recip, grid, block, 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_accum(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *rec)
{
	const dim3 grid(MULLS_NDT_TREE / 256u, P), block(256);
	hipLaunchKernelGGL(k_pcl_icp_accum, grid, block, 0, st, desc, arena, opt, rec);
	if (opt.metric == pcl_icp::POINT2POINT)
		hipLaunchKernelGGL(k_pcl_icp_cross, grid, block, 0, st, desc, arena, rec);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_decide(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec, double *frames,
								 uint32_t *running, uint32_t *next)
{
	hipLaunchKernelGGL(k_pcl_icp_decide, dim3(P), dim3(256), 0, st, desc, arena, opt, rec, frames, running, next);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_fitness(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec)
{
	hipLaunchKernelGGL(k_pcl_icp_fitness, dim3(P), dim3(256), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
