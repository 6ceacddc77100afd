// k_sor.hip — statistical outlier removal (CFilter::sor_filter, cfilter.hpp:204-247; pcl::StatisticalOutlierRemoval) for gfx950.
//   k_sor_gather    x, y, z out of a device cloud's 48-byte records
//   k_sor_bounds    bounding box (ordered-integer atomic min / max) and the non-finite flag
//   k_sor_brute     one wavefront per query over all points: admission against the running kk-th best, selection by rank counting in LDS.
//                   Answers the probes that set the cell edge and, at the end, the queries no grid level certified.
//   k_sor_cells     packed cell key per point, insertion into the hash of occupied cells, the cells' counts
//   k_sor_scatter   the points into cell order
//   k_sor_search    one lane per query: Chebyshev rings around its cell until its kk-th best is certainly nearer than anything unscanned;
//                   the k-best list lives in registers (static indices only, templated on the capacity): no scratch memory
//   k_sor_partials, k_sor_stats, k_sor_flags, k_sor_compact   the statistics in the defined order, the keep flags, the stable compaction
//   k_sor_emit      the kept records of a device cloud
//   k_sor_scan_*    exclusive scan of 32-bit counts (the cells' starts, the compaction's positions)
// Every loop's trip count is bounded by a launch argument (n, the table's slots) or a constant of sor_launch.h.  The arithmetic of the result is
// sor_math.h's, built with -ffp-contract=off: tests/sor_restated.py reproduces the bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sor_launch.h"

namespace
{
constexpr uint32_t SCAN_ITEMS = 4096u; // per block of 256 threads
constexpr uint32_t BRUTE_CAND = 512u;  // candidate buffer of a brute-force query

__device__ __forceinline__ uint32_t enc_ordered(float f)
{
	const uint32_t u = __float_as_uint(f);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t home_slot(uint64_t key, uint32_t slots) { return (uint32_t)(((mix64(key) >> 32) * (uint64_t)slots) >> 32); }
__device__ __forceinline__ uint64_t pack_key(int64_t cx, int64_t cy, int64_t cz)
{
	return (uint64_t)cx | ((uint64_t)cy << MULLS_SOR_CELL_BITS) | ((uint64_t)cz << (2 * MULLS_SOR_CELL_BITS));
}

// exclusive scan of one value per thread over a block of NW wavefronts; *total = the block's sum
template <int NW>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *wsum, uint32_t *total)
{
	const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
	uint32_t inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1)
	{
		const uint32_t o = __shfl_up(inc, d, 64);
		if (lane >= (uint32_t)d)
			inc += o;
	}
	if (lane == 63u)
		wsum[w] = inc;
	__syncthreads();
	uint32_t base = 0, all = 0;
#pragma unroll
	for (int k = 0; k < NW; k++)
	{
		const uint32_t s = wsum[k];
		base += (uint32_t)k < w ? s : 0u;
		all += s;
	}
	__syncthreads();
	*total = all;
	return base + inc - v;
}
} // namespace

__global__ void __launch_bounds__(256) k_sor_gather(const unsigned char *recs, uint32_t n, float4 *out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const float4 r = *reinterpret_cast<const float4 *>(recs + (size_t)i * 48u);
	out[i] = make_float4(r.x, r.y, r.z, __uint_as_float(i));
}

__global__ void __launch_bounds__(256) k_sor_bounds(const float4 *__restrict__ pts, uint32_t n, SorHeader *hdr)
{
	float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	uint32_t bad = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
	{
		const float4 p = pts[i];
		const float c[3] = {p.x, p.y, p.z};
#pragma unroll
		for (int a = 0; a < 3; a++)
		{
			bad |= isfinite(c[a]) ? 0u : 1u;
			lo[a] = fminf(lo[a], c[a]);
			hi[a] = fmaxf(hi[a], c[a]);
		}
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1)
	{
#pragma unroll
		for (int a = 0; a < 3; a++)
		{
			lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64));
			hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64));
		}
		bad |= __shfl_xor(bad, d, 64);
	}
	if ((threadIdx.x & 63u) == 0u)
	{
#pragma unroll
		for (int a = 0; a < 3; a++)
		{
			atomicMin(&hdr->lo_enc[a], enc_ordered(lo[a]));
			atomicMax(&hdr->hi_enc[a], enc_ordered(hi[a]));
		}
		if (bad)
			atomicOr(&hdr->bad, 1u);
	}
}

// One wavefront per query.  The lanes stream the points; a distance below the running kk-th best (everything, until there is one) is appended to the
// candidate buffer; a buffer that could overflow on the next step is pruned to its kk smallest by rank counting, ties broken by position, so that
// the ranks are a permutation.  Only the multiset of the kk smallest values leaves the kernel.
__global__ void __launch_bounds__(64) k_sor_brute(const float4 *__restrict__ pts, uint32_t n, uint32_t step, const uint32_t *__restrict__ qidx, int kk,
												   float *__restrict__ dist, float *__restrict__ kth)
{
	__shared__ float cand[BRUTE_CAND];
	__shared__ float sel[MULLS_SOR_MAX_K + 1];
	const uint32_t lane = threadIdx.x, qi = qidx[blockIdx.x];
	const float4 q = pts[qi];
	uint32_t c = 0;
	float thr = INFINITY;
	auto prune = [&]() {
		__syncthreads();
		for (uint32_t j = lane; j < c; j += 64u) // (c <= BRUTE_CAND)
		{
			const float dj = cand[j];
			uint32_t rank = 0;
			for (uint32_t u = 0; u < c; u++)
			{
				const float du = cand[u];
				rank += (du < dj || (du == dj && u < j)) ? 1u : 0u;
			}
			if (rank < (uint32_t)kk)
				sel[rank] = dj;
		}
		__syncthreads();
		c = c < (uint32_t)kk ? c : (uint32_t)kk;
		for (uint32_t j = lane; j < c; j += 64u)
			cand[j] = sel[j];
		thr = c == (uint32_t)kk ? sel[kk - 1] : INFINITY;
		__syncthreads();
	};
	const uint32_t m = (n + step - 1u) / step; // points visited
	for (uint32_t base = 0; base < m; base += 64u)
	{
		const uint32_t k = base + lane;
		bool admit = false;
		float d = INFINITY;
		if (k < m)
		{
			const float4 p = pts[(size_t)k * step];
			d = sor_d2(p.x, p.y, p.z, q.x, q.y, q.z);
			admit = d < thr || thr == INFINITY;
		}
		const uint64_t mask = __ballot(admit);
		if (mask)
		{
			if (admit)
				cand[c + __popcll(mask & ((1ull << lane) - 1ull))] = d;
			c += (uint32_t)__popcll(mask);
			if (c > BRUTE_CAND - 64u)
				prune();
		}
	}
	prune();
	if (lane == 0u)
	{
		// (fewer than kk points visited: only a probe on a thinned cloud can see that; its radius is then unknown)
		if (kth)
			kth[blockIdx.x] = c == (uint32_t)kk ? sel[kk - 1] : INFINITY;
		if (dist && c == (uint32_t)kk)
			dist[qi] = sor_mean_dist_list(sel, kk);
	}
}

__global__ void __launch_bounds__(256) k_sor_cells(const float4 *__restrict__ pts, uint32_t n, SorGrid G, uint32_t *__restrict__ slot_of, uint32_t *counts,
													SorHeader *hdr)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const float4 p = pts[i];
	int64_t c[3] = {sor_cell(p.x, G.lo[0], G.inv_edge), sor_cell(p.y, G.lo[1], G.inv_edge), sor_cell(p.z, G.lo[2], G.inv_edge)};
	const int64_t top = ((int64_t)1 << MULLS_SOR_CELL_BITS) - 1;
	bool over = false;
#pragma unroll
	for (int a = 0; a < 3; a++)
		if (c[a] < 0 || c[a] > top) // does not fit the packed key: refused by the host, never wrapped
		{
			over = true;
			c[a] = c[a] < 0 ? 0 : top;
		}
	const uint64_t key = pack_key(c[0], c[1], c[2]);
	uint32_t h = home_slot(key, G.slots);
	bool placed = false;
	for (uint32_t probe = 0; probe < G.slots; probe++)
	{
		const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(&G.keys[h]), (unsigned long long)MULLS_SOR_EMPTY, (unsigned long long)key);
		if (old == MULLS_SOR_EMPTY || old == key)
		{
			placed = true;
			break;
		}
		h = h + 1u == G.slots ? 0u : h + 1u;
	}
	if (over || !placed)
		atomicOr(&hdr->overflow, 1u);
	if (!placed) // (a full table cannot happen with slots > 2 n; the point still gets a valid slot)
		h = 0;
	slot_of[i] = h;
	atomicAdd(&counts[h], 1u);
}

__global__ void __launch_bounds__(256) k_sor_scatter(const float4 *__restrict__ pts, uint32_t n, const uint32_t *__restrict__ slot_of,
													  const uint32_t *__restrict__ start, uint32_t *fill, float4 *__restrict__ sorted)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const uint32_t s = slot_of[i];
	const float4 p = pts[i];
	sorted[start[s] + atomicAdd(&fill[s], 1u)] = make_float4(p.x, p.y, p.z, __uint_as_float(i)); // (order inside a cell is free: only multisets matter)
}

template <int CAP>
__global__ void __launch_bounds__(256) k_sor_search(SorGrid G, const float4 *__restrict__ pts, const uint32_t *__restrict__ qidx, uint32_t nq, int kk,
													 float *__restrict__ dist, uint32_t *__restrict__ left, uint32_t *n_left)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= nq)
		return;
	float4 q;
	uint32_t orig;
	if (qidx)
	{
		orig = qidx[t];
		q = pts[orig];
	}
	else
	{
		q = G.sorted[t];
		orig = __float_as_uint(q.w);
	}
	const int64_t cx = sor_cell(q.x, G.lo[0], G.inv_edge), cy = sor_cell(q.y, G.lo[1], G.inv_edge), cz = sor_cell(q.z, G.lo[2], G.inv_edge);
	const int64_t top = ((int64_t)1 << MULLS_SOR_CELL_BITS) - 1;
	SorKBest<CAP> kb;
	kb.init(kk);
	uint32_t budget = MULLS_SOR_SCAN_BUDGET;
	bool done = false, over = false;
	for (int R = 0; R <= MULLS_SOR_MAX_RING && !over && !done; R++)
	{
		for (int dz = -R; dz <= R && !over && !done; dz++)
			for (int dy = -R; dy <= R && !over && !done; dy++)
			{
				const bool face = dz == -R || dz == R || dy == -R || dy == R;
				const int stepx = face ? 1 : 2 * R; // off the shell's faces only dx = -R and dx = R belong to ring R
				for (int dx = -R; dx <= R; dx += stepx)
				{
					const int64_t nx = cx + dx, ny = cy + dy, nz = cz + dz;
					if (nx < 0 || ny < 0 || nz < 0 || nx > top || ny > top || nz > top)
						continue;
					const uint64_t key = pack_key(nx, ny, nz);
					uint32_t h = home_slot(key, G.slots), b = 0, e = 0;
					for (uint32_t probe = 0; probe < G.slots; probe++)
					{
						const uint64_t k = G.keys[h];
						if (k == key)
						{
							b = G.start[h], e = G.start[h + 1u];
							break;
						}
						if (k == MULLS_SOR_EMPTY)
							break;
						h = h + 1u == G.slots ? 0u : h + 1u;
					}
					const uint32_t cnt = e - b, part = cnt < budget ? cnt : budget;
					budget -= part;
					for (uint32_t j = b; j < b + part; j++) // (at most MULLS_SOR_SCAN_BUDGET points on a level)
					{
						const float4 p = G.sorted[j];
						kb.insert(sor_d2(p.x, p.y, p.z, q.x, q.y, q.z));
					}
					if (part < cnt) // out of budget: the query leaves this level, unless kk coincident points have settled it already
					{
						done = kb.worst() == 0.0f;
						over = !done;
						break;
					}
				}
			}
		if (!over && !done && sor_certified(kb.worst(), R, G.edge))
			done = true;
	}
	if (done)
		dist[orig] = kb.mean_dist(kk);
	else
		left[atomicAdd(n_left, 1u)] = orig;
}

__global__ void __launch_bounds__(256) k_sor_partials(const float *__restrict__ dist, uint32_t n, double *__restrict__ partials)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // the grid is MULLS_SOR_PARTIALS threads
	sor_partial(dist, n, p, &partials[p], &partials[MULLS_SOR_PARTIALS + p]);
}

__global__ void __launch_bounds__(1024) k_sor_stats(double *partials, uint32_t n, double std_mul, SorHeader *hdr)
{
	for (uint32_t half = MULLS_SOR_PARTIALS / 2u; half > 0u; half >>= 1)
	{
		for (uint32_t p = threadIdx.x; p < half; p += 1024u)
		{
			sor_tree_step(partials, half, p);
			sor_tree_step(partials + MULLS_SOR_PARTIALS, half, p);
		}
		__threadfence_block();
		__syncthreads();
	}
	if (threadIdx.x == 0u)
	{
		double out[3];
		sor_statistics(partials[0], partials[MULLS_SOR_PARTIALS], n, std_mul, out);
		hdr->mean = out[0], hdr->stddev = out[1], hdr->threshold = out[2];
	}
}

__global__ void __launch_bounds__(256) k_sor_flags(const float *__restrict__ dist, uint32_t n, const SorHeader *__restrict__ hdr, uint32_t *__restrict__ flags)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
		flags[i] = sor_keeps(dist[i], hdr->threshold) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_sor_compact(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ pos, uint32_t n, int32_t *__restrict__ kept_idx,
													  SorHeader *hdr)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && flags[i])
		kept_idx[pos[i]] = (int32_t)i;
	if (i == 0u)
		hdr->n_kept = pos[n];
}

__global__ void __launch_bounds__(256) k_sor_emit(const float4 *__restrict__ recs, const int32_t *__restrict__ kept_idx, uint32_t n_kept, float4 *__restrict__ out)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; // one 16-byte third of a record each
	if (t >= (uint64_t)n_kept * 3u)
		return;
	const uint32_t j = (uint32_t)(t / 3u), part = (uint32_t)(t % 3u);
	out[t] = recs[(size_t)(uint32_t)kept_idx[j] * 3u + part];
}

// ---- exclusive scan: block sums, their scan in one block, the blocks' own scans on top of it
__global__ void __launch_bounds__(256) k_sor_scan_sums(const uint32_t *__restrict__ in, uint32_t m, uint32_t *__restrict__ tmp)
{
	__shared__ uint32_t wsum[4];
	const uint64_t first = (uint64_t)blockIdx.x * SCAN_ITEMS + (uint64_t)threadIdx.x * 16u;
	uint32_t s = 0;
#pragma unroll
	for (uint32_t k = 0; k < 16u; k++)
		s += first + k < m ? in[first + k] : 0u;
	uint32_t total;
	(void)block_scan<4>(s, wsum, &total);
	if (threadIdx.x == 0u)
		tmp[blockIdx.x] = total;
}
__global__ void __launch_bounds__(1024) k_sor_scan_top(uint32_t *tmp, uint32_t nb)
{
	__shared__ uint32_t wsum[16];
	const uint32_t per = (nb + 1023u) / 1024u, first = threadIdx.x * per;
	uint32_t s = 0;
	for (uint32_t k = 0; k < per; k++)
		s += first + k < nb ? tmp[first + k] : 0u;
	uint32_t total;
	uint32_t run = block_scan<16>(s, wsum, &total);
	for (uint32_t k = 0; k < per; k++)
		if (first + k < nb)
		{
			const uint32_t v = tmp[first + k];
			tmp[first + k] = run;
			run += v;
		}
	if (threadIdx.x == 0u)
		tmp[nb] = total;
}
__global__ void __launch_bounds__(256) k_sor_scan_down(const uint32_t *__restrict__ in, uint32_t m, const uint32_t *__restrict__ tmp, uint32_t nb,
														uint32_t *__restrict__ out)
{
	__shared__ uint32_t wsum[4];
	const uint64_t first = (uint64_t)blockIdx.x * SCAN_ITEMS + (uint64_t)threadIdx.x * 16u;
	uint32_t v[16], s = 0;
#pragma unroll
	for (uint32_t k = 0; k < 16u; k++)
	{
		v[k] = first + k < m ? in[first + k] : 0u;
		s += v[k];
	}
	uint32_t total;
	uint32_t run = tmp[blockIdx.x] + block_scan<4>(s, wsum, &total);
#pragma unroll
	for (uint32_t k = 0; k < 16u; k++)
	{
		if (first + k < m)
			out[first + k] = run;
		run += v[k];
	}
	if (blockIdx.x == 0u && threadIdx.x == 0u)
		out[m] = tmp[nb];
}

// ---------------------------------------------------------------------------------------------------------------------------------------- launchers
namespace
{
inline uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1u) / per); }
} // namespace

hipError_t launch_sor_gather(hipStream_t st, const void *recs, uint32_t n, float4 *out)
{
	hipLaunchKernelGGL(k_sor_gather, dim3(blocks_of(n, 256)), dim3(256), 0, st, static_cast<const unsigned char *>(recs), n, out);
	return hipGetLastError();
}

hipError_t launch_sor_bounds(hipStream_t st, const float4 *pts, uint32_t n, SorHeader *hdr)
{
	hipError_t e = hipMemsetAsync(hdr, 0, sizeof(SorHeader), st);
	if (e != hipSuccess)
		return e;
	e = hipMemsetAsync(hdr->lo_enc, 0xff, sizeof(hdr->lo_enc), st);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(k_sor_bounds, dim3(std::min(blocks_of(n, 256), 1024u)), dim3(256), 0, st, pts, n, hdr);
	return hipGetLastError();
}

hipError_t launch_sor_brute(hipStream_t st, const float4 *pts, uint32_t n, uint32_t step, const uint32_t *qidx, uint32_t nq, int kk, float *dist, float *kth)
{
	if (!nq)
		return hipSuccess;
	hipLaunchKernelGGL(k_sor_brute, dim3(nq), dim3(64), 0, st, pts, n, step, qidx, kk, dist, kth);
	return hipGetLastError();
}

hipError_t launch_sor_scan(hipStream_t st, const uint32_t *in, uint32_t m, uint32_t *out, uint32_t *tmp)
{
	const uint32_t nb = blocks_of(m, SCAN_ITEMS);
	hipLaunchKernelGGL(k_sor_scan_sums, dim3(nb), dim3(256), 0, st, in, m, tmp);
	hipLaunchKernelGGL(k_sor_scan_top, dim3(1), dim3(1024), 0, st, tmp, nb);
	hipLaunchKernelGGL(k_sor_scan_down, dim3(nb), dim3(256), 0, st, in, m, tmp, nb, out);
	return hipGetLastError();
}

hipError_t launch_sor_build(hipStream_t st, const float4 *pts, uint32_t n, SorGrid G, float4 *sorted, uint32_t *slot_of, uint32_t *counts, uint32_t *scan_tmp,
							SorHeader *hdr)
{
	hipError_t e = hipMemsetAsync(G.keys, 0xff, (size_t)G.slots * sizeof(uint64_t), st);
	if (e != hipSuccess)
		return e;
	e = hipMemsetAsync(counts, 0, (size_t)G.slots * sizeof(uint32_t), st);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(k_sor_cells, dim3(blocks_of(n, 256)), dim3(256), 0, st, pts, n, G, slot_of, counts, hdr);
	e = launch_sor_scan(st, counts, G.slots, G.start, scan_tmp);
	if (e != hipSuccess)
		return e;
	e = hipMemsetAsync(counts, 0, (size_t)G.slots * sizeof(uint32_t), st);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(k_sor_scatter, dim3(blocks_of(n, 256)), dim3(256), 0, st, pts, n, slot_of, G.start, counts, sorted);
	return hipGetLastError();
}

hipError_t launch_sor_search(hipStream_t st, SorGrid G, const float4 *pts, const uint32_t *qidx, uint32_t nq, int kk, float *dist, uint32_t *left, uint32_t *n_left)
{
	if (!nq)
		return hipSuccess;
	const dim3 grid(blocks_of(nq, 256)), block(256);
	if (kk <= 9)
		hipLaunchKernelGGL(k_sor_search<9>, grid, block, 0, st, G, pts, qidx, nq, kk, dist, left, n_left);
	else if (kk <= 17)
		hipLaunchKernelGGL(k_sor_search<17>, grid, block, 0, st, G, pts, qidx, nq, kk, dist, left, n_left);
	else if (kk <= 33)
		hipLaunchKernelGGL(k_sor_search<33>, grid, block, 0, st, G, pts, qidx, nq, kk, dist, left, n_left);
	else
		hipLaunchKernelGGL(k_sor_search<MULLS_SOR_MAX_K + 1>, grid, block, 0, st, G, pts, qidx, nq, kk, dist, left, n_left);
	return hipGetLastError();
}

hipError_t launch_sor_finish(hipStream_t st, const float *dist, uint32_t n, double std_mul, double *partials, uint32_t *flags, uint32_t *pos, uint32_t *scan_tmp,
							 int32_t *kept_idx, SorHeader *hdr)
{
	hipLaunchKernelGGL(k_sor_partials, dim3(MULLS_SOR_PARTIALS / 256u), dim3(256), 0, st, dist, n, partials);
	hipLaunchKernelGGL(k_sor_stats, dim3(1), dim3(1024), 0, st, partials, n, std_mul, hdr);
	hipLaunchKernelGGL(k_sor_flags, dim3(blocks_of(n, 256)), dim3(256), 0, st, dist, n, hdr, flags);
	hipError_t e = launch_sor_scan(st, flags, n, pos, scan_tmp);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(k_sor_compact, dim3(blocks_of(n, 256)), dim3(256), 0, st, flags, pos, n, kept_idx, hdr);
	return hipGetLastError();
}

hipError_t launch_sor_emit(hipStream_t st, const void *recs, const int32_t *kept_idx, uint32_t n_kept, void *out)
{
	if (!n_kept)
		return hipSuccess;
	hipLaunchKernelGGL(k_sor_emit, dim3(blocks_of((uint64_t)n_kept * 3u, 256)), dim3(256), 0, st, static_cast<const float4 *>(recs), kept_idx, n_kept,
					   static_cast<float4 *>(out));
	return hipGetLastError();
}
