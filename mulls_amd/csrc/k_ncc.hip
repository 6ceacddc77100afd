// k_ncc.hip — key-point descriptor matching: CRegistration<PointT>::find_feature_correspondence_ncc (cregistration.hpp:409-601) for gfx950.
//
// The reference fills an Nt x Ns table of L1 distances between 11-float "neighbourhood category context" descriptors and then reads it three ways: row minima
// (nearest neighbour), column minima (the reciprocal test), or its corr_num smallest entries (a sort of all Nt * Ns).  Here the table is never stored.  One
// lane owns one row point, its descriptor in registers; the column descriptors are the same for every lane of a wave at the same time, so they come
// through the scalar cache into SGPRs (no LDS, no vector loads in the loop) and an entry costs its 22 VALU operations and nothing else.  d(i, j) is
// recomputed by the same eleven float additions in k order in every pass and with either cloud as the rows (|a - b| == |b - a| bit for bit), which is what lets
// the passes agree on equal distances.  Built with -ffp-contract=off like the rest of the library (there is no multiply in the distance anyway).
#include "ncc_device.h"

namespace
{
__global__ __launch_bounds__(1024) void k_ncc_minmax(NccCloudIn tgt, float *mm) { ncc_minmax_fold(tgt, mm); }

__global__ __launch_bounds__(256) void k_ncc_desc(NccCloudIn tgt, NccCloudIn src, const float *__restrict__ mm, float4 *desc_t, float4 *desc_s,
												  unsigned long long *rowkey, unsigned long long *colkey)
{
	const uint32_t g = blockIdx.x * 256u + threadIdx.x;
	if (g >= tgt.n + src.n)
		return;
	ncc_describe(tgt, src, mm, desc_t, desc_s, rowkey, colkey, g);
}

// The table passes.  blockIdx.x: block of NCC_ROWS rows, blockIdx.y: chunk of `chunk` columns (ncc_device.h has the bodies).
__global__ __launch_bounds__(NCC_ROWS) void k_ncc_rowmin(const float4 *__restrict__ rows, uint32_t n_rows, const float4 *__restrict__ cols, uint32_t n_cols,
														 uint32_t chunk, unsigned long long *key)
{
	ncc_rowmin_at(rows, n_rows, cols, n_cols, blockIdx.x, blockIdx.y * chunk, chunk, key);
}

__global__ __launch_bounds__(1024) void k_ncc_recip(const unsigned long long *__restrict__ rowkey, const unsigned long long *__restrict__ colkey, uint32_t n_t,
													int reciprocal, uint32_t *out)
{
	ncc_recip_compact(rowkey, colkey, n_t, reciprocal, out);
}

template <uint32_t LEVEL>
__global__ __launch_bounds__(NCC_ROWS) void k_ncc_hist(const float4 *__restrict__ desc_t, uint32_t n_t, const float4 *__restrict__ desc_s, uint32_t n_s,
													   uint32_t chunk, const NccSel *__restrict__ sel, uint32_t *hist)
{
	ncc_hist_at<LEVEL>(desc_t, n_t, desc_s, n_s, blockIdx.x, blockIdx.y * chunk, chunk, sel, hist);
}

__global__ __launch_bounds__(256) void k_ncc_pick(uint32_t level, uint32_t K, NccSel *sel, const uint32_t *__restrict__ hist) { ncc_pick_bucket(level, K, sel, hist); }

__global__ __launch_bounds__(NCC_ROWS) void k_ncc_collect(const float4 *__restrict__ desc_t, uint32_t n_t, const float4 *__restrict__ desc_s, uint32_t n_s,
														  uint32_t chunk, uint32_t K, const NccSel *__restrict__ sel, unsigned long long *cand)
{
	ncc_collect_at(desc_t, n_t, desc_s, n_s, blockIdx.x, blockIdx.y * chunk, chunk, K, sel, cand);
}

// the column range of a table pass: about NCC_WGS workgroups, chunks of at least 32 columns
uint32_t ncc_chunk(uint32_t n_rows, uint32_t n_cols)
{
	const uint32_t rb = (n_rows + NCC_ROWS - 1u) / NCC_ROWS;
	uint32_t splits = NCC_WGS / rb;
	splits = splits < 1u ? 1u : splits;
	uint32_t chunk = (n_cols + splits - 1u) / splits;
	chunk = chunk < 32u ? 32u : chunk;
	while ((n_cols + chunk - 1u) / chunk > 65535u) // gridDim.y
		chunk *= 2u;
	return chunk;
}
dim3 ncc_grid(uint32_t n_rows, uint32_t n_cols, uint32_t chunk) { return dim3((n_rows + NCC_ROWS - 1u) / NCC_ROWS, (n_cols + chunk - 1u) / chunk); }
} // namespace

hipError_t launch_ncc_minmax(hipStream_t st, NccCloudIn tgt, float *mm)
{
	hipLaunchKernelGGL(k_ncc_minmax, dim3(1), dim3(1024), 0, st, tgt, mm);
	return hipGetLastError();
}

hipError_t launch_ncc_desc(hipStream_t st, NccCloudIn tgt, NccCloudIn src, const float *mm, float4 *desc_t, float4 *desc_s, unsigned long long *rowkey,
						   unsigned long long *colkey)
{
	hipLaunchKernelGGL(k_ncc_desc, dim3((tgt.n + src.n + 255u) / 256u), dim3(256), 0, st, tgt, src, mm, desc_t, desc_s, rowkey, colkey);
	return hipGetLastError();
}

hipError_t launch_ncc_rowmin(hipStream_t st, const float4 *rows, uint32_t n_rows, const float4 *cols, uint32_t n_cols, unsigned long long *key)
{
	const uint32_t chunk = ncc_chunk(n_rows, n_cols);
	hipLaunchKernelGGL(k_ncc_rowmin, ncc_grid(n_rows, n_cols, chunk), dim3(NCC_ROWS), 0, st, rows, n_rows, cols, n_cols, chunk, key);
	return hipGetLastError();
}

hipError_t launch_ncc_recip(hipStream_t st, const unsigned long long *rowkey, const unsigned long long *colkey, uint32_t n_t, int reciprocal, uint32_t *out)
{
	hipLaunchKernelGGL(k_ncc_recip, dim3(1), dim3(1024), 0, st, rowkey, colkey, n_t, reciprocal, out);
	return hipGetLastError();
}

hipError_t launch_ncc_select(hipStream_t st, const float4 *desc_t, uint32_t n_t, const float4 *desc_s, uint32_t n_s, uint32_t K, NccSel *sel, uint32_t *hist,
							 unsigned long long *cand)
{
	const uint32_t chunk = ncc_chunk(n_t, n_s);
	const dim3 grid = ncc_grid(n_t, n_s, chunk);
	typedef void (*HistKernel)(const float4 *, uint32_t, const float4 *, uint32_t, uint32_t, const NccSel *, uint32_t *);
	static const HistKernel hist_level[MULLS_NCC_HIST_LEVELS] = {k_ncc_hist<0u>, k_ncc_hist<1u>, k_ncc_hist<2u>, k_ncc_hist<3u>, k_ncc_hist<4u>, k_ncc_hist<5u>};
	for (uint32_t level = 0; level < MULLS_NCC_HIST_LEVELS; level++)
	{
		hipLaunchKernelGGL(hist_level[level], grid, dim3(NCC_ROWS), 0, st, desc_t, n_t, desc_s, n_s, chunk, sel, hist);
		hipLaunchKernelGGL(k_ncc_pick, dim3(1), dim3(256), 0, st, level, K, sel, hist);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess)
			return e;
	}
	hipLaunchKernelGGL(k_ncc_collect, grid, dim3(NCC_ROWS), 0, st, desc_t, n_t, desc_s, n_s, chunk, K, sel, cand);
	return hipGetLastError();
}
