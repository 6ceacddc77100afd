// k_ncc_batch.hip — the kernels of mulls_ncc_correspond_batch and, as a batch of one, of mulls_ncc_correspond: every step over the problems of one
// sub-batch per launch, driven by the records of ncc_batch.h (a problem's sizes, K, column chunks, first workgroups and the offsets of its arrays in the
// arena).  The arithmetic is in ncc_device.h; a kernel here only finds which problem, row block and column range its workgroup works on.
//   single-workgroup steps (intensity range, pick, reciprocal compaction): blockIdx.x is the problem.
//   flat grids (descriptors; the table passes): a workgroup is one (problem, block of 256 key points) or one (problem, 256-row block, column chunk) and
//   never spans two problems, so every lane of a wave reads the same column descriptor and ncc_sweep_at's loads stay wave-uniform scalar loads.  The
//   problem comes from a binary search of blockIdx.x in a prefix table: uniform values only.
//   fixed-number selection, lock-step: each of the six digit levels is one histogram launch and one pick launch for all problems; a problem whose
//   NccSel record says done or none makes its workgroups return at once.  The three flat-index levels are LAUNCHED UNCONDITIONALLY: learning whether some
//   problem still needs them would take a readback in the middle of the sequence, which costs more than three launches that return at once.
// The arena comes in twice, `ro` and `rw`, the same address: what a kernel only reads (records, prefix tables, staged clouds, and the arrays earlier
// launches wrote) goes through `ro`, what it writes through `rw`.  No byte is reached through both inside one kernel, which is what lets the compiler keep
// the column descriptors in scalar loads beside the stores of the same kernel.
#include <hip/hip_runtime.h>

#include "ncc_batch.h"
#include "ncc_device.h"

namespace
{
template <typename T>
__device__ __forceinline__ T *at(unsigned char *arena, uint64_t off)
{
	return reinterpret_cast<T *>(arena + off);
}
template <typename T>
__device__ __forceinline__ const T *at(const unsigned char *arena, uint64_t off)
{
	return reinterpret_cast<const T *>(arena + off);
}

// the problem p with first[p] <= g < first[p + 1] (first[B] is the grid; every problem has a workgroup at least)
__device__ __forceinline__ uint32_t find_problem(const uint32_t *__restrict__ first, uint32_t B, uint32_t g)
{
	uint32_t lo = 0, hi = B;
	while (hi - lo > 1u)
	{
		const uint32_t mid = (lo + hi) >> 1;
		if (first[mid] <= g)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

__device__ __forceinline__ NccCloudIn cloud_in(const unsigned char *ro, uint64_t in, uint32_t ext, uint32_t n)
{
	return NccCloudIn{ext ? reinterpret_cast<const float *>(in) : at<float>(ro, in), n, ext ? 0u : 1u};
}

__global__ __launch_bounds__(1024) void k_nb_minmax(const unsigned char *__restrict__ ro, unsigned char *__restrict__ rw, uint64_t o_desc)
{
	const NccBatchDesc &D = at<NccBatchDesc>(ro, o_desc)[blockIdx.x];
	ncc_minmax_fold(cloud_in(ro, D.in_t, D.ext_t, D.n_t), at<float>(rw, D.mm));
}

__global__ __launch_bounds__(256) void k_nb_desc(const unsigned char *__restrict__ ro, unsigned char *__restrict__ rw, uint64_t o_desc, uint64_t o_first, uint32_t B,
												 int fixed)
{
	const uint32_t p = find_problem(at<uint32_t>(ro, o_first), B, blockIdx.x);
	const NccBatchDesc &D = at<NccBatchDesc>(ro, o_desc)[p];
	const uint32_t g = (blockIdx.x - D.blk) * 256u + threadIdx.x;
	if (fixed && g == 0u)
		*at<unsigned long long>(rw, D.out) = 0ull; // cand's counter
	if (g >= D.n_t + D.n_s)
		return;
	ncc_describe(cloud_in(ro, D.in_t, D.ext_t, D.n_t), cloud_in(ro, D.in_s, D.ext_s, D.n_s), at<float>(ro, D.mm), at<float4>(rw, D.desc_t), at<float4>(rw, D.desc_s),
				 at<unsigned long long>(rw, D.rowkey), at<unsigned long long>(rw, D.colkey), g);
}

// where a workgroup of a table pass works: rows x cols of problem p, row block and first column
struct Tile
{
	const NccBatchDesc *D;
	uint32_t row_block, j0, chunk;
};
__device__ __forceinline__ Tile find_tile(const unsigned char *__restrict__ ro, uint64_t o_desc, uint64_t o_first, uint32_t B, bool swapped)
{
	const uint32_t p = find_problem(at<uint32_t>(ro, o_first), B, blockIdx.x);
	const NccBatchDesc *D = at<NccBatchDesc>(ro, o_desc) + p;
	const uint32_t local = blockIdx.x - (swapped ? D->wg_swap : D->wg), rb = ((swapped ? D->n_s : D->n_t) + NCC_ROWS - 1u) / NCC_ROWS;
	const uint32_t chunk = swapped ? D->chunk_swap : D->chunk;
	return Tile{D, local % rb, (local / rb) * chunk, chunk};
}

template <bool SWAPPED>
__global__ __launch_bounds__(NCC_ROWS) void k_nb_rowmin(const unsigned char *__restrict__ ro, unsigned char *__restrict__ rw, uint64_t o_desc, uint64_t o_first,
														uint32_t B)
{
	const Tile t = find_tile(ro, o_desc, o_first, B, SWAPPED);
	const NccBatchDesc &D = *t.D;
	if constexpr (SWAPPED)
		ncc_rowmin_at(at<float4>(ro, D.desc_s), D.n_s, at<float4>(ro, D.desc_t), D.n_t, t.row_block, t.j0, t.chunk, at<unsigned long long>(rw, D.colkey));
	else
		ncc_rowmin_at(at<float4>(ro, D.desc_t), D.n_t, at<float4>(ro, D.desc_s), D.n_s, t.row_block, t.j0, t.chunk, at<unsigned long long>(rw, D.rowkey));
}

__global__ __launch_bounds__(1024) void k_nb_recip(const unsigned char *__restrict__ ro, unsigned char *__restrict__ rw, uint64_t o_desc, int reciprocal)
{
	const NccBatchDesc &D = at<NccBatchDesc>(ro, o_desc)[blockIdx.x];
	ncc_recip_compact(at<unsigned long long>(ro, D.rowkey), at<unsigned long long>(ro, D.colkey), D.n_t, reciprocal, at<uint32_t>(rw, D.out));
}

template <uint32_t LEVEL>
__global__ __launch_bounds__(NCC_ROWS) void k_nb_hist(const unsigned char *__restrict__ ro, unsigned char *__restrict__ rw, uint64_t o_desc, uint64_t o_first, uint32_t B)
{
	const Tile t = find_tile(ro, o_desc, o_first, B, false);
	const NccBatchDesc &D = *t.D;
	ncc_hist_at<LEVEL>(at<float4>(ro, D.desc_t), D.n_t, at<float4>(ro, D.desc_s), D.n_s, t.row_block, t.j0, t.chunk, at<NccSel>(ro, D.sel), at<uint32_t>(rw, D.hist));
}

__global__ __launch_bounds__(256) void k_nb_pick(const unsigned char *__restrict__ ro, unsigned char *__restrict__ rw, uint64_t o_desc, uint32_t level)
{
	const NccBatchDesc &D = at<NccBatchDesc>(ro, o_desc)[blockIdx.x];
	ncc_pick_bucket(level, D.K, at<NccSel>(rw, D.sel), at<uint32_t>(ro, D.hist));
}

__global__ __launch_bounds__(NCC_ROWS) void k_nb_collect(const unsigned char *__restrict__ ro, unsigned char *__restrict__ rw, uint64_t o_desc, uint64_t o_first, uint32_t B)
{
	const Tile t = find_tile(ro, o_desc, o_first, B, false);
	const NccBatchDesc &D = *t.D;
	ncc_collect_at(at<float4>(ro, D.desc_t), D.n_t, at<float4>(ro, D.desc_s), D.n_s, t.row_block, t.j0, t.chunk, D.K, at<NccSel>(ro, D.sel),
				   at<unsigned long long>(rw, D.out));
}
} // namespace

hipError_t launch_ncc_batch_describe(hipStream_t st, unsigned char *arena, const NccBatchLayout &L, uint32_t B, int fixed)
{
	hipLaunchKernelGGL(k_nb_minmax, dim3(B), dim3(1024), 0, st, arena, arena, L.o_desc);
	hipLaunchKernelGGL(k_nb_desc, dim3(L.blk[B]), dim3(256), 0, st, arena, arena, L.o_desc, L.o_blk, B, fixed);
	return hipGetLastError();
}

hipError_t launch_ncc_batch_rowmin(hipStream_t st, unsigned char *arena, const NccBatchLayout &L, uint32_t B, int swapped)
{
	if (swapped)
		hipLaunchKernelGGL(k_nb_rowmin<true>, dim3(L.wg_swap[B]), dim3(NCC_ROWS), 0, st, arena, arena, L.o_desc, L.o_wg_swap, B);
	else
		hipLaunchKernelGGL(k_nb_rowmin<false>, dim3(L.wg[B]), dim3(NCC_ROWS), 0, st, arena, arena, L.o_desc, L.o_wg, B);
	return hipGetLastError();
}

hipError_t launch_ncc_batch_recip(hipStream_t st, unsigned char *arena, const NccBatchLayout &L, uint32_t B, int reciprocal)
{
	hipLaunchKernelGGL(k_nb_recip, dim3(B), dim3(1024), 0, st, arena, arena, L.o_desc, reciprocal);
	return hipGetLastError();
}

hipError_t launch_ncc_batch_select(hipStream_t st, unsigned char *arena, const NccBatchLayout &L, uint32_t B)
{
	typedef void (*HistKernel)(const unsigned char *, unsigned char *, uint64_t, uint64_t, uint32_t);
	static const HistKernel hist_level[MULLS_NCC_HIST_LEVELS] = {k_nb_hist<0u>, k_nb_hist<1u>, k_nb_hist<2u>, k_nb_hist<3u>, k_nb_hist<4u>, k_nb_hist<5u>};
	for (uint32_t level = 0; level < MULLS_NCC_HIST_LEVELS; level++)
	{
		hipLaunchKernelGGL(hist_level[level], dim3(L.wg[B]), dim3(NCC_ROWS), 0, st, arena, arena, L.o_desc, L.o_wg, B);
		hipLaunchKernelGGL(k_nb_pick, dim3(B), dim3(256), 0, st, arena, arena, L.o_desc, level);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess)
			return e;
	}
	hipLaunchKernelGGL(k_nb_collect, dim3(L.wg[B]), dim3(NCC_ROWS), 0, st, arena, arena, L.o_desc, L.o_wg, B);
	return hipGetLastError();
}
