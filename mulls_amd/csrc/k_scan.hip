// k_scan.hip — the kernels of mulls_scan_prepare and mulls_mapper_add: the raw-scan steps of CFilter (vertical_intrinsic_calibration, dist_filter,
// random_downsample, get_pts_timestamp_ratio_in_frame), and for the mapper apply_motion_compensation and pcl::transformPointCloud behind them, over the
// frames of one sub-batch per launch.  The arithmetic is scan_math.h's (the text the CPU harness compiles); a kernel here only finds its frame and chunk,
// ranks the points and moves the records.
//   flag    one workgroup per chunk: the dist test of every point (on calibrated coordinates when the calibration comes first), left as the waves'
//           64-bit ballots — 32 bytes per chunk, which is what lets the later passes rank a point without evaluating the test (and its trigonometry) again.
//   ranks   one workgroup per frame: the exclusive scan of its chunks' survivor counts.  The thinning needs no pass: the survivor of rank r stays iff
//           r % ratio == 0 and lands at r / ratio, so a frame's size is multiples_below(survivors, ratio).
//   minmax  (time stamps only) per chunk, then per frame: upstream's max_ / min_ folds over the kept points' stamps, as trees that keep the cloud's order
//           (the folds are associative, not commutative: of +0 and -0 the later wins), and whether a stamp is NaN.  No atomics.
//   write   a kept point's record: calibration, time ratio, [compensation, pose], three float4 to out + rank / ratio.
// A point's rank comes from its wave's ballot and a lane-prefix popcount, plus the popcounts of the chunk's earlier waves, plus the chunk's base: nothing
// in the output depends on which workgroup runs first.
#include <hip/hip_runtime.h>

#include "scan_launch.h"

namespace
{
using namespace mulls::scan;

// the frame f with chunk0[f] <= g < chunk0[f + 1] (chunk0[F] is the grid; frames without points have no chunk and are never found)
__device__ __forceinline__ uint32_t find_frame(const uint32_t *__restrict__ chunk0, uint32_t F, uint32_t g)
{
	uint32_t lo = 0, hi = F;
	while (hi - lo > 1u)
	{
		const uint32_t mid = (lo + hi) >> 1;
		if (chunk0[mid] <= g)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

__global__ __launch_bounds__(MULLS_SCAN_CHUNK) void k_scan_flag(ScanBatch b, Prep P)
{
	const ScanFrame &f = b.frames[find_frame(b.chunk0, b.F, blockIdx.x)];
	const uint32_t i = (blockIdx.x - f.chunk0) * MULLS_SCAN_CHUNK + threadIdx.x;
	bool keep = false;
	if (i < f.n)
	{
		const float4 p = f.in[(size_t)i * 3];
		keep = survives(p.x, p.y, p.z, P);
	}
	const unsigned long long m = __ballot(keep);
	if ((threadIdx.x & 63u) == 0)
		b.ballots[(size_t)blockIdx.x * MULLS_SCAN_WAVES + (threadIdx.x >> 6)] = m;
}

__global__ __launch_bounds__(256) void k_scan_ranks(ScanBatch b, Prep P)
{
	__shared__ uint32_t sh[256];
	const ScanFrame &f = b.frames[blockIdx.x];
	const uint32_t nch = chunks_of(f.n);
	uint32_t running = 0;
	for (uint32_t c0 = 0; c0 < nch; c0 += 256u)
	{
		const uint32_t c = c0 + threadIdx.x;
		uint32_t cnt = 0;
		if (c < nch)
			for (uint32_t w = 0; w < MULLS_SCAN_WAVES; w++)
				cnt += (uint32_t)__popcll(b.ballots[(size_t)(f.chunk0 + c) * MULLS_SCAN_WAVES + w]);
		sh[threadIdx.x] = cnt;
		__syncthreads();
		for (uint32_t off = 1; off < 256u; off <<= 1)
		{
			const uint32_t v = threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
			__syncthreads();
			sh[threadIdx.x] += v;
			__syncthreads();
		}
		if (c < nch)
			b.base[f.chunk0 + c] = running + sh[threadIdx.x] - cnt;
		running += sh[255];
		__syncthreads();
	}
	if (threadIdx.x == 0)
	{
		ScanFrameStat s;
		s.n_dist = running;
		s.n_out = multiples_below(running, (uint32_t)P.ratio);
		s.nan_stamp = 0, s.pad = 0;
		s.first = MULLS_SCAN_FIRST_SEED, s.last = MULLS_SCAN_LAST_SEED;
		b.stats[blockIdx.x] = s;
	}
}

// this lane's point of chunk blockIdx.x: does it stay, and its rank among its frame's survivors of the dist filter
struct Rank
{
	bool kept;
	uint32_t rank;
};
__device__ __forceinline__ Rank rank_of(const ScanBatch &b, uint32_t ratio)
{
	const uint64_t *bal = b.ballots + (size_t)blockIdx.x * MULLS_SCAN_WAVES;
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	uint32_t before = 0;
	for (uint32_t w = 0; w < wave; w++)
		before += (uint32_t)__popcll(bal[w]);
	const uint64_t m = bal[wave];
	before += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
	const uint32_t rank = b.base[blockIdx.x] + before;
	return Rank{((m >> lane) & 1ull) != 0 && rank % ratio == 0, rank};
}

// the folds of a workgroup of 256 lanes, lane order = the cloud's order; thread 0 leaves with the results
__device__ __forceinline__ void block_fold(double &first, double &last, uint32_t &bad)
{
	__shared__ double sh_first[4], sh_last[4];
	__shared__ uint32_t sh_bad[4];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t off = 1; off < 64u; off <<= 1)
	{
		const double of = __shfl_down(first, off), ol = __shfl_down(last, off);
		if ((lane & (2u * off - 1u)) == 0) // lanes lane .. lane + off - 1 on the left, lane + off .. on the right
		{
			first = fold_first(first, of);
			last = fold_last(last, ol);
		}
	}
	const bool any_bad = __ballot(bad != 0) != 0ull;
	if (lane == 0)
	{
		sh_first[wave] = first, sh_last[wave] = last;
		sh_bad[wave] = any_bad ? 1u : 0u;
	}
	__syncthreads();
	if (threadIdx.x == 0)
		for (uint32_t w = 1; w < 4u; w++)
		{
			first = fold_first(first, sh_first[w]);
			last = fold_last(last, sh_last[w]);
			bad |= sh_bad[w];
		}
	if (threadIdx.x == 0)
		bad |= sh_bad[0];
}

__global__ __launch_bounds__(MULLS_SCAN_CHUNK) void k_scan_minmax(ScanBatch b, Prep P)
{
	static_assert(MULLS_SCAN_CHUNK == 256u, "block_fold folds four waves");
	const ScanFrame &f = b.frames[find_frame(b.chunk0, b.F, blockIdx.x)];
	const uint32_t i = (blockIdx.x - f.chunk0) * MULLS_SCAN_CHUNK + threadIdx.x;
	const Rank r = rank_of(b, (uint32_t)P.ratio);
	double first = MULLS_SCAN_FIRST_SEED, last = MULLS_SCAN_LAST_SEED;
	uint32_t bad = 0;
	if (r.kept) // (a kept point is inside the frame: the flag pass left 0 beyond its end)
	{
		const double c = (double)f.in[(size_t)i * 3 + 2].y;
		bad = c != c;
		first = fold_first(first, c);
		last = fold_last(last, c);
	}
	block_fold(first, last, bad);
	if (threadIdx.x == 0)
	{
		b.chunk_first[blockIdx.x] = first;
		b.chunk_last[blockIdx.x] = last;
		b.chunk_nan[blockIdx.x] = bad;
	}
}

__global__ __launch_bounds__(256) void k_scan_minmax_frame(ScanBatch b)
{
	const ScanFrame &f = b.frames[blockIdx.x];
	const uint32_t nch = chunks_of(f.n), per = (nch + 255u) / 256u; // a lane folds `per` consecutive chunks
	double first = MULLS_SCAN_FIRST_SEED, last = MULLS_SCAN_LAST_SEED;
	uint32_t bad = 0;
	for (uint32_t k = 0; k < per; k++)
	{
		const uint32_t c = threadIdx.x * per + k;
		if (c < nch)
		{
			first = fold_first(first, b.chunk_first[f.chunk0 + c]);
			last = fold_last(last, b.chunk_last[f.chunk0 + c]);
			bad |= b.chunk_nan[f.chunk0 + c];
		}
	}
	block_fold(first, last, bad);
	if (threadIdx.x == 0)
	{
		b.stats[blockIdx.x].first = first;
		b.stats[blockIdx.x].last = last;
		b.stats[blockIdx.x].nan_stamp = bad;
	}
}

__global__ __launch_bounds__(MULLS_SCAN_CHUNK) void k_scan_write(ScanBatch b, Prep P)
{
	const ScanFrame &f = b.frames[find_frame(b.chunk0, b.F, blockIdx.x)];
	const uint32_t i = (blockIdx.x - f.chunk0) * MULLS_SCAN_CHUNK + threadIdx.x;
	const Rank r = rank_of(b, (uint32_t)P.ratio);
	if (!r.kept)
		return;
	const float4 *rec = f.in + (size_t)i * 3;
	float4 r0 = rec[0], r2 = rec[2];
	const float4 r1 = rec[1];
	finish_point(r0.x, r0.y, r0.z, r2.y, P, f.move);
	float4 *o = f.out + (size_t)(r.rank / (uint32_t)P.ratio) * 3; // below the frame's n_out: rank < n_dist and rank % ratio == 0
	o[0] = r0;
	o[1] = r1;
	o[2] = r2;
}
} // namespace

hipError_t launch_scan_flag(hipStream_t st, const ScanBatch &b, const Prep &P)
{
	if (b.G)
		hipLaunchKernelGGL(k_scan_flag, dim3(b.G), dim3(MULLS_SCAN_CHUNK), 0, st, b, P);
	return hipGetLastError();
}
hipError_t launch_scan_ranks(hipStream_t st, const ScanBatch &b, const Prep &P)
{
	if (b.F)
		hipLaunchKernelGGL(k_scan_ranks, dim3(b.F), dim3(256), 0, st, b, P);
	return hipGetLastError();
}
hipError_t launch_scan_minmax(hipStream_t st, const ScanBatch &b, const Prep &P)
{
	if (b.G)
		hipLaunchKernelGGL(k_scan_minmax, dim3(b.G), dim3(MULLS_SCAN_CHUNK), 0, st, b, P);
	if (b.F)
		hipLaunchKernelGGL(k_scan_minmax_frame, dim3(b.F), dim3(256), 0, st, b);
	return hipGetLastError();
}
hipError_t launch_scan_write(hipStream_t st, const ScanBatch &b, const Prep &P)
{
	if (b.G)
		hipLaunchKernelGGL(k_scan_write, dim3(b.G), dim3(MULLS_SCAN_CHUNK), 0, st, b, P);
	return hipGetLastError();
}
