// k_image.hip — the kernels of mulls_cloud_centre, mulls_map_image_2d, mulls_range_image and mulls_scan_images_batch: CloudUtility::get_cloud_cpt,
// CFilter::generate_2d_map and CFilter::pointcloud_to_rangeimage over the scans of one sub-batch per launch.  The arithmetic is image_math.h's (the text
// the CPU harness compiles); a kernel here only finds its scan and chunk and folds the results.
//   centre   MULLS_NDT_TREE lanes per scan: lane l adds the terms of the points l, l + MULLS_NDT_TREE, .. in order (the strided partials of k_ndt.hip);
//            then one workgroup per scan runs the halving tree.
//   count    one workgroup per chunk: a point's pixel, and an integer atomic add on its count.  Two forms: one add per point; or a wave first folds runs of
//            equal pixels among neighbouring lanes and one lane per run adds the run's length.  profiles/images.txt has both measured.
//   range    one workgroup per chunk: a point's pixel and value, and an atomic max of (index << 8) | value: the highest index wins, in any order.
//   convert  over all pixels of all scans: counts to 8 bits, words to their low byte; the scans' counters into their stats.
// Every result is an integer reached by commutative atomics (add, max) or a sum in a fixed order: nothing depends on which workgroup runs first.
#include <hip/hip_runtime.h>

#include "image_launch.h"

namespace
{
using namespace mulls::image;

// the scan s with chunk0[s] <= g < chunk0[s + 1] (chunk0[S] is the grid; scans without points have no chunk and are never found)
__device__ __forceinline__ uint32_t find_scan(const uint32_t *__restrict__ chunk0, uint32_t S, uint32_t g)
{
	uint32_t lo = 0, hi = S;
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

constexpr uint32_t CENTRE_AHEAD = 8; // records a lane has in flight before it adds them, in order

__global__ __launch_bounds__(256) void k_image_centre_partial(ImageBatch b)
{
	const ImageScan f = b.scans[blockIdx.y];
	const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
	double acc[3] = {0.0, 0.0, 0.0};
	for (uint64_t i0 = lane; i0 < f.n; i0 += (uint64_t)CENTRE_AHEAD * MULLS_NDT_TREE)
	{
		float4 p[CENTRE_AHEAD];
#pragma unroll
		for (uint32_t k = 0; k < CENTRE_AHEAD; k++)
		{
			const uint64_t i = i0 + (uint64_t)k * MULLS_NDT_TREE;
			if (i < f.n)
				p[k] = f.in[i * 3];
		}
#pragma unroll
		for (uint32_t k = 0; k < CENTRE_AHEAD; k++)
			if (i0 + (uint64_t)k * MULLS_NDT_TREE < f.n)
			{
				acc[0] += centre_term(p[k].x, f.n);
				acc[1] += centre_term(p[k].y, f.n);
				acc[2] += centre_term(p[k].z, f.n);
			}
	}
	for (uint32_t k = 0; k < 3u; k++)
		b.partial[((size_t)blockIdx.y * 3u + k) * MULLS_NDT_TREE + lane] = acc[k];
}

__global__ __launch_bounds__(256) void k_image_centre_tree(ImageBatch b)
{
	__shared__ double sh[MULLS_NDT_TREE];
	for (uint32_t k = 0; k < 3u; k++)
	{
		const double *partial = b.partial + ((size_t)blockIdx.x * 3u + k) * MULLS_NDT_TREE;
		for (uint32_t l = threadIdx.x; l < MULLS_NDT_TREE; l += 256u)
			sh[l] = partial[l];
		__syncthreads();
		for (uint32_t w = MULLS_NDT_TREE / 2u; w >= 1u; w >>= 1)
		{
			for (uint32_t l = threadIdx.x; l < w; l += 256u)
				sh[l] += sh[l + w];
			__syncthreads();
		}
		if (threadIdx.x == 0)
			b.stats[blockIdx.x].centre[k] = sh[0];
		__syncthreads();
	}
}

// one add for the lanes of a wave for which `is` holds
__device__ __forceinline__ void wave_count(uint32_t *counter, bool is)
{
	const unsigned long long m = __ballot(is);
	if ((threadIdx.x & 63u) == 0 && m)
		atomicAdd(counter, (uint32_t)__popcll(m));
}

template <int FORM>
__global__ __launch_bounds__(MULLS_SCAN_CHUNK) void k_image_count(ImageBatch b, Map2d M)
{
	const uint32_t s = find_scan(b.chunk0, b.S, blockIdx.x);
	const ImageScan f = b.scans[s];
	const uint32_t i = (blockIdx.x - f.chunk0) * MULLS_SCAN_CHUNK + threadIdx.x;
	uint32_t kind = 3u, pixel = 0;
	if (i < f.n)
	{
		const float4 p = f.in[(size_t)i * 3];
		const float shift_x = M.shift ? (float)b.stats[s].centre[0] : 0.0f, shift_y = M.shift ? (float)b.stats[s].centre[1] : 0.0f;
		kind = map_point(p.x, p.y, p.z, shift_x, shift_y, M, &pixel);
	}
	wave_count(b.counters + 4u * s + MAP_COUNTED, kind == MAP_COUNTED);
	wave_count(b.counters + 4u * s + MAP_SKIPPED_HEIGHT, kind == MAP_SKIPPED_HEIGHT);
	wave_count(b.counters + 4u * s + MAP_SKIPPED_FRAME, kind == MAP_SKIPPED_FRAME);
	int32_t *counts = b.counts + (size_t)s * b.map_pixels; // pixel < map_pixels: map_point's range test
	if (FORM == 1)
	{
		if (kind == MAP_COUNTED)
			atomicAdd(counts + pixel, 1);
	}
	else
	{
		// runs of equal pixels among the wave's lanes: a lane is the head of a run when its key differs from the lane below; the run ends in front of the
		// next head.  A lane without a pixel has a key no pixel has (pixels are below 2^26), so it ends a run and starts none that is added.
		const uint32_t lane = threadIdx.x & 63u;
		const uint32_t key = kind == MAP_COUNTED ? pixel : 0xffffffffu;
		const uint32_t below = __shfl_up(key, 1);
		const bool head = lane == 0 || key != below;
		const unsigned long long heads = __ballot(head);
		if (head && kind == MAP_COUNTED)
		{
			const unsigned long long above = lane == 63u ? 0ull : heads >> (lane + 1u);
			const uint32_t len = above ? (uint32_t)__ffsll((long long)above) : 64u - lane; // ffs counts from 1: the next head is ffs lanes up
			atomicAdd(counts + pixel, (int32_t)len);
		}
	}
}

__global__ __launch_bounds__(MULLS_SCAN_CHUNK) void k_image_range(ImageBatch b, Range R)
{
	const uint32_t s = find_scan(b.chunk0, b.S, blockIdx.x);
	const ImageScan f = b.scans[s];
	const uint32_t i = (blockIdx.x - f.chunk0) * MULLS_SCAN_CHUNK + threadIdx.x;
	if (i >= f.n)
		return;
	const float4 p = f.in[(size_t)i * 3];
	uint32_t pixel, value;
	if (range_point(p.x, p.y, p.z, R, &pixel, &value)) // pixel < range_pixels: range_point's clamps; value <= 255; i < 2^24
		atomicMax(b.words + (size_t)s * b.range_pixels + pixel, (i << 8) | value);
}

// a thread converts four neighbouring pixels and stores them as one word: the blocks [0, bev_blocks) the 2-D map images, the others the range images.
// (Both 32-bit arrays and both byte arrays end on a multiple of 256 bytes: the last group of four is inside them.)
__global__ __launch_bounds__(256) void k_image_convert(ImageBatch b, Map2d M, uint32_t bev_blocks)
{
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	for (uint32_t s = t; s < b.S; s += gridDim.x * 256u) // the scans' counters, by the grid's first threads
	{
		ImageStat &st = b.stats[s];
		st.counted = b.counters[4u * s + MAP_COUNTED], st.skipped_height = b.counters[4u * s + MAP_SKIPPED_HEIGHT];
		st.skipped_frame = b.counters[4u * s + MAP_SKIPPED_FRAME], st.pad = 0;
	}
	if (blockIdx.x < bev_blocks)
	{
		const size_t p = (size_t)t * 4u;
		if (p >= (size_t)b.S * b.map_pixels)
			return;
		const int4 c = *reinterpret_cast<const int4 *>(b.counts + p);
		const uint32_t v = (uint32_t)map_value(c.x, M.min_points, M.a) | (uint32_t)map_value(c.y, M.min_points, M.a) << 8 |
						   (uint32_t)map_value(c.z, M.min_points, M.a) << 16 | (uint32_t)map_value(c.w, M.min_points, M.a) << 24;
		*reinterpret_cast<uint32_t *>(b.bev + p) = v;
	}
	else
	{
		const size_t p = ((size_t)(blockIdx.x - bev_blocks) * 256u + threadIdx.x) * 4u;
		if (p >= (size_t)b.S * b.range_pixels)
			return;
		const uint4 w = *reinterpret_cast<const uint4 *>(b.words + p);
		*reinterpret_cast<uint32_t *>(b.range + p) = (w.x & 255u) | (w.y & 255u) << 8 | (w.z & 255u) << 16 | (w.w & 255u) << 24;
	}
}

uint32_t blocks_of(size_t pixels) { return (uint32_t)((pixels + 1023u) / 1024u); }
} // namespace

hipError_t launch_image_centre(hipStream_t st, const ImageBatch &b)
{
	if (b.S)
	{
		hipLaunchKernelGGL(k_image_centre_partial, dim3(MULLS_NDT_TREE / 256u, b.S), dim3(256), 0, st, b);
		hipLaunchKernelGGL(k_image_centre_tree, dim3(b.S), dim3(256), 0, st, b);
	}
	return hipGetLastError();
}
hipError_t launch_image_count(hipStream_t st, const ImageBatch &b, const Map2d &M, int form)
{
	if (b.G && form == 2)
		hipLaunchKernelGGL(k_image_count<2>, dim3(b.G), dim3(MULLS_SCAN_CHUNK), 0, st, b, M);
	else if (b.G)
		hipLaunchKernelGGL(k_image_count<1>, dim3(b.G), dim3(MULLS_SCAN_CHUNK), 0, st, b, M);
	return hipGetLastError();
}
hipError_t launch_image_range(hipStream_t st, const ImageBatch &b, const Range &R)
{
	if (b.G)
		hipLaunchKernelGGL(k_image_range, dim3(b.G), dim3(MULLS_SCAN_CHUNK), 0, st, b, R);
	return hipGetLastError();
}
hipError_t launch_image_convert(hipStream_t st, const ImageBatch &b, const Map2d &M)
{
	const uint32_t bev_blocks = blocks_of((size_t)b.S * b.map_pixels), range_blocks = blocks_of((size_t)b.S * b.range_pixels);
	const uint32_t grid = bev_blocks + range_blocks;
	if (grid)
		hipLaunchKernelGGL(k_image_convert, dim3(grid), dim3(256), 0, st, b, M, bev_blocks);
	return hipGetLastError();
}
