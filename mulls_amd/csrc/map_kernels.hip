// map_kernels.hip — the stable segmented compaction of 48-B record clouds: the local map's radius filter, thinning, dynamic removal and refresh
// (map_batch.cpp), and the ground filter, classifier, non-maximum suppression and feature-extraction batch.  Clouds stay 48-B PointXYZINormal records
// (3 float4: x y z -, nx ny nz -, intensity curvature - -) so that a map class cloud can be handed to mulls_icp as a device-resident target unchanged.
// (the local map's other kernels: k_map_batch.hip)
#include <hip/hip_runtime.h>

#include "map_launch.h"

// Stable compaction of up to six clouds in three steps, so that a 400 k-point class cloud is not left to one CU's memory
// bandwidth: (1) every 256-lane workgroup counts the survivors of one 4096-record segment, (2) one workgroup per cloud
// turns the segment counts into segment bases (and the cloud's new size), (3) every workgroup rewrites its segment behind
// its base.  The order of the survivors is the input order (the reference pushes them back one by one).
#define MAP_SEG 4096u
namespace
{
__device__ __forceinline__ bool map_keep(const MapCompactArgs &a, const MapCloudArg &c, uint32_t i, const float4 &r0, double r2)
{
	if (a.mode == 0)
		return c.mask[i] != 0;
	const double dis_square = (double)(r0.x * r0.x + r0.y * r0.y); // float products and sum, then widened (cfilter.hpp:845)
	return dis_square < r2 && r0.z < 1.7976931348623157e308 && r0.z > -1.7976931348623157e308;
}
// which cloud and which of its segments a workgroup owns
__device__ __forceinline__ bool map_segment(const MapCompactArgs &a, uint32_t b, uint32_t &cloud, uint32_t &seg)
{
	for (cloud = 0; cloud < 6; cloud++)
	{
		const uint32_t ns = (a.cloud[cloud].n + MAP_SEG - 1u) / MAP_SEG;
		if (b < ns)
		{
			seg = b;
			return true;
		}
		b -= ns;
	}
	return false;
}
} // namespace

#define MAP_SEG_COUNT_BODY \
	__shared__ uint32_t wave_cnt[4]; \
	uint32_t cloud, seg; \
	if (!map_segment(a, blockIdx.x, cloud, seg)) \
		return; \
	const MapCloudArg c = a.cloud[cloud]; \
	const double r2 = a.radius * a.radius; \
	uint32_t mine = 0; \
	for (uint32_t k = 0; k < MAP_SEG; k += 256) \
	{ \
		const uint32_t i = seg * MAP_SEG + k + threadIdx.x; \
		if (i < c.n) \
			mine += map_keep(a, c, i, c.in[(size_t)i * 3], r2) ? 1u : 0u; \
	} \
	for (int off = 32; off > 0; off >>= 1) \
		mine += __shfl_down(mine, off); \
	if ((threadIdx.x & 63) == 0) \
		wave_cnt[threadIdx.x >> 6] = mine; \
	__syncthreads(); \
	if (threadIdx.x == 0) \
		seg_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3]; \
	/* end of MAP_SEG_COUNT_BODY */

// exclusive scan of each cloud's segment counts (in place), cloud totals to out_n; segments per cloud are few (<= a few hundred)
#define MAP_SEG_SCAN_BODY \
	uint32_t first = 0; \
	for (uint32_t c = 0; c < blockIdx.x; c++) \
		first += (a.cloud[c].n + MAP_SEG - 1u) / MAP_SEG; \
	const uint32_t ns = (a.cloud[blockIdx.x].n + MAP_SEG - 1u) / MAP_SEG; \
	uint32_t running = 0; \
	for (uint32_t base = 0; base < ns; base += 64) \
	{ \
		const uint32_t s = base + threadIdx.x; \
		const uint32_t v = s < ns ? seg_cnt[first + s] : 0u; \
		uint32_t incl = v; \
		for (int off = 1; off < 64; off <<= 1) \
		{ \
			const uint32_t o = __shfl_up(incl, off); \
			if ((int)threadIdx.x >= off) \
				incl += o; \
		} \
		if (s < ns) \
			seg_cnt[first + s] = running + incl - v; \
		running += __shfl(incl, 63); \
	} \
	if (threadIdx.x == 0) \
		a.out_n[blockIdx.x] = running; \
	/* end of MAP_SEG_SCAN_BODY */

#define MAP_SEG_SCATTER_BODY \
	__shared__ uint32_t wave_cnt[4]; \
	uint32_t cloud, seg; \
	if (!map_segment(a, blockIdx.x, cloud, seg)) \
		return; \
	const MapCloudArg c = a.cloud[cloud]; \
	const double r2 = a.radius * a.radius; \
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6; \
	uint32_t running = seg_base[blockIdx.x]; \
	for (uint32_t k = 0; k < MAP_SEG; k += 256) \
	{ \
		const uint32_t i = seg * MAP_SEG + k + threadIdx.x; \
		bool keep = false; \
		float4 r0, r1, rr; \
		if (i < c.n) \
		{ \
			r0 = c.in[(size_t)i * 3]; \
			r1 = c.in[(size_t)i * 3 + 1]; \
			rr = c.in[(size_t)i * 3 + 2]; \
			keep = map_keep(a, c, i, r0, r2); \
		} \
		const unsigned long long b = __ballot(keep); \
		const uint32_t before = (uint32_t)__popcll(b & ((1ull << lane) - 1ull)); \
		__syncthreads(); \
		if (lane == 0) \
			wave_cnt[wave] = (uint32_t)__popcll(b); \
		__syncthreads(); \
		uint32_t wbase = 0, total = 0; \
		for (int w = 0; w < 4; w++) \
		{ \
			if (w < wave) \
				wbase += wave_cnt[w]; \
			total += wave_cnt[w]; \
		} \
		if (keep) \
		{ \
			const size_t o = (size_t)(running + wbase + before) * 3; \
			c.out[o] = r0; \
			c.out[o + 1] = r1; \
			c.out[o + 2] = rr; \
		} \
		running += total; \
	} \
	/* end of MAP_SEG_SCATTER_BODY */

// The three steps for one set of clouds (arguments by value, read where the launch put them) and for the set at blockIdx.y of a table in device memory
// (mulls_extract_features_batch).  One text, the MAP_*_BODY above, with `a` and the scratch bound either way: handing the by-value arguments on to a
// function by reference made the compiler keep a private copy of them (224 bytes of scratch per lane), so the bodies are spelled as macros.
__global__ __launch_bounds__(256) void k_map_seg_count(MapCompactArgs a, uint32_t *__restrict__ seg_cnt)
{
	MAP_SEG_COUNT_BODY
}
__global__ __launch_bounds__(64) void k_map_seg_scan(MapCompactArgs a, uint32_t *__restrict__ seg_cnt)
{
	MAP_SEG_SCAN_BODY
}
__global__ __launch_bounds__(256) void k_map_seg_scatter(MapCompactArgs a, const uint32_t *__restrict__ seg_base)
{
	MAP_SEG_SCATTER_BODY
}
__global__ __launch_bounds__(256) void k_map_seg_count_b(const MapCompactJob *__restrict__ tab)
{
	const MapCompactArgs &a = tab[blockIdx.y].a;
	uint32_t *__restrict__ seg_cnt = tab[blockIdx.y].seg;
	MAP_SEG_COUNT_BODY
}
__global__ __launch_bounds__(64) void k_map_seg_scan_b(const MapCompactJob *__restrict__ tab)
{
	const MapCompactArgs &a = tab[blockIdx.y].a;
	uint32_t *__restrict__ seg_cnt = tab[blockIdx.y].seg;
	if (!a.out_n) // (an entry without clouds has no counters to write either)
		return;
	MAP_SEG_SCAN_BODY
}
__global__ __launch_bounds__(256) void k_map_seg_scatter_b(const MapCompactJob *__restrict__ tab)
{
	const MapCompactArgs &a = tab[blockIdx.y].a;
	const uint32_t *__restrict__ seg_base = tab[blockIdx.y].seg;
	MAP_SEG_SCATTER_BODY
}

uint32_t map_compact_segments(const MapCompactArgs &a)
{
	uint32_t ns = 0;
	for (int c = 0; c < 6; c++)
		ns += (a.cloud[c].n + MAP_SEG - 1u) / MAP_SEG;
	return ns;
}
void launch_map_compact(hipStream_t st, const MapCompactArgs &a, uint32_t *seg_scratch)
{
	const uint32_t ns = map_compact_segments(a);
	if (ns)
		hipLaunchKernelGGL(k_map_seg_count, dim3(ns), dim3(256), 0, st, a, seg_scratch);
	hipLaunchKernelGGL(k_map_seg_scan, dim3(6), dim3(64), 0, st, a, seg_scratch);
	if (ns)
		hipLaunchKernelGGL(k_map_seg_scatter, dim3(ns), dim3(256), 0, st, a, seg_scratch);
}
int launch_map_compact_batch(hipStream_t st, const MapCompactJob *tab_dev, const MapCompactJob *tab_host, uint32_t count)
{
	uint32_t ns = 0;
	for (uint32_t b = 0; b < count; b++)
		ns = ns > map_compact_segments(tab_host[b].a) ? ns : map_compact_segments(tab_host[b].a);
	if (!count)
		return 0;
	if (ns)
		hipLaunchKernelGGL(k_map_seg_count_b, dim3(ns, count), dim3(256), 0, st, tab_dev);
	hipLaunchKernelGGL(k_map_seg_scan_b, dim3(6, count), dim3(64), 0, st, tab_dev);
	if (ns)
		hipLaunchKernelGGL(k_map_seg_scatter_b, dim3(ns, count), dim3(256), 0, st, tab_dev);
	return ns ? 3 : 1;
}
