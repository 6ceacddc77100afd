// map_kernels.hip — device side of the local map (MapManager::update_local_map, src/map_manager.cpp:18-140; dynamic
// object removal :149-268).  Clouds stay 48-B PointXYZINormal records (3 float4: x y z -, nx ny nz -, intensity
// curvature - -) so that a map class cloud can be handed to mulls_icp as a device-resident target unchanged.
#include <hip/hip_runtime.h>

#include "map_bodies.h"
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

// get_cloud_bbx (utility.hpp:817-848) over the six class clouds, and over the same points moved by pose_lo
// (pcl::transformPointCloud: double arithmetic, float store) — ordered-uint atomics; NaN coordinates never win a
// comparison in the reference and are skipped here.
__global__ __launch_bounds__(256) void k_map_bbox(MapBoxArgs a)
{
	const uint32_t cls = blockIdx.y;
	map_body::bbox(a.recs[cls], blockIdx.x * blockDim.x + threadIdx.x, a.n[cls], gridDim.x * blockDim.x, a.pose, a.keys);
}

// Exact nearest tree point (FLANN L2_Simple<float> distance) of every frame point, brute force: blockIdx.y splits the tree
// into chunks of MAP_NN_CHUNK points staged through LDS, atomicMin on the float bits combines the chunks (distances are >= 0).
// (the body, MAP_NN_CHUNK and MAP_NN_TILE: map_bodies.h)
__global__ __launch_bounds__(256) void k_map_nn(const float4 *__restrict__ frame, uint32_t n_frame, const float4 *__restrict__ tree, uint32_t n_tree,
												 int use_box, double b0, double b1, double b2, double b3, double b4, double b5,
												 uint32_t *__restrict__ best)
{
	__shared__ float4 tile[MAP_NN_TILE];
	map_body::nn(frame, n_frame, tree, n_tree, use_box, b0, b1, b2, b3, b4, b5, best, blockIdx.x, blockIdx.y, tile);
}

// map_scan_feature_pts_distance_removal's keep rule (map_manager.cpp:246-256), all in float as written there
__global__ void k_map_keep(const float4 *__restrict__ frame, uint32_t n_frame, const uint32_t *__restrict__ best, float center_radius, float dmin,
						   float dmax, float near, uint8_t *__restrict__ keep)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= n_frame)
		return;
	map_body::keep(frame, q, best, center_radius, dmin, dmax, near, keep);
}

// ---------------------------------------------------------------------------------------------------------------------
// MapManager::update_cloud_vectors (src/map_manager.cpp:258-292): every point of a linear-feature cloud gets the principal direction
// of its radius-limited k-neighbourhood (pca.hpp:209-290, :392-437) and survives only if the neighbourhood is linear enough and its
// direction steep (pillars) or flat (beams) enough.  One lane per point; the cloud streams through LDS in 256-point tiles and every
// lane keeps its `max_k` nearest neighbours as a sorted list in LDS (slot-major, so that neighbouring lanes touch neighbouring banks).
// A cloud of a few thousand points is all this ever sees (the map's pillar / beam share of max_num_pts): n^2 distances is microseconds.
//   neighbourhood   squared L2_Simple distance (((dx*dx)+dy*dy)+dz*dz, float) < radius^2, the max_k nearest in (distance, index) order,
//                   the point itself included — pcl::KdTreeFLANN::radiusSearch with max_nn
//   pcl::PCA        float centroid and float demeaned covariance summed in the neighbours' order, scaled by 1/(n-1); the
//                   eigen-decomposition of that float matrix in double (cyclic Jacobi), eigenvalues rounded to float
// (the body and MAP_PCA_K, the list slots per lane: map_bodies.h)
__global__ __launch_bounds__(256) void k_map_pca(MapPcaArgs a)
{
	__shared__ float tx[256], ty[256], tz[256];
	__shared__ float ld[MAP_PCA_K * 256];
	__shared__ uint32_t li[MAP_PCA_K * 256];
	map_body::pca(a, blockIdx.x, tx, ty, tz, ld, li);
}
void launch_map_pca(hipStream_t st, const MapPcaArgs &a)
{
	if (a.n)
		hipLaunchKernelGGL(k_map_pca, dim3((a.n + 255u) / 256u), dim3(256), 0, st, a);
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
void launch_map_bbox(hipStream_t st, const MapBoxArgs &a) { hipLaunchKernelGGL(k_map_bbox, dim3(64, 6), dim3(256), 0, st, a); }
void launch_map_nn(hipStream_t st, const float4 *frame, uint32_t n_frame, const float4 *tree, uint32_t n_tree, int use_box, const double box[6],
				   uint32_t *best)
{
	if (!n_frame || !n_tree)
		return;
	hipLaunchKernelGGL(k_map_nn, dim3((n_frame + 255) / 256, (n_tree + MAP_NN_CHUNK - 1) / MAP_NN_CHUNK), dim3(256), 0, st, frame, n_frame, tree,
					   n_tree, use_box, box[0], box[1], box[2], box[3], box[4], box[5], best);
}
void launch_map_keep(hipStream_t st, const float4 *frame, uint32_t n_frame, const uint32_t *best, float center_radius, float dmin, float dmax,
					 float near, uint8_t *keep)
{
	if (n_frame)
		hipLaunchKernelGGL(k_map_keep, dim3((n_frame + 255) / 256), dim3(256), 0, st, frame, n_frame, best, center_radius, dmin, dmax, near, keep);
}
