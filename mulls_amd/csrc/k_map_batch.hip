// k_map_batch.hip — the local map's kernels in table-driven form (mulls_map_update_batch, map_batch.cpp): every workgroup reads its job — which entry of the
// launch's table, which block of that entry's cloud — from a flat list in device memory, so one launch serves every map and class of a lock-step group and its
// grid is the sum of the work, not the largest cloud times the group.  The arithmetic is map_bodies.h, the text the one-map kernels run: the bytes are theirs.
// Combining stays order-free: atomicMin on a frame point's `best` word, ordered-uint min / max on a map's 12 `keys` words.
#include <hip/hip_runtime.h>

#include "map_bodies.h"
#include "map_launch.h"

// several byte ranges in one launch: the frames' clouds on their way into the maps' frame buffers (from the pinned staging or from device-resident sources), the
// frames' clouds appended to the class clouds, class clouds moving to a larger buffer
__global__ __launch_bounds__(256) void k_mapb_copy(const MapbCopyEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	const MapbJob j = jobs[blockIdx.x];
	const MapbCopyEnt e = ent[j.ent];
	const size_t first = (size_t)j.block * MAPB_COPY_BLOCK;
	if (first >= e.bytes)
		return;
	const uint32_t len = (uint32_t)min((size_t)MAPB_COPY_BLOCK, (size_t)e.bytes - first);
	if (((e.dst | e.src) & 15ull) == 0ull)
	{
		const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(e.src + first);
		uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(e.dst + first);
		const uint32_t w16 = len >> 4;
		uint4 v[4];
#pragma unroll
		for (int k = 0; k < 4; k++)
		{
			const uint32_t w = threadIdx.x + 256u * (uint32_t)k;
			v[k] = w < w16 ? src[w] : make_uint4(0u, 0u, 0u, 0u);
		}
#pragma unroll
		for (int k = 0; k < 4; k++)
		{
			const uint32_t w = threadIdx.x + 256u * (uint32_t)k;
			if (w < w16)
				dst[w] = v[k];
		}
		// (a tail of 4, 8 or 12 bytes: only the last block of a range whose size is no multiple of 16)
		const uint32_t *__restrict__ s4 = reinterpret_cast<const uint32_t *>(e.src + first);
		uint32_t *__restrict__ d4 = reinterpret_cast<uint32_t *>(e.dst + first);
		const uint32_t w = (w16 << 2) + threadIdx.x;
		if (w < (len >> 2))
			d4[w] = s4[w];
	}
	else
	{
		const uint32_t *__restrict__ s4 = reinterpret_cast<const uint32_t *>(e.src + first);
		uint32_t *__restrict__ d4 = reinterpret_cast<uint32_t *>(e.dst + first);
		for (uint32_t w = threadIdx.x; w < (len >> 2); w += 256u)
			d4[w] = s4[w];
	}
}

__global__ __launch_bounds__(256) void k_mapb_transform(const MapbXformEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	const MapbJob j = jobs[blockIdx.x];
	const MapbXformEnt *e = ent + j.ent;
	const uint32_t i = j.block * 256u + threadIdx.x;
	if (i >= e->n)
		return;
	map_body::transform(e->recs, i, e->T);
}

__global__ __launch_bounds__(256) void k_mapb_fill_best(const MapbRemEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	const MapbJob j = jobs[blockIdx.x];
	const MapbRemEnt *e = ent + j.ent;
	const uint32_t q = j.block * 256u + threadIdx.x;
	if (q < e->n_frame)
		e->best[q] = 0x7f800000u;
}

__global__ __launch_bounds__(256) void k_mapb_nn(const MapbRemEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	__shared__ float4 tile[MAP_NN_TILE];
	const MapbJob j = jobs[blockIdx.x];
	const MapbRemEnt *e = ent + j.ent;
	map_body::nn(e->frame, e->n_frame, e->tree, e->n_tree, e->use_box, e->box[0], e->box[1], e->box[2], e->box[3], e->box[4], e->box[5], e->best, j.block, j.chunk,
				 tile);
}

__global__ __launch_bounds__(256) void k_mapb_keep(const MapbRemEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	const MapbJob j = jobs[blockIdx.x];
	const MapbRemEnt *e = ent + j.ent;
	const uint32_t q = j.block * 256u + threadIdx.x;
	if (q >= e->n_frame)
		return;
	map_body::keep(e->frame, q, e->best, e->center_radius, e->dmin, e->dmax, e->near_, e->keep);
}

__global__ __launch_bounds__(256) void k_mapb_bbox(const MapbBoxEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	const MapbJob j = jobs[blockIdx.x];
	const MapbBoxEnt *e = ent + j.ent;
	const uint32_t t0 = j.block * MAPB_BOX_TILE, t1 = min(e->n, t0 + MAPB_BOX_TILE);
	map_body::bbox(e->recs, t0 + threadIdx.x, t1, 256u, e->pose, e->keys);
}

// 51 KB of LDS per workgroup (48 KB of neighbour lists, 3 KB of tile): three workgroups, twelve waves, share a CU's 160 KB.  Halving the block to 128 lanes
// halves the lists and doubles the workgroups per CU — the same twelve waves — and would stage every tile twice as often, so the block stays the one-map
// kernel's 256 and the tile loop stays its text.
__global__ __launch_bounds__(256) void k_mapb_pca(const MapPcaArgs *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	__shared__ float tx[256], ty[256], tz[256];
	__shared__ float ld[MAP_PCA_K * 256];
	__shared__ uint32_t li[MAP_PCA_K * 256];
	const MapbJob j = jobs[blockIdx.x];
	const MapPcaArgs a = ent[j.ent];
	map_body::pca(a, j.block, tx, ty, tz, ld, li);
}

#define MAPB_LAUNCH(kernel)                                                             \
	if (!n_jobs)                                                                        \
		return 0;                                                                       \
	hipLaunchKernelGGL(kernel, dim3(n_jobs), dim3(256), 0, st, ent, jobs);              \
	return 1;
int launch_mapb_copy(hipStream_t st, const MapbCopyEnt *ent, const MapbJob *jobs, uint32_t n_jobs) { MAPB_LAUNCH(k_mapb_copy) }
int launch_mapb_transform(hipStream_t st, const MapbXformEnt *ent, const MapbJob *jobs, uint32_t n_jobs) { MAPB_LAUNCH(k_mapb_transform) }
int launch_mapb_fill_best(hipStream_t st, const MapbRemEnt *ent, const MapbJob *jobs, uint32_t n_jobs) { MAPB_LAUNCH(k_mapb_fill_best) }
int launch_mapb_nn(hipStream_t st, const MapbRemEnt *ent, const MapbJob *jobs, uint32_t n_jobs) { MAPB_LAUNCH(k_mapb_nn) }
int launch_mapb_keep(hipStream_t st, const MapbRemEnt *ent, const MapbJob *jobs, uint32_t n_jobs) { MAPB_LAUNCH(k_mapb_keep) }
int launch_mapb_bbox(hipStream_t st, const MapbBoxEnt *ent, const MapbJob *jobs, uint32_t n_jobs) { MAPB_LAUNCH(k_mapb_bbox) }
int launch_mapb_pca(hipStream_t st, const MapPcaArgs *ent, const MapbJob *jobs, uint32_t n_jobs) { MAPB_LAUNCH(k_mapb_pca) }
