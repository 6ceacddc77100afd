// k_map_batch.hip — the local map's kernels in table-driven form (mulls_map_update_batch, map_batch.cpp): every workgroup reads its job — which entry of the
// launch's table, which block of that entry's cloud — from a flat list in device memory, so one launch serves every map and class of a lock-step group and its
// grid is the sum of the work, not the largest cloud times the group.  mulls_map_update is a batch of one, so these are the only kernels of steps 2, 3, 8 and 9
// (the compactions: map_kernels.hip).  Combining stays order-free: atomicMin on a frame point's `best` word, ordered-uint min / max on a map's 12 `keys` words.
#include <hip/hip_runtime.h>

#include "map_launch.h"
#include "pca_device.h"

// (MAP_NN_CHUNK, the tree points per workgroup: map_launch.h — the host sizes its job lists by it)
#define MAP_NN_TILE 1024u
#define MAP_PCA_K 24 // list slots per lane (max_k <= 24: 48 KB of lists per workgroup)

namespace
{
__device__ __forceinline__ uint32_t float_ord(float f)
{
	const uint32_t u = __float_as_uint(f);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
} // namespace

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

// pcl::transformPointCloudWithNormals on a record: double arithmetic, float store; T = rows of [R|t]
__global__ __launch_bounds__(256) void k_mapb_transform(const MapbXformEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	const MapbJob j = jobs[blockIdx.x];
	const MapbXformEnt *e = ent + j.ent;
	const uint32_t i = j.block * 256u + threadIdx.x;
	if (i >= e->n)
		return;
	float4 *__restrict__ recs = e->recs;
	const double *T = e->T;
	float4 a = recs[(size_t)i * 3], b = recs[(size_t)i * 3 + 1];
	double x = a.x, y = a.y, z = a.z, nx = b.x, ny = b.y, nz = b.z;
	a.x = (float)(T[0] * x + T[1] * y + T[2] * z + T[3]);
	a.y = (float)(T[4] * x + T[5] * y + T[6] * z + T[7]);
	a.z = (float)(T[8] * x + T[9] * y + T[10] * z + T[11]);
	b.x = (float)(T[0] * nx + T[1] * ny + T[2] * nz);
	b.y = (float)(T[4] * nx + T[5] * ny + T[6] * nz);
	b.z = (float)(T[8] * nx + T[9] * ny + T[10] * nz);
	recs[(size_t)i * 3] = a;
	recs[(size_t)i * 3 + 1] = b;
}

__global__ __launch_bounds__(256) void k_mapb_fill_best(const MapbRemEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	const MapbJob j = jobs[blockIdx.x];
	const MapbRemEnt *e = ent + j.ent;
	const uint32_t q = j.block * 256u + threadIdx.x;
	if (q < e->n_frame)
		e->best[q] = 0x7f800000u;
}

// Exact nearest tree point (FLANN L2_Simple<float> distance) of the 256 frame points of block j.block, brute force, among the MAP_NN_CHUNK tree points of chunk
// j.chunk staged through LDS; atomicMin on the float bits combines the chunks (distances are >= 0).
__global__ __launch_bounds__(256) void k_mapb_nn(const MapbRemEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	__shared__ float4 tile[MAP_NN_TILE];
	const MapbJob j = jobs[blockIdx.x];
	const MapbRemEnt *e = ent + j.ent;
	const float4 *__restrict__ frame = e->frame, *__restrict__ tree = e->tree;
	uint32_t *__restrict__ best = e->best;
	const uint32_t n_frame = e->n_frame, n_tree = e->n_tree;
	const int use_box = e->use_box;
	const double b0 = e->box[0], b1 = e->box[1], b2 = e->box[2], b3 = e->box[3], b4 = e->box[4], b5 = e->box[5];
	const uint32_t q = j.block * blockDim.x + threadIdx.x;
	float qx = 0, qy = 0, qz = 0;
	if (q < n_frame)
	{
		const float4 p = frame[(size_t)q * 3];
		qx = p.x, qy = p.y, qz = p.z;
	}
	float d_best = __builtin_inff();
	const uint32_t t0 = j.chunk * MAP_NN_CHUNK, t1 = min(n_tree, t0 + MAP_NN_CHUNK);
	for (uint32_t base = t0; base < t1; base += MAP_NN_TILE)
	{
		__syncthreads();
		for (uint32_t k = threadIdx.x; k < MAP_NN_TILE; k += blockDim.x)
		{
			float4 t = make_float4(0, 0, 0, 0); // w = 1: member of the tree
			if (base + k < t1)
			{
				t = tree[(size_t)(base + k) * 3];
				const bool in = !use_box || (t.x > b0 && t.x < b3 && t.y > b1 && t.y < b4 && t.z > b2 && t.z < b5); // bbx_filter, cfilter.hpp:950-981
				t.w = in ? 1.0f : 0.0f;
			}
			tile[k] = t;
		}
		__syncthreads();
		const uint32_t cnt = min(MAP_NN_TILE, t1 - base);
		for (uint32_t k = 0; k < cnt; k++)
		{
			const float4 t = tile[k];
			float diff = qx - t.x;
			float d = diff * diff;
			diff = qy - t.y;
			d += diff * diff;
			diff = qz - t.z;
			d += diff * diff;
			if (t.w != 0.0f && d < d_best)
				d_best = d;
		}
	}
	if (q < n_frame && d_best < __builtin_inff())
		atomicMin(&best[q], __float_as_uint(d_best));
}

// map_scan_feature_pts_distance_removal's keep rule (map_manager.cpp:246-256), all in float as written there
__global__ __launch_bounds__(256) void k_mapb_keep(const MapbRemEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	const MapbJob j = jobs[blockIdx.x];
	const MapbRemEnt *e = ent + j.ent;
	const uint32_t q = j.block * 256u + threadIdx.x;
	if (q >= e->n_frame)
		return;
	const float4 p = e->frame[(size_t)q * 3];
	bool k = true;
	if (!(p.x * p.x + p.y * p.y > e->center_radius * e->center_radius))
	{
		const uint32_t bits = e->best[q];
		if (bits != 0x7f800000u) // an empty tree leaves the cloud alone (see oracle)
		{
			const float d2 = __uint_as_float(bits);
			k = (d2 > e->near_ * e->near_ && d2 < e->dmin * e->dmin) || d2 > e->dmax * e->dmax;
		}
	}
	e->keep[q] = k ? 1 : 0;
}

// get_cloud_bbx (utility.hpp:817-848) over one tile of a class cloud, and over the same points moved by pose_lo (pcl::transformPointCloud: double arithmetic,
// float store) — ordered-uint atomics; NaN coordinates never win a comparison in the reference and are skipped here.
// keys: [0..2] min xyz, [3..5] max xyz, [6..8] posed min, [9..11] posed max.
__global__ __launch_bounds__(256) void k_mapb_bbox(const MapbBoxEnt *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	const MapbJob j = jobs[blockIdx.x];
	const MapbBoxEnt *e = ent + j.ent;
	const uint32_t t0 = j.block * MAPB_BOX_TILE, t1 = min(e->n, t0 + MAPB_BOX_TILE);
	const float4 *__restrict__ recs = e->recs;
	const double *pose = e->pose;
	uint32_t *keys = e->keys;
	float lo[6], hi[6];
	for (int k = 0; k < 6; k++)
	{
		lo[k] = __builtin_inff();
		hi[k] = -__builtin_inff();
	}
	for (uint32_t i = t0 + threadIdx.x; i < t1; i += 256u)
	{
		const float4 p = recs[(size_t)i * 3];
		const double x = p.x, y = p.y, z = p.z;
		const float v[6] = {p.x, p.y, p.z, (float)(pose[0] * x + pose[1] * y + pose[2] * z + pose[3]),
							(float)(pose[4] * x + pose[5] * y + pose[6] * z + pose[7]),
							(float)(pose[8] * x + pose[9] * y + pose[10] * z + pose[11])};
		for (int k = 0; k < 6; k++)
		{
			lo[k] = fminf(lo[k], v[k]);
			hi[k] = fmaxf(hi[k], v[k]);
		}
	}
	for (int k = 0; k < 6; k++)
	{
		for (int off = 32; off > 0; off >>= 1)
		{
			lo[k] = fminf(lo[k], __shfl_down(lo[k], off));
			hi[k] = fmaxf(hi[k], __shfl_down(hi[k], off));
		}
		if ((threadIdx.x & 63) == 0)
		{
			const int base = k < 3 ? 0 : 6, ax = k % 3;
			if (lo[k] <= hi[k])
			{
				atomicMin(&keys[base + ax], float_ord(lo[k]));
				atomicMax(&keys[base + 3 + ax], float_ord(hi[k]));
			}
		}
	}
}

// MapManager::update_cloud_vectors (src/map_manager.cpp:258-292): every point of a linear-feature cloud gets the principal direction of its radius-limited
// k-neighbourhood (pca.hpp:209-290, :392-437) and survives only if the neighbourhood is linear enough and its direction steep (pillars) or flat (beams) enough.
// One lane per point of tile j.block; the cloud streams through LDS in 256-point tiles and every lane keeps its `max_k` nearest neighbours as a sorted list in LDS
// (slot-major, so that neighbouring lanes touch neighbouring banks).  A cloud of a few thousand points is all this ever sees (the map's pillar / beam share of
// max_num_pts): n^2 distances is microseconds.
//   neighbourhood   squared L2_Simple distance (((dx*dx)+dy*dy)+dz*dz, float) < radius^2, the max_k nearest in (distance, index) order,
//                   the point itself included — pcl::KdTreeFLANN::radiusSearch with max_nn
//   pcl::PCA        float centroid and float demeaned covariance summed in the neighbours' order, scaled by 1/(n-1); the
//                   eigen-decomposition of that float matrix in double (cyclic Jacobi), eigenvalues rounded to float
// 51 KB of LDS per workgroup (48 KB of neighbour lists, 3 KB of tile): three workgroups, twelve waves, share a CU's 160 KB.  Halving the block to 128 lanes
// halves the lists and doubles the workgroups per CU — the same twelve waves — and would stage every tile twice as often, so the block stays 256.
__global__ __launch_bounds__(256) void k_mapb_pca(const MapPcaArgs *__restrict__ ent, const MapbJob *__restrict__ jobs)
{
	__shared__ float tx[256], ty[256], tz[256];
	__shared__ float ld[MAP_PCA_K * 256];
	__shared__ uint32_t li[MAP_PCA_K * 256];
	const MapbJob j = jobs[blockIdx.x];
	const MapPcaArgs a = ent[j.ent];
	const uint32_t t = threadIdx.x, i = j.block * 256u + t;
	const bool live = i < a.n;
	float qx = 0, qy = 0, qz = 0;
	if (live)
	{
		const float4 r0 = a.recs[(size_t)i * 3];
		qx = r0.x, qy = r0.y, qz = r0.z;
	}
	const float r2 = a.radius * a.radius;
	const uint32_t K = (uint32_t)a.max_k;
	uint32_t m = 0;	   // list length
	float worst = r2; // a candidate enters while its distance is below this
	for (uint32_t base = 0; base < a.n; base += 256u)
	{
		__syncthreads();
		if (base + t < a.n)
		{
			const float4 r0 = a.recs[(size_t)(base + t) * 3];
			tx[t] = r0.x, ty[t] = r0.y, tz[t] = r0.z;
		}
		__syncthreads();
		const uint32_t cnt = min(256u, a.n - base);
		if (!live)
			continue;
		for (uint32_t jj = 0; jj < cnt; jj++)
		{
			const float dx = qx - tx[jj], dy = qy - ty[jj], dz = qz - tz[jj];
			const float d = dx * dx + dy * dy + dz * dz;
			if (!(d < worst))
				continue;
			// behind every entry with distance <= d: candidates arrive in index order, so ties stay in index order
			uint32_t pos = m < K ? m : K - 1u;
			while (pos > 0 && ld[(pos - 1u) * 256u + t] > d)
			{
				ld[pos * 256u + t] = ld[(pos - 1u) * 256u + t];
				li[pos * 256u + t] = li[(pos - 1u) * 256u + t];
				pos--;
			}
			ld[pos * 256u + t] = d;
			li[pos * 256u + t] = base + jj;
			if (m < K)
				m++;
			if (m == K)
				worst = ld[(K - 1u) * 256u + t];
		}
	}
	if (!live)
		return;
	uint8_t keep = 0;
	if (m > 3u && (int)m >= a.min_k)
	{
		float mx = 0, my = 0, mz = 0;
		for (uint32_t k = 0; k < m; k++)
		{
			const float4 r0 = a.recs[(size_t)li[k * 256u + t] * 3];
			mx += r0.x, my += r0.y, mz += r0.z;
		}
		mx /= (float)m, my /= (float)m, mz /= (float)m;
		float s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
		for (uint32_t k = 0; k < m; k++)
		{
			const float4 r0 = a.recs[(size_t)li[k * 256u + t] * 3];
			const float dx = r0.x - mx, dy = r0.y - my, dz = r0.z - mz;
			s0 += dx * dx, s1 += dx * dy, s2 += dx * dz, s3 += dy * dy, s4 += dy * dz, s5 += dz * dz;
		}
		const float alpha = 1.f / ((float)m - 1.f);
		const mulls_pca::Eig E = mulls_pca::eigen3(alpha * s0, alpha * s1, alpha * s2, alpha * s3, alpha * s4, alpha * s5);
		const float e1 = E.e1, e2 = E.e2;
		float dx = E.px, dy = E.py, dz = E.pz;
		mulls_pca::normalize3(dx, dy, dz); // Vector3f::normalize()
		const double linear_2 = ((double)e1 - (double)e2) / (double)e1; // pca_feature_t keeps eigenvalues and ratios as doubles (pca.hpp:18-40)
		if (linear_2 > (double)a.min_linearity && (fabsf(dz) > a.sin_high || fabsf(dz) < a.sin_low))
		{
			keep = 1;
			a.recs[(size_t)i * 3 + 1] = make_float4(dx, dy, dz, (float)linear_2); // assign_normal(pt, feature, false)
			float4 r2v = a.recs[(size_t)i * 3 + 2];
			r2v.y = (float)linear_2; // curvature <- linearity (:280)
			a.recs[(size_t)i * 3 + 2] = r2v;
		}
	}
	a.keep[i] = keep;
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
