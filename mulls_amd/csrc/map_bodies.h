// map_bodies.h — the arithmetic of the local map's kernels as __device__ bodies, so that the one-map launches (map_kernels.hip, k_transform_clouds of k_reduce.hip)
// and the table-driven launches of mulls_map_update_batch (k_map_batch.hip) are one text: a batch returns the bytes of the single calls because both run these
// lines.  A body gets what its kernel found out about its share of the work (which cloud, which block of it) and the LDS arrays the kernel declared.
#pragma once
#include <hip/hip_runtime.h>

#include "map_launch.h"
#include "pca_device.h"

// (MAP_NN_CHUNK, the tree points per workgroup: map_launch.h — the hosts size their grids and job lists by it)
#define MAP_NN_TILE 1024u
#define MAP_PCA_K 24 // list slots per lane (max_k <= 24: 48 KB of lists per workgroup)

namespace map_body
{
__device__ __forceinline__ uint32_t float_ord(float f)
{
	const uint32_t u = __float_as_uint(f);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// pcl::transformPointCloudWithNormals on record i: double arithmetic, float store; T = rows of [R|t]
__device__ __forceinline__ void transform(float4 *__restrict__ recs, uint32_t i, const double *T)
{
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

// get_cloud_bbx (utility.hpp:817-848) over records [i0, i1) in steps of `step` (256 lanes), and over the same points moved by pose_lo
// (pcl::transformPointCloud: double arithmetic, float store) — ordered-uint atomics; NaN coordinates never win a comparison in the reference and are skipped
// here.  keys: [0..2] min xyz, [3..5] max xyz, [6..8] posed min, [9..11] posed max.
__device__ __forceinline__ void bbox(const float4 *__restrict__ recs, uint32_t i0, uint32_t i1, uint32_t step, const double *pose, uint32_t *keys)
{
	float lo[6], hi[6];
	for (int k = 0; k < 6; k++)
	{
		lo[k] = __builtin_inff();
		hi[k] = -__builtin_inff();
	}
	for (uint32_t i = i0; i < i1; i += step)
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

// Exact nearest tree point (FLANN L2_Simple<float> distance) of the 256 frame points of block `fblock`, among the MAP_NN_CHUNK tree points of chunk `tchunk`
// staged through LDS (tile: MAP_NN_TILE float4); atomicMin on the float bits combines the chunks (distances are >= 0).
__device__ __forceinline__ void nn(const float4 *__restrict__ frame, uint32_t n_frame, const float4 *__restrict__ tree, uint32_t n_tree, int use_box, double b0,
								   double b1, double b2, double b3, double b4, double b5, uint32_t *__restrict__ best, uint32_t fblock, uint32_t tchunk, float4 *tile)
{
	const uint32_t q = fblock * blockDim.x + threadIdx.x;
	float qx = 0, qy = 0, qz = 0;
	if (q < n_frame)
	{
		const float4 p = frame[(size_t)q * 3];
		qx = p.x, qy = p.y, qz = p.z;
	}
	float d_best = __builtin_inff();
	const uint32_t t0 = tchunk * MAP_NN_CHUNK, t1 = min(n_tree, t0 + MAP_NN_CHUNK);
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

// map_scan_feature_pts_distance_removal's keep rule (map_manager.cpp:246-256) for frame point q, all in float as written there
__device__ __forceinline__ void keep(const float4 *__restrict__ frame, uint32_t q, const uint32_t *__restrict__ best, float center_radius, float dmin, float dmax,
									 float near, uint8_t *__restrict__ keep_out)
{
	const float4 p = frame[(size_t)q * 3];
	bool k = true;
	if (!(p.x * p.x + p.y * p.y > center_radius * center_radius))
	{
		const uint32_t bits = best[q];
		if (bits != 0x7f800000u) // an empty tree leaves the cloud alone (see oracle)
		{
			const float d2 = __uint_as_float(bits);
			k = (d2 > near * near && d2 < dmin * dmin) || d2 > dmax * dmax;
		}
	}
	keep_out[q] = k ? 1 : 0;
}

// MapManager::update_cloud_vectors for the 256 points of tile `tile_idx` of a linear-feature cloud (see k_map_pca, map_kernels.hip).  tx ty tz: 256 floats each,
// ld li: MAP_PCA_K * 256 each, all LDS.
__device__ __forceinline__ void pca(const MapPcaArgs &a, uint32_t tile_idx, float *tx, float *ty, float *tz, float *ld, uint32_t *li)
{
	const uint32_t t = threadIdx.x, i = tile_idx * 256u + t;
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
		for (uint32_t j = 0; j < cnt; j++)
		{
			const float dx = qx - tx[j], dy = qy - ty[j], dz = qz - tz[j];
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
			li[pos * 256u + t] = base + j;
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
} // namespace map_body
