// k_submaps.hip — kernels of the device-resident submap archive (include/mulls_hip.h, "the submap archive"): CloudUtility::get_cloud_bbx
// (utility.hpp:817-847) over the records of many submaps at once, as stored and moved by each submap's pose_lo (pcl::transformPointCloud with a Matrix4d:
// double arithmetic, float store), and the gather of a strided device cloud into packed records.  One workgroup takes one job of MULLS_SUBMAP_CHUNK records
// of one submap, reduces it with wave shuffles and LDS and combines into the submap's keys with ordered-integer atomic min / max: minima and maxima are exact
// in any order, so nothing depends on the job size or on which workgroup arrives first.
#include <hip/hip_runtime.h>

#include "../../include/mulls_hip.h"
#include "submaps_launch.h"

namespace
{
constexpr uint32_t BLOCK = 256u, WAVES = BLOCK / 64u;
static_assert(MULLS_SUBMAP_CHUNK % BLOCK == 0, "a job is a whole number of passes of the workgroup");

// floats in an order unsigned integers share (map_kernels.hip's float_ord)
__device__ __forceinline__ uint32_t float_ord(float f)
{
	const uint32_t u = __float_as_uint(f);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// keys[k]: a minimum's "nothing won" is the largest key, a maximum's the smallest; +inf never becomes a minimum and -inf never a maximum under
// get_cloud_bbx's comparisons with +-DBL_MAX, so neither value can be mistaken for a winner
__global__ __launch_bounds__(BLOCK) void k_submap_keys_init(uint32_t *keys, uint32_t total)
{
	const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
	if (k < total)
		keys[k] = (k % 6u) < 3u ? 0xffffffffu : 0u;
}

__global__ __launch_bounds__(BLOCK) void k_submap_keys_out(const uint32_t *keys, double *out, uint32_t total)
{
	const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
	if (k >= total)
		return;
	const bool is_min = (k % 6u) < 3u;
	const uint32_t key = keys[k];
	if (is_min ? key == 0xffffffffu : key == 0u)
		out[k] = is_min ? 1.7976931348623157e308 : -1.7976931348623157e308;
	else
		out[k] = (double)ord_float(key);
}

// NV = 3: the posed points; NV = 6: the stored points (values 0..2) and the posed points (3..5)
template <int NV>
__global__ __launch_bounds__(BLOCK) void k_submap_bounds(SubmapBoundsArgs a)
{
	__shared__ float red[WAVES][2 * NV];
	// the job's submap: the last s in [first, first + n) with job_first[s] <= job (an empty submap shares its job_first with its successor and is never found)
	const uint32_t job = a.job_first[a.first] + blockIdx.x;
	uint32_t lo_s = a.first, hi_s = a.first + a.n; // job_first[lo_s] <= job < job_first[hi_s]
	while (hi_s - lo_s > 1u)
	{
		const uint32_t mid = lo_s + (hi_s - lo_s) / 2u;
		if (a.job_first[mid] <= job)
			lo_s = mid;
		else
			hi_s = mid;
	}
	const uint32_t s = lo_s;
	const uint32_t begin = a.sub_off[s] + (job - a.job_first[s]) * MULLS_SUBMAP_CHUNK;
	const uint32_t end = min(a.sub_off[s + 1u], begin + MULLS_SUBMAP_CHUNK);
	const double *P = a.poses + (size_t)(s - a.first) * 12u;
	const double m00 = P[0], m01 = P[1], m02 = P[2], m03 = P[3], m10 = P[4], m11 = P[5], m12 = P[6], m13 = P[7], m20 = P[8], m21 = P[9], m22 = P[10], m23 = P[11];

	float lo[NV], hi[NV];
	for (int k = 0; k < NV; k++)
	{
		lo[k] = __builtin_inff();
		hi[k] = -__builtin_inff();
	}
	for (uint32_t i = begin + threadIdx.x; i < end; i += BLOCK)
	{
		const float4 p = a.recs[(size_t)i * 3u];
		const double x = p.x, y = p.y, z = p.z;
		float v[NV];
		int o = 0;
		if (NV == 6)
		{
			v[0] = p.x, v[1] = p.y, v[2] = p.z;
			o = 3;
		}
		v[o] = (float)(m00 * x + m01 * y + m02 * z + m03);
		v[o + 1] = (float)(m10 * x + m11 * y + m12 * z + m13);
		v[o + 2] = (float)(m20 * x + m21 * y + m22 * z + m23);
		for (int k = 0; k < NV; k++)
		{
			lo[k] = fminf(lo[k], v[k]); // (a NaN operand is dropped)
			hi[k] = fmaxf(hi[k], v[k]);
		}
	}
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (int k = 0; k < NV; k++)
	{
		for (int off = 32; off > 0; off >>= 1)
		{
			lo[k] = fminf(lo[k], __shfl_down(lo[k], off));
			hi[k] = fmaxf(hi[k], __shfl_down(hi[k], off));
		}
		if (lane == 0)
		{
			red[wave][k] = lo[k];
			red[wave][NV + k] = hi[k];
		}
	}
	__syncthreads();
	if (threadIdx.x < 2u * NV)
	{
		const uint32_t t = threadIdx.x;
		const bool is_min = t < (uint32_t)NV;
		float r = red[0][t];
		for (uint32_t w = 1; w < WAVES; w++)
			r = is_min ? fminf(r, red[w][t]) : fmaxf(r, red[w][t]);
		// key slots of a group of three values: [min xyz, max xyz]
		const uint32_t val = is_min ? t : t - NV, group = val / 3u, ax = val % 3u;
		uint32_t *key = a.keys + (size_t)(s - a.first) * (2u * NV) + group * 6u + (is_min ? 0u : 3u) + ax;
		if (is_min)
		{
			if (r < __builtin_inff())
				atomicMin(key, float_ord(r));
		}
		else if (r > -__builtin_inff())
			atomicMax(key, float_ord(r));
	}
}

__global__ __launch_bounds__(BLOCK) void k_submap_gather(uint32_t *dst, const unsigned char *src, uint32_t stride, uint32_t n)
{
	const size_t total = (size_t)n * 12u;
	for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK)
	{
		const size_t rec = i / 12u, w = i % 12u;
		dst[i] = reinterpret_cast<const uint32_t *>(src + rec * stride)[w];
	}
}
} // namespace

void launch_submap_bounds(hipStream_t st, const SubmapBoundsArgs &a, uint32_t n_jobs)
{
	const uint32_t total = a.n * (a.with_local ? 12u : 6u);
	if (!total)
		return;
	const uint32_t kb = (total + BLOCK - 1u) / BLOCK;
	hipLaunchKernelGGL(k_submap_keys_init, dim3(kb), dim3(BLOCK), 0, st, a.keys, total);
	if (n_jobs)
	{
		if (a.with_local)
			hipLaunchKernelGGL(k_submap_bounds<6>, dim3(n_jobs), dim3(BLOCK), 0, st, a);
		else
			hipLaunchKernelGGL(k_submap_bounds<3>, dim3(n_jobs), dim3(BLOCK), 0, st, a);
	}
	hipLaunchKernelGGL(k_submap_keys_out, dim3(kb), dim3(BLOCK), 0, st, (const uint32_t *)a.keys, a.out, total);
}

void launch_submap_gather(hipStream_t st, float4 *dst, const void *src, uint32_t stride, uint32_t n)
{
	if (!n)
		return;
	const size_t total = (size_t)n * 12u;
	const uint32_t blocks = (uint32_t)std::min<size_t>((total + BLOCK - 1u) / BLOCK, 65536u);
	hipLaunchKernelGGL(k_submap_gather, dim3(blocks), dim3(BLOCK), 0, st, reinterpret_cast<uint32_t *>(dst), static_cast<const unsigned char *>(src), stride, n);
}
