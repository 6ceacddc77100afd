// teaser_device.h — the device helpers that k_teaser.hip (one problem per call) and k_teaser_batch.hip (many problems per launch) share, so that both compile
// one text of the measurement order and of the summation tree (include/mulls_hip.h: mulls_coarse_reg_teaser, "measures" and "rotation").
#pragma once
#include <hip/hip_runtime.h>

#include "teaser_math.h"

namespace
{
constexpr int WAVE = 64;
constexpr uint32_t P = MULLS_TEASER_PARTIALS;
constexpr int RT = 1024; // threads of the single-workgroup kernels
static_assert(P == 4u * RT, "the reductions fold four partials per thread before the LDS tree");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
	for (int off = WAVE / 2; off > 0; off >>= 1)
		v += __shfl_xor(v, off, WAVE);
	return v;
}

// measurement k: a = s[c_b] - s[c_a], b = t[c_b] - t[c_a], widened first
__device__ __forceinline__ void measurement(const float4 *cs, const float4 *ct, uint32_t C, uint64_t k, double *a, double *b)
{
	uint32_t ia, ib;
	teaser_decode(k, C, &ia, &ib);
	const float4 s0 = cs[ia], s1 = cs[ib], t0 = ct[ia], t1 = ct[ib];
	a[0] = (double)s1.x - (double)s0.x, a[1] = (double)s1.y - (double)s0.y, a[2] = (double)s1.z - (double)s0.z;
	b[0] = (double)t1.x - (double)t0.x, b[1] = (double)t1.y - (double)t0.y, b[2] = (double)t1.z - (double)t0.z;
}

// the pairwise tree over P partials: p[t] += p[t + s], s = P / 2, ..., 1 — the two widest levels in registers, the rest in LDS
__device__ double tree_sum(const double *part, double *red)
{
	const int t = threadIdx.x;
	const double v = (part[t] + part[t + 2 * RT]) + (part[t + RT] + part[t + 3 * RT]);
	__syncthreads(); // (red may still be read by the previous sum)
	red[t] = v;
	__syncthreads();
	for (int s = RT / 2; s > 0; s >>= 1)
	{
		if (t < s)
			red[t] = red[t] + red[t + s];
		__syncthreads();
	}
	return red[0];
}
} // namespace
