// ndt_tree.h — the halving tree over MULLS_NDT_TREE strided partial sums, device only: k_ndt.hip (the 28 sums, the fitness) and k_gicp.hip (the 28 sums)
// expand the same text, so a sum has the same bits in both
#pragma once
#include <hip/hip_runtime.h>

#include "ndt_launch.h"

namespace
{
// the pairwise tree over MULLS_NDT_TREE partials held as r[16] per thread of a 256-thread workgroup (r[m] = partial[t + 256 m]); the sum in every thread
__device__ inline double tree_of_partials(double *r, double *s_p)
{
	const uint32_t t = threadIdx.x;
#pragma unroll
	for (int h = 8; h >= 1; h >>= 1) // the levels w = 2048 .. 256: partner l + w of l = t + 256 m is held by the same thread
#pragma unroll
		for (int m = 0; m < h; m++)
			r[m] += r[m + h];
	__syncthreads();
	s_p[t] = r[0];
	__syncthreads();
	for (uint32_t w = 128; w >= 1; w >>= 1)
	{
		if (t < w)
			s_p[t] += s_p[t + w];
		__syncthreads();
	}
	return s_p[0];
}
} // namespace
