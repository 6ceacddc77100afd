// k_pair_gather.hip — the one gather of the coarse-registration solvers' staging (pair_stage.h) for gfx950: the four live floats of the pairs out of
// device-resident clouds of 48-byte records, optionally through an index list, into the problems' points.  One launch runs a list of jobs (pair_gather.h):
// the second grid axis is the job, the first is sized for the largest one.
#include <hip/hip_runtime.h>

#include "pair_stage.h"

namespace
{
__global__ void __launch_bounds__(256) k_pair_gather(const PairGather *__restrict__ jobs, unsigned char *arena)
{
	const PairGather J = jobs[blockIdx.y];
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= J.n)
		return;
	const size_t r = J.indexed ? (size_t)(uint32_t) reinterpret_cast<const int32_t *>(arena + J.idx)[i] : (size_t)i; // (the host has checked every index against its cloud)
	reinterpret_cast<float4 *>(arena + J.out)[i] = *reinterpret_cast<const float4 *>(J.recs + r * 48u);
}
} // namespace

hipError_t launch_pair_gather(hipStream_t st, const PairGather *jobs, uint32_t n_jobs, uint32_t n_max, unsigned char *arena)
{
	if (!n_jobs || !n_max)
		return hipSuccess;
	hipLaunchKernelGGL(k_pair_gather, dim3((n_max + 255u) / 256u, n_jobs), dim3(256), 0, st, jobs, arena);
	return hipGetLastError();
}
