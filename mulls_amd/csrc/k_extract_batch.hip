// k_extract_batch.hip — the one kernel mulls_extract_features_batch adds to those of k_ground.hip, k_classify.hip and map_kernels.hip (which it runs through
// their table forms): a table of byte ranges copied or cleared in one launch.  What a single extraction does with a copy or fill command per array — staging the
// non-ground cloud, zeroing the grid's counters, reading a scan's counts, placing twelve clouds in a block — is one range per scan and array here.
#include <hip/hip_runtime.h>

#include "extract_launch.h"

#define EX_CHUNK 16384u // bytes per workgroup
__global__ __launch_bounds__(256) void k_ex_segs(const ExSeg *__restrict__ tab)
{
	const ExSeg s = tab[blockIdx.y]; // wave-uniform: scalar loads
	const uint32_t first = blockIdx.x * EX_CHUNK;
	if (first >= s.bytes)
		return;
	const uint32_t len = min(EX_CHUNK, s.bytes - first);
	if (((s.dst | s.src | (unsigned long long)s.bytes) & 15ull) == 0ull)
	{
		uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(s.dst + first);
		const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(s.src + first);
		for (uint32_t w = threadIdx.x; w < len / 16u; w += 256u)
			dst[w] = s.src ? src[w] : make_uint4(0u, 0u, 0u, 0u);
	}
	else
	{
		uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(s.dst + first);
		const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(s.src + first);
		for (uint32_t w = threadIdx.x; w < len / 4u; w += 256u)
			dst[w] = s.src ? src[w] : 0u;
	}
}
int launch_ex_segs(hipStream_t st, const ExSeg *tab_dev, uint32_t count, uint32_t max_bytes)
{
	if (!count || !max_bytes)
		return 0;
	hipLaunchKernelGGL(k_ex_segs, dim3((max_bytes + EX_CHUNK - 1u) / EX_CHUNK, count), dim3(256), 0, st, tab_dev);
	return 1;
}
