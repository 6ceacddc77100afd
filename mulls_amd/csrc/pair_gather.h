// pair_gather.h — the gather job the two coarse-registration solvers (ransac.cpp, teaser.cpp) stage their device-resident clouds with.  Host code without
// HIP, so that the planners (ransac_batch.h, teaser_batch.h) and their harnesses under tests/ can size the job tables on the CPU.  pair_stage.h has the
// staging that fills the jobs, k_pair_gather.hip the kernel that runs them.
#pragma once
#include <stdint.h>

// a gather of a device-resident cloud into a problem's points: out[i] = x, y, z, data[3] of record idx[i] (i when not indexed)
struct PairGather
{
	const unsigned char *recs; // the cloud: 48-byte records in device memory
	uint64_t idx, out;		   // arena offsets: n int32 (read when indexed), n float4
	uint32_t n, indexed;
};
