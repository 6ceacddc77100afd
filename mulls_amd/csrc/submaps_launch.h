// submaps_launch.h — host-callable launchers of k_submaps.hip: the bounds of many submaps of the device-resident archive (mulls_submaps_*) in one launch set
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

// Submaps [first, first + n) of one arena.  A job is MULLS_SUBMAP_CHUNK records of one submap; job_first[s] counts the jobs of the submaps before s, so the
// jobs of the call are job_first[first] .. job_first[first + n) and an empty submap has none.
struct SubmapBoundsArgs
{
	const float4 *recs;		   // the arena, 3 float4 per record
	const uint32_t *sub_off;   // [count + 1] first record of every submap
	const uint32_t *job_first; // [count + 1]
	const double *poses;	   // [12 n] rows of [R|t] of submap first + k
	uint32_t *keys;			   // [per n] ordered-uint keys, per = 6 (posed min xyz, max xyz) or 12 (the stored points' first)
	double *out;			   // [per n] the same as doubles, (DBL_MAX, -DBL_MAX) where nothing won
	uint32_t first, n;
	int with_local; // 1: per = 12
};
// three launches on st: keys to "nothing won", the jobs, keys to doubles
void launch_submap_bounds(hipStream_t st, const SubmapBoundsArgs &a, uint32_t n_jobs);
// n records of `stride` bytes (a multiple of 4) at src to packed 48-byte records at dst, both device memory
void launch_submap_gather(hipStream_t st, float4 *dst, const void *src, uint32_t stride, uint32_t n);
