// scan_launch.h — host-callable launchers of k_scan.hip: the raw-scan steps (mulls_scan_prepare) and the merged-map builder (mulls_mapper_add) over the
// frames of one sub-batch, one launch per pass.  A workgroup works on one chunk of MULLS_SCAN_CHUNK points of one frame; which frame comes from a binary
// search of blockIdx.x in the prefix table of the frames' first chunks (k_ncc_batch.hip's manner).
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "scan_math.h"

#define MULLS_SCAN_WAVES (MULLS_SCAN_CHUNK / 64u) // a chunk's survivor flags are this many 64-bit ballots

// one frame as the host describes it (uploaded in front of the flag pass; again, with out and move filled, in front of the write pass)
struct ScanFrame
{
	const float4 *in; // its n records: staged, or the caller's device cloud where it is
	float4 *out;	  // where its first kept record goes
	uint32_t n, chunk0;
	mulls::scan::FrameMove move;
};
// ... and what the device finds out about it (downloaded between the counting passes and the write pass)
struct ScanFrameStat
{
	uint32_t n_dist, n_out; // survivors of the dist filter; of those, the ones the thinning keeps
	uint32_t nan_stamp, pad;
	double first, last; // mode 1: the folds over the kept points' time stamps
};
// the arrays of a sub-batch: F frames, G chunks
struct ScanBatch
{
	const ScanFrame *frames;  // [F]
	const uint32_t *chunk0;	  // [F + 1] prefix table of the frames' chunks
	ScanFrameStat *stats;	  // [F]
	uint64_t *ballots;		  // [G * MULLS_SCAN_WAVES] the flag pass's result
	uint32_t *base;			  // [G] a chunk's first rank among its frame's survivors
	double *chunk_first, *chunk_last; // [G] mode 1
	uint32_t *chunk_nan;			  // [G]
	uint32_t F, G;
};

hipError_t launch_scan_flag(hipStream_t st, const ScanBatch &b, const mulls::scan::Prep &P);
hipError_t launch_scan_ranks(hipStream_t st, const ScanBatch &b, const mulls::scan::Prep &P);
hipError_t launch_scan_minmax(hipStream_t st, const ScanBatch &b, const mulls::scan::Prep &P);
hipError_t launch_scan_write(hipStream_t st, const ScanBatch &b, const mulls::scan::Prep &P);
