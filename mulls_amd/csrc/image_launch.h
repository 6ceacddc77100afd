// image_launch.h — host-callable launchers of k_image.hip: the centre points, the 2-D map images and the range images of the scans of one sub-batch, one
// launch per pass.  A workgroup of the per-point passes works on one chunk of MULLS_SCAN_CHUNK points of one scan; which scan comes from a binary search
// of blockIdx.x in the prefix table of the scans' first chunks (k_scan.hip's manner).
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "image_math.h"

// one scan as the host describes it
struct ImageScan
{
	const float4 *in; // its n records: staged, or the caller's device cloud where it is
	uint32_t n, chunk0;
};
// what the device finds out about a scan (downloaded in front of the images)
struct ImageStat
{
	double centre[3];
	uint32_t counted, skipped_height, skipped_frame, pad;
};
// the arrays of a sub-batch: S scans, G chunks.  The 32-bit words [counters | counts | words] are one zeroed range, [stats | bev | range] one download.
struct ImageBatch
{
	const ImageScan *scans;	 // [S]
	const uint32_t *chunk0;	 // [S + 1] prefix table of the scans' chunks
	double *partial;		 // [S * 3 * MULLS_NDT_TREE] the centre's strided partial sums
	uint32_t *counters;		 // [S * 4] counted, skipped by height, skipped by the frame, unused
	int32_t *counts;		 // [S * map pixels] (2-D map images asked for)
	uint32_t *words;		 // [S * range pixels] (index << 8) | value (range images asked for)
	ImageStat *stats;		 // [S]
	uint8_t *bev, *range;	 // [S * map pixels], [S * range pixels]
	uint32_t S, G;
	uint32_t map_pixels, range_pixels; // per scan; 0: that image is not asked for
};

hipError_t launch_image_centre(hipStream_t st, const ImageBatch &b);
hipError_t launch_image_count(hipStream_t st, const ImageBatch &b, const mulls::image::Map2d &M, int form /* 1 or 2 */);
hipError_t launch_image_range(hipStream_t st, const ImageBatch &b, const mulls::image::Range &R);
hipError_t launch_image_convert(hipStream_t st, const ImageBatch &b, const mulls::image::Map2d &M);
