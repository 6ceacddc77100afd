// nms_launch.h — host-callable launchers of k_nms.hip: CFilter::non_max_suppress (cfilter.hpp:1183-1312) on a cloud that is already in visiting order
// (include/mulls_hip.h has the definition).  The multi-launch path uses classify_launch.h's launchers instead; k_nms.hip holds the one-workgroup path.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mulls_hip.h"
#include "nms_batch.h"

#define MULLS_NMS_BLOCK 1024u // lanes of the one workgroup
#define MULLS_NMS_LIST_CAP 8u // earlier neighbours a point keeps in LDS; a point with more walks its cells' buckets in every round
// buckets of the one-workgroup path's hashed grid: the power of two that is at least n (and at least 64)
inline uint32_t nms_buckets(uint32_t n) { return nms_batch_buckets(n); } // (nms_batch.h: the planner writes it into the problems' records)
// dynamic LDS of the one-workgroup path: x, y, z (floats), the list (16-bit positions), the position in bucket order (16 bits), the state byte and the
// list's fill byte per point; the buckets' ends
inline size_t nms_lds_bytes(uint32_t n) { return (size_t)n * (12u + 2u * MULLS_NMS_LIST_CAP + 2u + 1u + 1u) + ((size_t)nms_buckets(n) + 1u) * 4u; }
static_assert(MULLS_NMS_LDS_MAX_POINTS == 4096u, "the limit below is worked out for 4096 points: 4096 * 32 + 4097 * 4 = 147460 bytes, under the 160 KiB of a CU");
static_assert(MULLS_NMS_LDS_MAX_POINTS <= 65536u, "16-bit positions");

// what the one-workgroup kernel leaves for the host (one download, with the kept positions behind it)
struct NmsHeader
{
	uint32_t n_kept, rounds;
	uint32_t pad[2];
};

// keys[i] = normal[3] of record i of a device cloud of 48-byte records; *bad |= 1 where a coordinate is not finite (the caller zeroes it)
hipError_t launch_nms_keys(hipStream_t st, const void *recs, uint32_t n, float *keys, uint32_t *bad);
// The whole suppression of n <= MULLS_NMS_LDS_MAX_POINTS records in visiting order in one workgroup: hdr->n_kept, hdr->rounds, kept_pos[0 .. n_kept) = the
// kept records' positions in visiting order, ascending; out (may be NULL) = the first min(n_kept, out_cap) kept records
hipError_t launch_nms_one(hipStream_t st, const float4 *recs, uint32_t n, float radius, NmsHeader *hdr, uint32_t *kept_pos, float4 *out, uint32_t out_cap);

// ---- mulls_non_max_suppress_batch: the launches of one sub-batch (nms_batch.h: the arena `L` lays out; the head has been uploaded)
// keys[i] and the non-finite flag (one word per cloud at L.o_bad, zeroed by the caller) of every device-resident cloud
hipError_t launch_nms_batch_keys(hipStream_t st, unsigned char *arena, const NmsBatchLayout &L);
// the records of the device-resident one-workgroup clouds in visiting order, from the uploaded permutations
hipError_t launch_nms_batch_gather(hipStream_t st, unsigned char *arena, const NmsBatchLayout &L);
// the suppression of every problem of L.desc, one workgroup each: headers, kept positions, and the kept records compact at L.o_out (the cursor at L.o_cursor
// zeroed by the caller); one launch, its LDS sized by the largest cloud
hipError_t launch_nms_batch(hipStream_t st, unsigned char *arena, const NmsBatchLayout &L, float radius);
