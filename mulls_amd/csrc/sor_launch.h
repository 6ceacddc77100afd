// sor_launch.h — host-callable launchers of k_sor.hip: the statistical outlier removal, CFilter::sor_filter (cfilter.hpp:204-247), whose body is
// pcl::StatisticalOutlierRemoval: an exact, unbounded (mean_k + 1)-nearest-neighbour query for every point of a large sparse cloud, then a two-pass
// statistic (include/mulls_hip.h has the definition).  The index is a hash of occupied cells; every loop of every kernel is bounded by a launch argument
// or a constant, never by what the coordinates happen to be.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "sor_math.h"

#define MULLS_SOR_CELL_BITS 21		  // a cell coordinate's bits in the packed 63-bit key
#define MULLS_SOR_MAX_RING 3		  // Chebyshev rings a query walks on one grid level: at most 7^3 cells
#define MULLS_SOR_SCAN_BUDGET 8192u	  // points a query may visit on one grid level before it leaves for the next
#define MULLS_SOR_LEVELS 3			  // grid levels, each four times the edge of the one before; what they leave goes to k_sor_brute
#define MULLS_SOR_PROBES 128u		  // queries answered by brute force up front: their mean_k-th neighbour distance sets the cell edge
#define MULLS_SOR_EMPTY 0xffffffffffffffffull

// the occupied-cell hash of one level and the points in cell order
struct SorGrid
{
	double lo[3];	 // the cloud's minimum corner
	double edge, inv_edge;
	uint64_t *keys;	 // [slots] packed cell coordinates, MULLS_SOR_EMPTY where free (open addressing, linear probing)
	uint32_t *start; // [slots + 1] the exclusive scan of the cells' counts: cell of slot s holds sorted[start[s] .. start[s + 1])
	const float4 *sorted; // x, y, z, original index
	uint32_t slots;
};
// what the device leaves for the host (one download, together with the index list and the distances behind it)
struct SorHeader
{
	double mean, stddev, threshold;
	uint32_t n_kept, bad;			  // bad: a non-finite coordinate was seen
	uint32_t lo_enc[3], hi_enc[3];	  // the bounding box as order-preserving integers (atomic min / max)
	uint32_t n_left[MULLS_SOR_LEVELS]; // queries each grid level left uncertified
	uint32_t overflow;				  // a cell coordinate did not fit the packed key
	uint32_t pad[2];
};

// out[i] = x, y, z of record i of a device cloud of 48-byte records, w = i
hipError_t launch_sor_gather(hipStream_t st, const void *recs, uint32_t n, float4 *out);
// hdr->lo / hi = the bounding box, hdr->bad = 1 if a coordinate is not finite (the call zeroes and seeds the header itself)
hipError_t launch_sor_bounds(hipStream_t st, const float4 *pts, uint32_t n, SorHeader *hdr);
// exact answer of query qidx[b], one wavefront each, over pts[0], pts[step], pts[2 step], ...: the kk smallest squared distances by rank counting.
// dist (may be NULL): dist[qidx[b]] = the mean distance; kth (may be NULL): kth[b] = the kk-th smallest squared distance
hipError_t launch_sor_brute(hipStream_t st, const float4 *pts, uint32_t n, uint32_t step, const uint32_t *qidx, uint32_t nq, int kk, float *dist, float *kth);
// one grid level: keys / counts of the cells (tables cleared by the call), then the scan and the scatter into cell order
hipError_t launch_sor_build(hipStream_t st, const float4 *pts, uint32_t n, SorGrid G, float4 *sorted, uint32_t *slot_of, uint32_t *counts, uint32_t *scan_tmp,
							SorHeader *hdr);
// the grid walk of nq queries (qidx == NULL: every point, in cell order); uncertified queries are appended to left[*n_left ..]
hipError_t launch_sor_search(hipStream_t st, SorGrid G, const float4 *pts, const uint32_t *qidx, uint32_t nq, int kk, float *dist, uint32_t *left, uint32_t *n_left);
// statistics in the defined order, the keep flags, their stable compaction: hdr->mean .. n_kept, kept_idx[0 .. n_kept)
hipError_t launch_sor_finish(hipStream_t st, const float *dist, uint32_t n, double std_mul, double *partials, uint32_t *flags, uint32_t *pos, uint32_t *scan_tmp,
							 int32_t *kept_idx, SorHeader *hdr);
// out[j] = record kept_idx[j] of a device cloud, all 48 bytes, j < n_kept
hipError_t launch_sor_emit(hipStream_t st, const void *recs, const int32_t *kept_idx, uint32_t n_kept, void *out);
// exclusive scan of in[0 .. m) into out[0 .. m], out[m] = the total; tmp holds m / 4096 + 2 entries
hipError_t launch_sor_scan(hipStream_t st, const uint32_t *in, uint32_t m, uint32_t *out, uint32_t *tmp);
