// pcl_icp_launch.h — what pcl_icp.cpp and k_pcl_icp.hip share: a problem's descriptor (written by the host), its record (kept by the device) and the
// launches.  The crop and the nearest-neighbour pass of the fitness are mulls_ndt's (ndt_launch.h): a problem has an NdtDesc and an NdtRec for them
// beside the structures here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/mulls_hip.h"
#include "ndt_launch.h"
#include "pcl_icp_math.h"

#define MULLS_PCL_ICP_SEG 1024u // threads of the one-workgroup-per-table scan; a table has a multiple of this many slots
#define MULLS_PCL_ICP_TILE 256u // target indices of one LDS tile of the normals kernel

// a hash table of occupied cells over one cloud, open addressing with linear probing, and the cloud's points in cell order (gicp_launch.h's GicpTab
// with a copy of the coordinates in that order).  Three per problem: the cropped target in cells of the correspondence distance, the cropped target in
// cells of the normals' radius (Point2Plane only) and the moved source in cells of the correspondence distance (reciprocal only; rebuilt every tick).
enum
{
	PCL_ICP_TAB_TGT = 0,
	PCL_ICP_TAB_NRM = 1,
	PCL_ICP_TAB_SRC = 2,
	PCL_ICP_TABS = 3
};
struct PclIcpTab
{
	uint32_t n_cap;		   // the cloud's points before the crop: the bound of every per-point loop; 0: the table is not built
	uint32_t slots, shift; // a power of two >= max(2 n_cap, MULLS_PCL_ICP_SEG); 64 - log2(slots)
	uint32_t pad;
	uint64_t o_pts;					   // packed float xyz
	uint64_t o_cell, o_list;		   // per point: its slot; the points of every slot
	uint64_t o_sorted;				   // packed float xyz in the order of o_list
	uint64_t o_keys;				   // uint64 a slot: the packed cell coordinates, all ones where free
	uint64_t o_count, o_start, o_fill; // uint32 a slot: points, first entry in list, fill counter (contiguous: cleared together)
};
struct PclIcpDesc
{
	PclIcpTab tab[PCL_ICP_TABS];
	uint32_t n_src_cap, n_tgt_cap;
	uint64_t o_src;		// the cropped source (the crop's output: read only)
	uint64_t o_mov;		// the moved source, packed float xyz
	uint64_t o_match;	// int32 a source point: its target point, -1 without a pair
	uint64_t o_d2;		// float a source point: the pair's squared distance
	uint64_t o_nrm;		// packed float xyz a target point (Point2Plane)
	uint64_t o_dist;	// float a source point: the fitness pass' nearest squared distance (NdtDesc's)
	uint64_t o_partial; // 28 x MULLS_NDT_TREE doubles
	uint64_t o_hits;	// MULLS_NDT_TREE uint32: pairs per lane
};
enum PclIcpStatus
{
	PCL_ICP_ST_OK = 0,
	PCL_ICP_ST_NONFINITE = 1,
	PCL_ICP_ST_EMPTY = 2
};
struct PclIcpRec
{
	pcl_icp::State S;
	double fitness;
	uint32_t n[2]; // points after the crop: source, target
	uint32_t n_fit, range;
	int32_t status, pad;
};
struct PclIcpOpts
{
	double inv_edge[PCL_ICP_TABS]; // of a table's cells
	double thr2, radius2, fit_range;
	double transformation_epsilon, euclidean_fitness_epsilon;
	int32_t metric, reciprocal, max_iter_num, pad;
};

// the records' start, the moved copy of the cropped source, the source's range check
hipError_t launch_pcl_icp_begin(hipStream_t st, const PclIcpDesc *desc, uint32_t P, uint32_t n_src_max, unsigned char *arena, PclIcpOpts opt, const NdtRec *nrec,
								PclIcpRec *rec, double *frames);
// one table of every problem: (the clear, when `clear`,) cells, the scan, the scatter
hipError_t launch_pcl_icp_table(hipStream_t st, const PclIcpDesc *desc, uint32_t P, int tb, uint32_t n_max, uint32_t slots_max, bool clear, unsigned char *arena,
								PclIcpOpts opt, PclIcpRec *rec);
// the target's normals: every cell's list ascending, then a workgroup per cell
hipError_t launch_pcl_icp_normals(hipStream_t st, const PclIcpDesc *desc, uint32_t P, uint32_t slots_max, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *rec);
hipError_t launch_pcl_icp_search(hipStream_t st, const PclIcpDesc *desc, uint32_t P, uint32_t n_src_max, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *rec);
hipError_t launch_pcl_icp_accum(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *rec);
// *running: += the problems still running; *next: set to 0 (the word of the tick after)
hipError_t launch_pcl_icp_decide(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec, double *frames,
								 uint32_t *running, uint32_t *next);
// after launch_ndt_fitness has left the nearest squared distances: the thresholded mean
hipError_t launch_pcl_icp_fitness(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec);
