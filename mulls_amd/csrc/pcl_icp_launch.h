// pcl_icp_launch.h — what pcl_icp.cpp and k_pcl_icp.hip share: a problem's descriptor (written by the host), its record (kept by the device) and the
// launches.  The crop and the nearest-neighbour pass of the fitness are mulls_ndt's (ndt_launch.h): a problem has an NdtDesc and an NdtRec for them
// beside the structures here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/mulls_hip.h"
#include "ndt_launch.h"
#include "pcl_icp_math.h"
#include "reg_launch.h"

#define MULLS_PCL_ICP_TILE 256u // target indices of one LDS tile of the normals kernel

// Three cell tables (reg_table.h) per problem, each with a copy of the coordinates in cell order: the cropped target in cells of the correspondence
// distance, the cropped target in cells of the normals' radius (Point2Plane only) and the moved source in cells of the correspondence distance
// (reciprocal only; rebuilt every tick, and a moved point outside the cells' range takes no part instead of refusing the problem).
enum
{
	PCL_ICP_TAB_TGT = 0,
	PCL_ICP_TAB_NRM = 1,
	PCL_ICP_TAB_SRC = 2,
	PCL_ICP_TABS = 3
};
struct PclIcpDesc
{
	uint32_t n_src_cap, n_tgt_cap;
	uint64_t o_src, o_tgt; // the cropped clouds (the crop's output: read only)
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
	uint32_t n_fit, pad;
};
struct PclIcpOpts
{
	double thr2, radius2, fit_range;
	double transformation_epsilon, euclidean_fitness_epsilon;
	int32_t metric, reciprocal, max_iter_num, pad;
};

// The head's status is a PclIcpStatus; the problem's tables are tabs[MULLS_REG_TABS * p + PCL_ICP_TAB_*].
// the records' start, the moved copy of the cropped source, the source's range check
hipError_t launch_pcl_icp_begin(hipStream_t st, const PclIcpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t n_src_max, unsigned char *arena, const NdtRec *nrec,
								PclIcpRec *rec, RegHead *head, double *frames);
// the target's normals: every cell's list ascending, then a workgroup per cell
hipError_t launch_pcl_icp_normals(hipStream_t st, const PclIcpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t slots_max, unsigned char *arena, PclIcpOpts opt,
								  const RegHead *head);
hipError_t launch_pcl_icp_search(hipStream_t st, const PclIcpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t n_src_max, unsigned char *arena, PclIcpOpts opt,
								 const PclIcpRec *rec, const RegHead *head);
hipError_t launch_pcl_icp_accum(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *rec, const RegHead *head);
// *running: += the problems still running; *next: set to 0 (the word of the tick after)
hipError_t launch_pcl_icp_decide(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec, RegHead *head,
								 double *frames, uint32_t *running, uint32_t *next);
// after launch_ndt_fitness has left the nearest squared distances: the thresholded mean
hipError_t launch_pcl_icp_fitness(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec, const RegHead *head);
