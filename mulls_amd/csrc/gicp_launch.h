// gicp_launch.h — what gicp.cpp and k_gicp.hip share: a problem's descriptor (written by the host), its record (kept by the device) and the launches.
// The crop and the fitness pass are mulls_ndt's (ndt_launch.h): a problem has an NdtDesc and an NdtRec for them beside the structures here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/mulls_hip.h"
#include "gicp_math.h"
#include "ndt_launch.h"

#define MULLS_GICP_MAX_RING 3 // Chebyshev rings a neighbour query walks before it leaves for the brute-force kernel: at most 7^3 cells
#define MULLS_GICP_SEG 1024u  // threads of the one-workgroup-per-table scan; a table has a multiple of this many slots

// a hash table of occupied cells over one cropped cloud, open addressing with linear probing, and the cloud's points in cell order.
// Three per problem: the neighbour grid of the source, that of the target (cells of knn_edge) and the voxel map of the target.
enum
{
	GICP_TAB_KNN_SRC = 0,
	GICP_TAB_KNN_TGT = 1,
	GICP_TAB_VOXEL = 2,
	GICP_TABS = 3
};
struct GicpTab
{
	uint32_t n_cap;		   // the cloud's points before the crop: the bound of every per-point loop
	uint32_t slots, shift; // a power of two >= max(2 n_cap, MULLS_GICP_SEG); 64 - log2(slots)
	uint32_t pad;
	uint64_t o_pts;						   // packed float xyz (the cropped cloud)
	uint64_t o_cell, o_list;			   // per point: its slot; the points of every slot
	uint64_t o_keys;					   // uint64 a slot: the packed cell coordinates, all ones where free
	uint64_t o_count, o_start, o_fill;	   // uint32 a slot: points, first entry in list, fill counter
};
struct GicpDesc
{
	GicpTab tab[GICP_TABS];
	uint64_t o_cov[2];	// 6 doubles a point: source, target
	uint64_t o_left[2]; // uint32 a point: the queries the ring walk did not certify
	uint64_t o_vox;		// 9 doubles (mean, cov) of a slot of the voxel map at index start[slot]
	uint64_t o_partial; // 28 x MULLS_NDT_TREE doubles
	uint64_t o_hits;	// MULLS_NDT_TREE uint32: points with a voxel, per lane
};
enum GicpStatus
{
	GICP_ST_OK = 0,
	GICP_ST_NONFINITE = 1,
	GICP_ST_RANGE = 2,
	GICP_ST_FEW = 3
};
struct GicpRec
{
	gicp::State S;
	uint32_t n[2];		// points after the crop: source, target
	uint32_t n_left[2]; // queries left for the brute-force kernel
	uint32_t n_voxels, range;
	int32_t status, pad;
};
struct GicpOpts
{
	double knn_edge, knn_inv_edge;
	double rotation_epsilon, transformation_epsilon;
	float resolution;
	float start_rotvec[3];
	int32_t k, max_iterations;
};

hipError_t launch_gicp_begin(hipStream_t st, uint32_t P, const NdtRec *nrec, GicpRec *rec, double *frames, GicpOpts opt);
// the three tables of every problem: cells, the scan, the scatter
hipError_t launch_gicp_tables(hipStream_t st, const GicpDesc *desc, uint32_t P, uint32_t n_max, unsigned char *arena, GicpOpts opt, GicpRec *rec);
// the ring walk of every point of both clouds; *max_left: the largest number of queries a cloud left uncertified
hipError_t launch_gicp_knn(hipStream_t st, const GicpDesc *desc, uint32_t P, uint32_t n_max, unsigned char *arena, GicpOpts opt, GicpRec *rec, uint32_t *max_left);
hipError_t launch_gicp_brute(hipStream_t st, const GicpDesc *desc, uint32_t P, uint32_t max_left, unsigned char *arena, GicpOpts opt, const GicpRec *rec);
hipError_t launch_gicp_voxels(hipStream_t st, const GicpDesc *desc, uint32_t P, uint32_t slots_max, unsigned char *arena, const GicpRec *rec);
hipError_t launch_gicp_eval(hipStream_t st, const GicpDesc *desc, uint32_t P, unsigned char *arena, GicpOpts opt, const GicpRec *rec);
hipError_t launch_gicp_decide(hipStream_t st, const GicpDesc *desc, uint32_t P, unsigned char *arena, GicpOpts opt, GicpRec *rec, double *frames, uint32_t *running);
