// gicp_launch.h — what gicp.cpp and k_gicp.hip share: a problem's descriptor (written by the host), its record (kept by the device) and the launches.
// The crop and the fitness pass are mulls_ndt's (ndt_launch.h): a problem has an NdtDesc and an NdtRec for them beside the structures here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/mulls_hip.h"
#include "gicp_math.h"
#include "ndt_launch.h"
#include "reg_launch.h"

#define MULLS_GICP_MAX_RING 3 // Chebyshev rings a neighbour query walks before it leaves for the brute-force kernel: at most 7^3 cells
// Three cell tables (reg_table.h) per problem: the neighbour grid of the source, that of the target (cells of knn_edge) and the voxel map of the target.
enum
{
	GICP_TAB_KNN_SRC = 0,
	GICP_TAB_KNN_TGT = 1,
	GICP_TAB_VOXEL = 2,
	GICP_TABS = 3
};
struct GicpDesc
{
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
	GICP_ST_FEW = 3
};
struct GicpRec
{
	gicp::State S;
	uint32_t n_left[2]; // queries left for the brute-force kernel
};
struct GicpOpts
{
	double knn_edge;
	double rotation_epsilon, transformation_epsilon;
	float resolution;
	float start_rotvec[3];
	int32_t k, max_iterations;
};

// the head's status is a GicpStatus; the problem's tables are tabs[MULLS_REG_TABS * p + GICP_TAB_*]
hipError_t launch_gicp_begin(hipStream_t st, uint32_t P, const NdtRec *nrec, GicpRec *rec, RegHead *head, double *frames, GicpOpts opt);
// the ring walk of every point of both clouds; *max_left: the largest number of queries a cloud left uncertified
hipError_t launch_gicp_knn(hipStream_t st, const GicpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t n_max, unsigned char *arena, GicpOpts opt, GicpRec *rec,
						   const RegHead *head, uint32_t *max_left);
hipError_t launch_gicp_brute(hipStream_t st, const GicpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t max_left, unsigned char *arena, GicpOpts opt,
							 const GicpRec *rec, const RegHead *head);
hipError_t launch_gicp_voxels(hipStream_t st, const GicpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t slots_max, unsigned char *arena, const RegHead *head);
hipError_t launch_gicp_eval(hipStream_t st, const GicpDesc *desc, const RegTab *tabs, uint32_t P, unsigned char *arena, GicpOpts opt, const GicpRec *rec,
							const RegHead *head);
// *running: += the problems still running; *next: set to 0 (the word of the tick after)
hipError_t launch_gicp_decide(hipStream_t st, const GicpDesc *desc, uint32_t P, unsigned char *arena, GicpOpts opt, GicpRec *rec, RegHead *head, double *frames,
							  uint32_t *running, uint32_t *next);
