// ndt_launch.h — what ndt.cpp and k_ndt.hip share: a problem's descriptor (written by the host), its record (kept by the device) and the launches
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/mulls_hip.h"
#include "ndt_math.h"

#define MULLS_NDT_SEG 1024u // threads of the one-workgroup-per-problem setup kernels: a cloud is cut into this many contiguous segments

// byte offsets into the sub-batch's arena; every loop of a kernel is bounded by a field of this descriptor, a launch argument or a constant
struct NdtDesc
{
	uint32_t n_src_in, n_tgt_in;
	uint32_t table_size, table_shift; // a power of two >= max(2 n_tgt_in, MULLS_NDT_SEG); 32 - log2(table_size)
	int32_t apply_guess, crop, n_offsets, offset_first; // rows [offset_first, offset_first + n_offsets) of the offset table
	double G[12];						   // the guess: rotation row-major, translation
	double tgt_bound[6], src_bound[6];
	uint64_t o_src_in, o_tgt_in; // packed float xyz as given (the source: moved by the guess in place)
	uint64_t o_src, o_tgt;		 // ... after the crop
	uint64_t o_cell, o_list;	 // per target point: its slot; the points of every slot, ascending
	uint64_t o_keys, o_count, o_start, o_fill; // the hash table: cell index (-1: free), points, first entry in list, fill counter
	uint64_t o_leaves;						   // ndt::Leaf of a slot at index start[slot]
	uint64_t o_partial;						   // 28 x MULLS_NDT_TREE doubles
	uint64_t o_dist;						   // float per source point
};
enum NdtStatus
{
	NDT_ST_OK = 0,
	NDT_ST_NONFINITE = 1,
	NDT_ST_GRID = 2,
	NDT_ST_EMPTY = 3
};
struct NdtRec
{
	ndt::State S;
	ndt::Frame F; // of S.xt
	double fitness;
	uint32_t n_src, n_tgt, n_leaves, n_leaves_used;
	int32_t min_b[3], max_b[3], div_b[3];
	int32_t status;
};
struct NdtOpts
{
	ndt::Opts o; // (n_src is filled per problem on the device)
	double d1, d2, eig_mult;
	float resolution, inv_resolution;
	int32_t min_points;
};

hipError_t launch_ndt_crop(hipStream_t st, const NdtDesc *desc, uint32_t P, unsigned char *arena, NdtOpts opt, NdtRec *rec);
// the table emptied (every slot below table_max), then the cells
hipError_t launch_ndt_cells(hipStream_t st, const NdtDesc *desc, uint32_t P, uint32_t n_tgt_max, uint32_t table_max, unsigned char *arena, NdtOpts opt, NdtRec *rec);
hipError_t launch_ndt_offsets(hipStream_t st, const NdtDesc *desc, uint32_t P, unsigned char *arena, NdtRec *rec);
hipError_t launch_ndt_scatter(hipStream_t st, const NdtDesc *desc, uint32_t P, uint32_t n_tgt_max, unsigned char *arena, const NdtRec *rec);
hipError_t launch_ndt_leaves(hipStream_t st, const NdtDesc *desc, uint32_t P, uint32_t table_max, unsigned char *arena, NdtOpts opt, NdtRec *rec);
hipError_t launch_ndt_begin(hipStream_t st, uint32_t P, NdtRec *rec);
hipError_t launch_ndt_eval(hipStream_t st, const NdtDesc *desc, uint32_t P, unsigned char *arena, NdtOpts opt, const NdtRec *rec);
// *running: += the problems still running; *next: set to 0 (the word of the tick after)
hipError_t launch_ndt_decide(hipStream_t st, const NdtDesc *desc, uint32_t P, unsigned char *arena, NdtOpts opt, NdtRec *rec, uint32_t *running, uint32_t *next);
// frames: NULL (the pose is T(rec[p].S.p)), or 12 doubles a problem: the rotation row-major, the translation (mulls_gicp)
hipError_t launch_ndt_fitness(hipStream_t st, const NdtDesc *desc, uint32_t P, uint32_t n_src_max, unsigned char *arena, NdtRec *rec, const double *frames);
