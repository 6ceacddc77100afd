// fpfh_launch.h — what fpfh.cpp and k_fpfh.hip share: a cloud's descriptor (written by the host) and the launches.  A cloud takes the place of a
// problem in the shared cell tables (reg_table.h): its table is tabs[MULLS_REG_TABS * c], its head head[c] with the cloud's points in n[0].  The
// nearest-target pass of SAC-IA's hypotheses and of the fitness is mulls_ndt's (ndt_launch.h): a hypothesis has an NdtDesc and an NdtRec for it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/mulls_hip.h"
#include "fpfh_math.h"
#include "ndt_launch.h"
#include "reg_launch.h"

#define MULLS_FPFH_HYP_CHUNK 1024u // hypotheses whose nearest-target distances are held at a time (one grid dimension of the pass)

struct FpfhDesc
{
	uint32_t n, pad;
	uint64_t o_pts, o_nrm;	 // packed float xyz as given: the coordinates, the normals
	uint64_t o_cpts, o_cnrm; // ... in the order of the table's list: cell by cell, ascending index inside a cell
	uint64_t o_spfh, o_hist; // n x 33 float
	uint64_t o_k;			 // uint32 a point: the size of its neighbourhood
};
// head[c].range: bit 0 a coordinate outside the cells' range (k_reg_table.hip), bit 1 a coordinate or normal that is not finite, bit 2 a cell too full
#define MULLS_FPFH_RANGE 1u
#define MULLS_FPFH_NONFINITE 2u
#define MULLS_FPFH_CELL_FULL 4u // a cell holds more than MULLS_FPFH_MAX_CELL_POINTS points

struct FpfhSacOut
{
	int32_t best, pad;
	double error;
	double frame[12]; // the winner's rotation row-major, then its translation
};

// C clouds: the finiteness check, the tables, every cell's list ascending and the coordinates and normals in that order, SPFH, FPFH
hipError_t launch_fpfh_features(hipStream_t st, const FpfhDesc *desc, const RegTab *tabs, uint32_t C, uint32_t n_max, uint32_t slots_max, unsigned char *arena,
								double r2, RegHead *head);
// corr[s]: the target descriptor of rank ranks[s] among the k_eff nearest to the source descriptor samples[s], by (d2, index)
hipError_t launch_fpfh_similar(hipStream_t st, const float *src_hist, const float *tgt_hist, const int32_t *samples, const int32_t *ranks, uint32_t n_samples,
							   uint32_t n_src, uint32_t n_tgt, uint32_t k_eff, int32_t *corr);
// frames[12 h ..]: the rigid transform of hypothesis h's three pairs (ransac_math.h), rotation row-major then translation, as doubles of its floats
hipError_t launch_fpfh_models(hipStream_t st, const float *src, const float *tgt, const int32_t *samples, const int32_t *corr, uint32_t n_hyp, uint32_t n_src,
							  uint32_t n_tgt, double *frames);
// desc[h], rec[h], h < n: base with the distances of hypothesis slot h at base.o_dist + 4 n_src h
hipError_t launch_fpfh_slots(hipStream_t st, NdtDesc base, uint32_t n_src, uint32_t n_tgt, uint32_t n, NdtDesc *desc, NdtRec *rec);
// err[h], h < n: the strided-partial sum of the error terms over desc[h]'s distances
hipError_t launch_fpfh_errors(hipStream_t st, const NdtDesc *desc, uint32_t n, uint32_t n_src, unsigned char *arena, float thr, int huber, double *err);
// the lowest error, the first among equals
hipError_t launch_fpfh_pick(hipStream_t st, const double *err, const double *frames, uint32_t n_hyp, FpfhSacOut *out);

// ---- many problems per launch (k_fpfh_batch.hip): a sub-batch's table, written by the host.  The samples, ranks, correspondences, frames and errors of
// all problems are flat lists in problem order; problem b's hypotheses are first_hyp .. first_hyp + n_hyp - 1, its samples first_sample .. + 3 n_hyp - 1.
struct FpfhProb
{
	uint64_t o_src, o_tgt;			 // packed float xyz
	uint64_t o_src_hist, o_tgt_hist; // n x 33 float
	uint64_t o_win_dist;			 // float per source point: the winner's distances
	uint64_t dist_first;			 // the distance bytes of all hypotheses before first_hyp
	uint32_t n_src, n_tgt, k_eff;
	uint32_t first_sample, first_hyp, n_hyp;
};
// corr[s], s < n_samples: as launch_fpfh_similar, the wave finding its problem from s
hipError_t launch_fpfh_batch_similar(hipStream_t st, const FpfhProb *prob, uint32_t P, unsigned char *arena, const int32_t *samples, const int32_t *ranks,
									 uint32_t n_samples, int32_t *corr);
// frames[12 h ..], h < n_hyp
hipError_t launch_fpfh_batch_models(hipStream_t st, const FpfhProb *prob, uint32_t P, unsigned char *arena, const int32_t *samples, const int32_t *corr,
									uint32_t n_hyp, double *frames);
// desc[j], rec[j], j < n: hypothesis h0 + j of the flat list, its distances at o_pool + d(h0 + j) - d0
hipError_t launch_fpfh_batch_slots(hipStream_t st, const FpfhProb *prob, uint32_t P, uint32_t h0, uint32_t n, uint64_t o_pool, uint64_t d0, NdtDesc *desc, NdtRec *rec);
// err[j], j < n: over desc[j]'s distances, n_src its own
hipError_t launch_fpfh_batch_errors(hipStream_t st, const NdtDesc *desc, uint32_t n, unsigned char *arena, float thr, int huber, double *err);
// a workgroup per problem: out[b], the winner's frame in win_frames[12 b ..], and the slot of its fitness pass in desc[b], rec[b]
hipError_t launch_fpfh_batch_pick(hipStream_t st, const FpfhProb *prob, uint32_t P, const double *err, const double *frames, FpfhSacOut *out, double *win_frames,
								  NdtDesc *desc, NdtRec *rec);
