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
