// ransac_launch.h — host-callable launchers of k_ransac.hip: the RANSAC coarse-registration solver, CRegistration::coarse_reg_ransac
// (cregistration.hpp:605-661).  The sample sequence does not depend on the hypotheses' counts, so the host draws every sample up front, one launch
// builds and one launch scores all hypotheses, and the host applies PCL's sequential rule to the counts (include/mulls_hip.h has the definition).
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "ransac_batch.h"

#define MULLS_RANSAC_MAX_POINTS 65536u
#define MULLS_RANSAC_MAX_ITER (1 << 20)
#define MULLS_RANSAC_REFINE_THREADS 256u // the partial sums of a refinement fit: part of the definition, not a tuning knob

// rows 0..2 of a 4 x 4 rigid transform, row-major, float
struct RansacModel
{
	float m[12];
};
// what one refinement round leaves for the host
struct RansacRound
{
	RansacModel T;	  // the fit to the previous inliers
	uint32_t n_new;	  // inliers of T within the round's threshold
	uint32_t changed; // the new inlier set differs from the previous one
	float median;	  // the selected squared distances' element of rank n_new / 2 (ascending)
	uint32_t n_prev;
};

// models[h] = the rigid transform of the three pairs triples[3h .. 3h + 2]
hipError_t launch_ransac_models(hipStream_t st, const float4 *src, const float4 *tgt, const int32_t *triples, uint32_t n_hyp, RansacModel *models);
// counts[h] = number of pairs within thresh (squared, double) of models[h]
hipError_t launch_ransac_score(hipStream_t st, const float4 *src, const float4 *tgt, uint32_t n, const RansacModel *models, uint32_t n_hyp, double thresh,
							   uint32_t *counts);
// mask[i] = pair i lies within thresh of *model (a device pointer); *count (zeroed by the caller) = their number
hipError_t launch_ransac_select(hipStream_t st, const float4 *src, const float4 *tgt, uint32_t n, const RansacModel *model, double thresh, uint8_t *mask,
								uint32_t *count);
// one round of refineModel: fit to the pairs of mask_prev, select within thresh into mask_new, the median for the next threshold
hipError_t launch_ransac_refine(hipStream_t st, const float4 *src, const float4 *tgt, uint32_t n, const uint8_t *mask_prev, uint8_t *mask_new, float *d2,
								double thresh, RansacRound *out);

// ---- mulls_coarse_reg_ransac_batch: the same steps for the `count` problems of a sub-batch, read from their descriptors (ransac_batch.h; device memory);
// arena: the base the descriptors' offsets count from.  n_max / n_hyp_max: the largest problem's pairs / hypotheses (both above 0: a zero-sized grid is an error)
hipError_t launch_ransac_batch_models(hipStream_t st, const RansacBatchDesc *desc, uint32_t count, uint32_t n_hyp_max, unsigned char *arena);
hipError_t launch_ransac_batch_score(hipStream_t st, const RansacBatchDesc *desc, uint32_t count, uint32_t n_hyp_max, unsigned char *arena, double thresh);
// every problem's winner (desc[b].best): its mask into buffer 0, its model and count into win[b] (T, n_new; zeroed by the caller)
hipError_t launch_ransac_batch_select(hipStream_t st, const RansacBatchDesc *desc, uint32_t count, uint32_t n_max, unsigned char *arena, double thresh, RansacRound *win);
// one refinement round of the n_jobs problems the jobs name, one workgroup each; a problem without a job is not touched
hipError_t launch_ransac_batch_refine(hipStream_t st, const RansacBatchDesc *desc, const RansacBatchJob *jobs, uint32_t n_jobs, unsigned char *arena);
