// teaser_batch_launch.h — host-callable launchers of k_teaser_batch.hip: the steps of teaser_launch.h over the problems of one sub-batch of
// mulls_coarse_reg_teaser_batch per launch.  desc: the sub-batch's descriptor table in device memory (teaser_batch.h), arena: the base its offsets count from.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "teaser_batch.h"

// the jobs' device-resident clouds into the points of their problems; n_max: the largest job
hipError_t launch_teaser_batch_gather(hipStream_t st, const TeaserBatchGather *jobs, uint32_t n_jobs, uint32_t n_max, unsigned char *arena);
// of every problem: the bit matrix, the degrees and deg_sum[b] (zeroed by the caller), the core numbers, the greedy clique sizes (behind the core numbers)
hipError_t launch_teaser_batch_graph(hipStream_t st, const TeaserBatchDesc *desc, uint32_t B, uint32_t n_max, unsigned char *arena, double beta,
									 unsigned long long *deg_sum);
// of every problem with m > 0: the m x Wm sub-matrix of the vertices of its keep list; words_max: the largest m * Wm
hipError_t launch_teaser_batch_compact(hipStream_t st, const TeaserBatchDesc *desc, uint32_t B, uint64_t words_max, unsigned char *arena);
// of every problem: cs[k] = src[keep[k]], ct[k] = tgt[keep[k]], k < C
hipError_t launch_teaser_batch_pick(hipStream_t st, const TeaserBatchDesc *desc, uint32_t B, uint32_t C_max, unsigned char *arena);
// GNC iteration `iter` of the problems first .. first + count that still run (C >= 2, no stop word from an earlier iteration): launch_teaser_gnc_iteration's
// five steps, one launch each for all of them.  gnc, frozen: one entry per problem of the sub-batch (frozen zeroed before iteration 0).
hipError_t launch_teaser_batch_gnc_iteration(hipStream_t st, const TeaserBatchDesc *desc, uint32_t first, uint32_t count, uint64_t M_max, int iter, double nb2,
											 unsigned char *arena, unsigned char *weights, TeaserGnc *gnc, uint32_t *frozen);
