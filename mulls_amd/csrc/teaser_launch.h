// teaser_launch.h — host-callable launchers of k_teaser.hip and k_teaser_clique.hip: the TEASER coarse-registration solver, CRegistration::coarse_reg_teaser
// (cregistration.hpp:664-759).  The device builds the pair-consistency graph as a bit matrix, peels it to core numbers, bounds the clique from below with
// a greedy clique per vertex and compacts the vertices that can still belong to a maximum clique; the exact search runs on the host (teaser_host.h) or,
// with MULLS_OPT_TEASER_DEVICE_SEARCH, on the device (k_teaser_clique.hip, the scheme of teaser_search.h); the GNC-TLS rotation runs on the device
// again, one launch set per iteration (include/mulls_hip.h has the definition).
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "teaser_batch.h"
#include "teaser_math.h"
#include "teaser_search.h"

// adj: n rows of W = ceil(n / 64) words, bit j of row i = edge {i, j}; bits at and above n are zero, the diagonal is zero
hipError_t launch_teaser_graph(hipStream_t st, const float4 *src, const float4 *tgt, uint32_t n, double beta, uint64_t *adj);
// deg[i] = popcount of row i; *deg_sum (zeroed by the caller) = their sum = twice the edge count
hipError_t launch_teaser_degrees(hipStream_t st, const uint64_t *adj, uint32_t n, uint32_t *deg, unsigned long long *deg_sum);
// core[i] = core number of vertex i
hipError_t launch_teaser_cores(hipStream_t st, const uint64_t *adj, uint32_t n, const uint32_t *deg, uint32_t *core);
// greedy[v] = size of the clique grown from v by taking the smallest common neighbour until none is left
hipError_t launch_teaser_greedy(hipStream_t st, const uint64_t *adj, uint32_t n, uint32_t *greedy);
// sub: the m x ceil(m / 64) bit matrix of the vertices keep[0] < ... < keep[m - 1]
hipError_t launch_teaser_compact(hipStream_t st, const uint64_t *adj, uint32_t n, const int32_t *keep, uint32_t m, uint64_t *sub);
// cs[k] = src[clique[k]], ct[k] = tgt[clique[k]]
hipError_t launch_teaser_pick(hipStream_t st, const float4 *src, const float4 *tgt, const int32_t *clique, uint32_t C, float4 *cs, float4 *ct);
// one GNC iteration over the M = C (C - 1) / 2 measurements of the clique: fit (S->R), residuals and cost (S->cost, S->mu, S->stop), weight update
// (weights, S->n_inlier; skipped on the device when S->stop == 1).  part: 9 * MULLS_TEASER_PARTIALS doubles.
hipError_t launch_teaser_gnc_iteration(hipStream_t st, const float4 *cs, const float4 *ct, uint32_t C, int iter, double nb2, double *weights, double *part,
									   TeaserGnc *S);

// ---- the same steps over the problems of one sub-batch of mulls_coarse_reg_teaser_batch per launch.  desc: the sub-batch's descriptor table in device memory
// (teaser_batch.h), arena: the base its offsets count from.
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

// ---- k_teaser_clique.hip: the device clique search (teaser_search.h has the scheme)
// later[v] = the neighbours of v above v in the m x ceil(m / 64) matrix sub
hipError_t launch_teaser_later(hipStream_t st, const uint64_t *sub, uint32_t m, uint32_t *later);
struct TeaserSearchArgs
{
	const uint64_t *sub;   // m x W
	const uint32_t *first; // m + 1: TeaserPlan::first
	uint32_t m, W, n_tasks, levels;
	uint32_t phase, omega; // 0: the size (ctl->bound rises from lb); 1: the list of omega vertices
	uint32_t quota, workers;
	TeaserSearchCtl *ctl;
	TeaserWorkerState *state; // workers
	uint64_t *slab;			  // workers x levels x W: the stacks
	uint32_t *cur;			  // workers x levels: the cliques so far
};
// one launch: every worker enters at most `quota` tree nodes
hipError_t launch_teaser_clique(hipStream_t st, const TeaserSearchArgs &A);
// out[0] = size, out[1 .. size] = the greedy clique of vertex v in the order taken; out: m + 1 words
hipError_t launch_teaser_witness(hipStream_t st, const uint64_t *sub, uint32_t m, uint32_t v, uint32_t *out);
