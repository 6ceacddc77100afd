// pgo_launch.h — host-callable launchers of k_pgo.hip: the pose graph optimisation (include/mulls_hip.h has the definition).  The problems of one
// sub-batch of mulls_pgo_optimize_batch lie side by side in one device arena; a descriptor per problem holds the offsets of its tables.  The host drives
// the Levenberg-Marquardt iterations in lock step: six launches and one 4-byte readback per iteration for the whole sub-batch.  Every loop of every kernel
// is bounded by a launch argument, a descriptor field the host wrote, or a constant.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define MULLS_PGO_TREE 256		  // width of the strided partials and of the pairwise tree of the cost and model-decrease sums; the workgroup of the per-problem kernels
#define MULLS_PGO_SLOT_DOUBLES 120 // an edge's own slot: Haa, Hab, Hbb (36 each, row-major), ga, gb (6 each)

// one used edge as the device reads it
struct PgoEdge
{
	int32_t a, b;	// node indices
	double th[3];	// t^
	double qh[4];	// q^
	double W[36];	// the weight matrix, row-major
};
// one problem of a sub-batch: sizes and byte offsets into the arena
struct PgoDesc
{
	uint32_t n_nodes, n_edges, n_unk, n_blocks; // n_edges: used edges; n_unk: non-fixed nodes; n_blocks: 6 x 6 blocks of the skyline
	// tables the host uploads
	uint64_t o_state;  // double [7 n_nodes]: t, q
	uint64_t o_init;   // double [7 n_nodes]: the state at the start (the centre of the boxes)
	uint64_t o_limit;  // double [2 n_nodes]: t limit, r limit
	uint64_t o_unk;	   // int32 [n_nodes]: unknown index, -1 for a fixed node
	uint64_t o_boxed;  // int32 [n_nodes]
	uint64_t o_edges;  // PgoEdge [n_edges]
	uint64_t o_adj0;   // uint32 [n_nodes + 1]: node i's used edges are adj[adj0[i] .. adj0[i + 1]), ascending
	uint64_t o_adj;	   // uint32 [2 n_edges]
	uint64_t o_node;   // uint32 [n_unk]: the node of an unknown
	uint64_t o_first;  // uint32 [n_unk]: first block column of block row i
	uint64_t o_rowoff; // uint32 [n_unk + 1]: block (i, j) is block rowoff[i] + j - first[i]
	uint64_t o_colmax; // uint32 [n_unk]: the last block row that holds column j
	uint64_t o_blkrow; // uint32 [n_blocks]: the block row of a block
	// work arrays
	uint64_t o_cand;  // double [7 n_nodes]
	uint64_t o_slot;  // double [MULLS_PGO_SLOT_DOUBLES n_edges]
	uint64_t o_term;  // double [n_edges]: rho(s) of the state (at the start) or of the candidate
	uint64_t o_H;	  // double [36 n_blocks]: H + D, then L in place
	uint64_t o_g;	  // double [6 n_unk]
	uint64_t o_diag;  // double [6 n_unk]: D
	uint64_t o_delta; // double [6 n_unk]: -g, y, delta in place
};
// one problem's record: the loop's scalars, written by the device, downloaded once at the end
struct PgoRec
{
	double cost, initial_cost, radius, nu, md, gmax, dmax;
	int32_t status, termination, iterations, successful;
	int32_t running, relin, solve_failed, pad;
};
// what the kernels need of mulls_pgo_params
struct PgoOpts
{
	double delta, function_tolerance;
	int32_t robustify, only_translation, num_iterations, pad;
};

// rec[p] = the start of the loop for every problem of the sub-batch
hipError_t launch_pgo_reset(hipStream_t st, PgoRec *rec, uint32_t P);
// edges of the problems that run and whose state moved (rec.relin): the slot and term[e] at the state.  e_max: the largest n_edges
hipError_t launch_pgo_linearize(hipStream_t st, const PgoDesc *desc, uint32_t P, uint32_t e_max, unsigned char *arena, PgoOpts opt, const PgoRec *rec);
// once, after the first linearisation: the initial cost and the stops that precede the first iteration
hipError_t launch_pgo_begin(hipStream_t st, const PgoDesc *desc, uint32_t P, unsigned char *arena, PgoOpts opt, PgoRec *rec);
// H + D into the skyline, D, g and -g.  w_max: the largest 36 n_blocks + 6 n_unk
hipError_t launch_pgo_assemble(hipStream_t st, const PgoDesc *desc, uint32_t P, uint64_t w_max, unsigned char *arena, const PgoRec *rec);
// one workgroup per problem: the gradient stop, iterations += 1, the factorisation, the two substitutions, the step stop, the model decrease
hipError_t launch_pgo_factor_solve(hipStream_t st, const PgoDesc *desc, uint32_t P, unsigned char *arena, PgoRec *rec);
// cand = projection of the update of the state.  n_max: the largest n_nodes
hipError_t launch_pgo_candidate(hipStream_t st, const PgoDesc *desc, uint32_t P, uint32_t n_max, unsigned char *arena, PgoOpts opt, const PgoRec *rec);
// term[e] at the candidate
hipError_t launch_pgo_cost(hipStream_t st, const PgoDesc *desc, uint32_t P, uint32_t e_max, unsigned char *arena, PgoOpts opt, const PgoRec *rec);
// one workgroup per problem: cost+, accept or reject, the radius rule, the stops; *running += 1 per problem that goes on (zeroed by the caller)
hipError_t launch_pgo_decide(hipStream_t st, const PgoDesc *desc, uint32_t P, unsigned char *arena, PgoOpts opt, PgoRec *rec, uint32_t *running);
