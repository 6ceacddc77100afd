// pair_stage.h — what the two coarse-registration solvers (ransac.cpp, teaser.cpp) share on the host: how a call refuses, where a problem's clouds lie, and
// the staging of its pairs.  A solver takes pairs of points out of two clouds, each in host or in device memory, with or without index lists; stage_pairs
// puts the points of a list of problems into a device arena as n float4 per side (x, y, z, data[3]).  pair_stage.cpp has the code, k_pair_gather.hip the kernel.
#pragma once
#include "ctx.h"
#include "pair_gather.h"

// who refuses: the entry point's name and, in a batch, the problem's index — mulls_last_error reads "<entry point>: [problem <b>: ]<why>"
struct Refusal
{
	mulls_ctx *ctx;
	const char *who;
	int64_t problem; // -1: a single call

	int operator()(int code, const char *why) const
	{
		ctx->err = std::string(who) + (problem >= 0 ? ": problem " + std::to_string(problem) : std::string()) + ": " + why;
		return code;
	}
	// a refusal the single calls make without a message
	int quiet(int code, const char *why) const { return problem >= 0 ? (*this)(code, why) : code; }
};

struct BatchProblem // a problem that reaches the device
{
	uint32_t index, n;
	bool indexed, t_dev, s_dev;
};

inline void identity16(double T[16])
{
	for (int k = 0; k < 16; k++)
		T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

bool cloud_on_device(mulls_ctx *ctx, const mulls_cloud &c);
// x, y, z, data[3] of the n pairs' points out of a host cloud
void pack_xyzw(const mulls_cloud &c, const int32_t *idx, uint32_t n, float *out);
// once the device is set, for a problem that runs: where its clouds lie (A->t_dev, A->s_dev), and their strides
int check_strides(const Refusal &refuse, const mulls_cloud &T, const mulls_cloud &S, BatchProblem *A);

// one problem of a staging: its clouds and lists as the caller handed them in, what the checks found, and its places in the device arena
struct PairStageItem
{
	const mulls_cloud *tgt, *src;
	const int32_t *tgt_idx, *src_idx; // read when indexed
	uint32_t n;
	bool indexed, t_dev, s_dev;
	uint64_t o_src, o_tgt, o_idx; // n float4, n float4, 2 n int32 (the target's list, then the source's)
};
// the regions of a staging in the device arena and their pinned mirrors: an array lies at the same offset inside its region in both.  Every problem's points
// lie inside [o_pts, o_pts + pts_bytes), its lists inside [o_idx, o_idx + idx_bytes); the job tables hold two PairGather per problem.
struct PairStagePlaces
{
	uint64_t o_pts, pts_bytes, o_idx, idx_bytes, o_jobs;
	uint64_t p_pts, p_idx, p_jobs;
};
// The points of `count` problems into the arena d (pinned mirror h), on the stream: host clouds packed into the mirror and up in one copy, the index lists
// of problems with a device-resident cloud up in one copy, the jobs up and one gather launch for the device-resident clouds.  Nothing is waited for.
int stage_pairs(mulls_ctx *ctx, hipStream_t st, unsigned char *d, unsigned char *h, const PairStagePlaces &L, const PairStageItem *items, uint32_t count);

// k_pair_gather.hip: the jobs' device-resident clouds into the points of their problems (jobs: device memory; arena: the base their offsets count from);
// n_max: the largest job
hipError_t launch_pair_gather(hipStream_t st, const PairGather *jobs, uint32_t n_jobs, uint32_t n_max, unsigned char *arena);
