// extract_internal.h — what the translation units of the feature stage share besides the ABI: ground.cpp (the ground stage's checks and samplers, voxel
// down-sampling, feature blocks), classify.cpp (the classification's checks and samplers) and extract_batch.cpp (the chain itself, for every entry point).
// Nothing here is exported.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/mulls_hip.h"
#include "classify_launch.h"
#include "ctx.h"
#include "extract_batch.h"

#define MULLS_HIDDEN __attribute__((visibility("hidden")))

extern "C"
{
	// classify.cpp
	MULLS_HIDDEN void mulls_classify_thin_down(std::vector<unsigned char> *host, const mulls_classify_params *P);
	MULLS_HIDDEN int mulls_classify_check(mulls_ctx *ctx, const mulls_classify_params *P);
	MULLS_HIDDEN void mulls_classify_kernel_params(const mulls_classify_params *P, ClParams *out);
	// ground.cpp
	MULLS_HIDDEN int gf_check(mulls_ctx *ctx, const mulls_ground_params *P, uint32_t n);
	MULLS_HIDDEN int gf_rnd_table(mulls_ctx *ctx);
	MULLS_HIDDEN void gf_ground_down_indices(const mulls_ground_params *P, uint32_t n_ground, std::vector<uint32_t> &idx);
	MULLS_HIDDEN int vox_run(mulls_ctx *ctx, unsigned char *base, const mulls_ex::GfArena &a, const float4 *in, uint32_t n, float voxel_size, float4 *down, uint32_t *n_down);
	// extract_batch.cpp
	MULLS_HIDDEN int ex_arena_reserve(mulls_ctx *ctx, uint64_t need, uint64_t limit);
}
