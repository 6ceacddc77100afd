// extract_internal.h — what the translation units of the feature stage share besides the ABI: ground.cpp (ground filter, single-scan extraction),
// classify.cpp (classification) and extract_batch.cpp (mulls_extract_features_batch).  Nothing here is exported.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/mulls_hip.h"
#include "classify_launch.h"
#include "ctx.h"

#define MULLS_HIDDEN __attribute__((visibility("hidden")))

extern "C"
{
	// classify.cpp
	MULLS_HIDDEN int mulls_classify_impl(mulls_ctx *ctx, const void *pts, bool pts_on_device, uint32_t n_in, uint32_t stride, const mulls_classify_params *P,
										 void *const out[MULLS_CL_COUNT], const uint32_t cap[MULLS_CL_COUNT], uint32_t n_out[MULLS_CL_COUNT], void *cloud_in_after,
										 uint32_t *n_cloud_in_after, ClassifyDev *dev_out);
	MULLS_HIDDEN void mulls_classify_thin_down(std::vector<unsigned char> *host, const mulls_classify_params *P);
	MULLS_HIDDEN int mulls_classify_check(mulls_ctx *ctx, const mulls_classify_params *P);
	MULLS_HIDDEN void mulls_classify_kernel_params(const mulls_classify_params *P, ClParams *out);
	// ground.cpp
	MULLS_HIDDEN int gf_check(mulls_ctx *ctx, const mulls_ground_params *P, uint32_t n);
	MULLS_HIDDEN int gf_rnd_table(mulls_ctx *ctx);
	MULLS_HIDDEN void gf_ground_down_indices(const mulls_ground_params *P, uint32_t n_ground, std::vector<uint32_t> &idx);
	MULLS_HIDDEN int extract_impl(mulls_ctx *ctx, const void *scan, uint32_t n_in, uint32_t stride, const mulls_extract_params *X, void *const out[MULLS_EX_COUNT],
								  const uint32_t cap[MULLS_EX_COUNT], uint32_t n_out[MULLS_EX_COUNT], mulls_block *blk);
}
