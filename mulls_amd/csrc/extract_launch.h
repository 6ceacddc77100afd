// extract_launch.h — host-callable launcher of k_extract_batch.hip: the byte ranges mulls_extract_features_batch moves or clears, any number of them in one launch
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

// one byte range: dst <- src, or dst <- 0 where src is 0.  Addresses and sizes are multiples of 4 (whole 16-byte words are moved where all three are multiples
// of 16).  Either side may be host-mapped pinned memory: that is how words, keys and records cross in one launch instead of one copy command per scan.
struct ExSeg
{
	unsigned long long dst, src;
	uint32_t bytes, pad_;
};
// tab_dev: `count` ranges in device memory; max_bytes: the longest of them.  Returns the kernels launched (0 or 1).
int launch_ex_segs(hipStream_t st, const ExSeg *tab_dev, uint32_t count, uint32_t max_bytes);
