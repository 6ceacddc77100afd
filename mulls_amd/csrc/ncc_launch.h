// ncc_launch.h — host-callable launchers of k_ncc.hip: key-point descriptor matching, CRegistration::find_feature_correspondence_ncc
// (cregistration.hpp:409-601).  The Nt x Ns table of 11-term L1 distances is never stored: every pass recomputes d(i, j) from the two
// descriptor arrays, with the same float expression, so that it has the same bits wherever it is formed.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

// the five floats of a key point the descriptor reads: data[3], normal[0], normal[1], normal[3], intensity
#define MULLS_NCC_LIVE 5u
// key points of one side as the kernels read them: 48-byte records (a device-resident cloud) or the five live floats packed (staged host cloud)
struct NccCloudIn
{
	const float *p;
	uint32_t n;
	uint32_t packed;
};
#define MULLS_NCC_ROWS 256u // rows (= lanes) of a workgroup of the table passes
#define MULLS_NCC_WGS 2048u // workgroups a table pass aims at: the column range is split until there are about this many
#define MULLS_NCC_HIST_LEVELS 6u
#define MULLS_NCC_HIST_BUCKETS 2048u
#define MULLS_NCC_MAX_CORR 65536u
// device state of the fixed-number selection: the rank-K key (float bits of d, flat index i * Ns + j) found digit by digit
struct NccSel
{
	uint32_t remaining; // rank still looked for among the entries that share the digits found so far (1-based)
	uint32_t thr_d;		// digits found so far of the K-th distance's bit pattern, then the pattern
	uint32_t thr_i;		// ... of the flat index up to which distances equal to it belong to the K smallest
	uint32_t done;		// both are final: the remaining levels return at once
	uint32_t none;		// no finite-or-infinite distance at all (every entry NaN): nothing is selected
	uint32_t pad_[3];
};

// intensity_min / intensity_max over the target exactly as the loop of :436-442 leaves them -> mm[0], mm[1]
hipError_t launch_ncc_minmax(hipStream_t st, NccCloudIn tgt, float *mm);
// 11-float descriptors (padded to 12) of both clouds; rowkey[Nt] / colkey[Ns] preset to (FLT_MAX, 0)
hipError_t launch_ncc_desc(hipStream_t st, NccCloudIn tgt, NccCloudIn src, const float *mm, float4 *desc_t, float4 *desc_s, unsigned long long *rowkey,
						   unsigned long long *colkey);
// key[r] = min over the columns of (float bits of d(r, c) << 32 | c): the first column with the strictly smallest distance below FLT_MAX
hipError_t launch_ncc_rowmin(hipStream_t st, const float4 *rows, uint32_t n_rows, const float4 *cols, uint32_t n_cols, unsigned long long *key);
// out[0] = count, out[2 + k] = i, out[2 + n_t + k] = j*(i) of the k-th surviving target in ascending i
hipError_t launch_ncc_recip(hipStream_t st, const unsigned long long *rowkey, const unsigned long long *colkey, uint32_t n_t, int reciprocal, uint32_t *out);
// fixed-number mode: the six digit levels (histogram + pick each), then the collection of every key up to the rank-K key into
// cand[1 ...] (at most MULLS_NCC_MAX_CORR, unordered), their count in the low word of cand[0].  hist: MULLS_NCC_HIST_LEVELS x MULLS_NCC_HIST_BUCKETS words;
// sel, hist and cand[0] zeroed by the caller
hipError_t launch_ncc_select(hipStream_t st, const float4 *desc_t, uint32_t n_t, const float4 *desc_s, uint32_t n_s, uint32_t K, NccSel *sel, uint32_t *hist,
							 unsigned long long *cand);
