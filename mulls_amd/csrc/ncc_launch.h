// ncc_launch.h — what the host and the device code of key-point descriptor matching, CRegistration::find_feature_correspondence_ncc
// (cregistration.hpp:409-601), share: the input view, the constants and the selection record (ncc_device.h has the device code, ncc_batch.h the planner
// and the launchers).
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
