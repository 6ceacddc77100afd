// Test harness: C entry points around mulls_amd/csrc/ncc_batch.h, the planner of mulls_ncc_correspond_batch (sub-batch cuts, the arena layout, the
// per-problem records and the prefix tables), built for the CPU so that tests/test_ncc_batch.py can check it without a device.
#include <stdint.h>

#include "../mulls_amd/csrc/ncc_batch.h"

extern "C"
{
	uint64_t nb_problem_bytes(uint32_t n_t, uint32_t n_s, int fixed, uint32_t K) { return ncc_batch_problem_bytes(n_t, n_s, fixed != 0, K); }

	// out: count + 2 slots; returns the number of cut positions written
	int nb_cuts(const uint64_t *bytes, const uint64_t *wgs, uint32_t count, uint64_t limit, uint32_t *out)
	{
		std::vector<uint32_t> c;
		ncc_batch_cuts(bytes, wgs, count, limit, &c);
		for (size_t k = 0; k < c.size(); k++)
			out[k] = c[k];
		return (int)c.size();
	}

	// key_t / key_s: a host cloud's address (0: device-resident).  rec: 20 words per problem, info: 16 words (the order tests/test_ncc_batch.py names)
	int nb_layout(const uint32_t *n_t, const uint32_t *n_s, const uint32_t *K, const uint64_t *key_t, const uint64_t *key_s, uint32_t count, int fixed, uint64_t *rec,
				  uint64_t *info)
	{
		std::vector<NccBatchShape> shape(count);
		for (uint32_t b = 0; b < count; b++)
			shape[b] = NccBatchShape{n_t[b], n_s[b], K[b], (const void *)(uintptr_t)key_t[b], (const void *)(uintptr_t)key_s[b], 48u, 48u, ~0u, ~0u};
		NccBatchLayout L;
		ncc_batch_layout(shape.data(), count, fixed != 0, &L);
		for (uint32_t b = 0; b < count; b++)
		{
			const NccBatchDesc &D = L.desc[b];
			const uint64_t v[20] = {D.in_t, D.in_s, D.desc_t, D.desc_s, D.rowkey, D.colkey, D.mm, D.out, D.sel, D.hist, D.n_t, D.n_s, D.K, D.ext_t, D.ext_s,
									D.chunk, D.chunk_swap, D.wg, D.wg_swap, D.blk};
			for (int k = 0; k < 20; k++)
				rec[20u * b + k] = v[k];
			if (L.wg[b] != D.wg || L.wg_swap[b] != D.wg_swap || L.blk[b] != D.blk)
				return 1; // the prefix tables hold the records' first workgroups
		}
		const uint64_t v[16] = {L.o_desc, L.o_wg, L.o_wg_swap, L.o_blk, L.o_in, L.up_bytes, L.o_sel, L.sel_bytes, L.o_out, L.out_bytes, L.dev_bytes, L.wg[count],
								L.wg_swap[count], L.blk[count], L.staged_at.size(), sizeof(NccBatchDesc)};
		for (int k = 0; k < 16; k++)
			info[k] = v[k];
		return 0;
	}
}
