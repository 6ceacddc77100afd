// Test harness: C entry points around mulls_amd/csrc/nms_batch.h, the planner of mulls_non_max_suppress_batch (sub-batch cuts, the arena layout, the
// per-problem records), built for the CPU so that tests/test_nms_batch.py can check it without a device.
#include <stdint.h>

#include "../mulls_amd/csrc/nms_batch.h"

namespace
{
std::vector<NmsBatchShape> shapes(const uint64_t *pts, const uint32_t *n, const uint32_t *cap, const uint32_t *on_dev, uint32_t count, int path)
{
	std::vector<NmsBatchShape> s(count);
	for (uint32_t b = 0; b < count; b++)
		s[b] = NmsBatchShape{(const void *)(uintptr_t)pts[b], n[b], 48u, cap[b], on_dev[b], nms_batch_takes_lds(n[b], path), ~0u};
	return s;
}
} // namespace

extern "C"
{
	uint64_t nmb_cloud_bytes(uint32_t n, int on_dev, int lds) { return nms_batch_cloud_bytes(n, on_dev != 0, lds != 0); }
	uint64_t nmb_problem_bytes(uint32_t n, uint32_t cap, int lds) { return nms_batch_problem_bytes(n, cap, lds != 0); }
	uint64_t nmb_fixed_bytes(void) { return MULLS_NMS_BATCH_FIXED_BYTES; }
	uint64_t nmb_limit(uint64_t scratch_limit_bytes) { return nms_batch_limit(scratch_limit_bytes); }

	// cuts: count + 2 slots, bytes: count + 1 slots (every sub-batch's counted bytes); returns the number of cut positions written
	int nmb_cuts(const uint64_t *pts, const uint32_t *n, const uint32_t *cap, const uint32_t *on_dev, uint32_t count, int path, uint64_t limit, uint32_t *cuts,
				 uint64_t *bytes)
	{
		std::vector<NmsBatchShape> s = shapes(pts, n, cap, on_dev, count, path);
		std::vector<uint32_t> c;
		std::vector<uint64_t> held;
		nms_batch_cuts(s.data(), count, limit, &c, &held);
		for (size_t k = 0; k < c.size(); k++)
			cuts[k] = c[k];
		for (size_t k = 0; k < held.size(); k++)
			bytes[k] = held[k];
		return (int)c.size();
	}

	// rec: 8 words per problem (stage, in the suppression launch?, recs, hdr, kept, n, H, out_cap; the offsets 0 for a problem without a workgroup),
	// info: 14 words (the order tests/test_nms_batch.py names)
	int nmb_layout(const uint64_t *pts, const uint32_t *n, const uint32_t *cap, const uint32_t *on_dev, uint32_t count, int path, uint64_t *rec, uint64_t *info)
	{
		std::vector<NmsBatchShape> s = shapes(pts, n, cap, on_dev, count, path);
		NmsBatchLayout L;
		nms_batch_layout(s.data(), count, &L);
		for (uint32_t b = 0; b < count; b++)
		{
			rec[8u * b] = s[b].stage;
			for (int k = 1; k < 8; k++)
				rec[8u * b + k] = 0;
		}
		for (size_t k = 0; k < L.desc.size(); k++)
		{
			const NmsBatchDesc &D = L.desc[k];
			if (D.problem >= count || (k && D.problem <= L.desc[k - 1].problem))
				return 1; // in problem order
			const uint64_t v[7] = {1, D.recs, D.hdr, D.kept, D.n, D.H, D.out_cap};
			for (int j = 0; j < 7; j++)
				rec[8u * D.problem + 1 + j] = v[j];
		}
		if (L.blk.size() != L.src.size() + 1u)
			return 2;
		for (size_t c = 0; c < L.src.size(); c++)
			if (L.blk[c] != L.src[c].blk || (c < L.n_gather) != (L.src[c].recs != 0))
				return 3; // the prefix table holds the clouds' first blocks; the gathered clouds come first
		const uint64_t v[14] = {L.desc.size(), L.n_max, L.staged.size(), L.src.size(), L.n_gather, L.gather_blk, L.blk[L.src.size()],
								L.head_bytes, L.up_bytes, L.o_cursor, L.down_bytes, L.o_out, L.out_records, L.dev_bytes};
		for (int k = 0; k < 14; k++)
			info[k] = v[k];
		return 0;
	}
}
