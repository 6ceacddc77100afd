// extract_batch_harness.cpp — the planner of mulls_extract_features_batch (mulls_amd/csrc/extract_batch.h) on the CPU, for tests/test_extract_batch.py:
// as a shared library the test calls through ctypes, and (with -DEB_MAIN) as a stand-alone program that checks the same properties itself, so that it can
// run under -fsanitize=address,undefined.  Host code only: the HIP headers it sees declare types, nothing is linked.
#include <cstdio>
#include <vector>

#include "../mulls_amd/csrc/extract_batch.h"

using namespace mulls_ex;

extern "C"
{
	// the single calls' formulas: gf_layout(...).total and carve(nullptr, ...).total
	uint64_t eb_gf_total(uint32_t n, int prefilter, int normal_method) { return gf_layout(n, prefilter != 0, false, normal_method).total; }
	uint64_t eb_cl_total(uint32_t n, uint32_t K, uint32_t n_in) { return carve(nullptr, n, K, n_in).total; }
	uint32_t eb_work_points(uint32_t n_in, int fixed_num, int unground_down_fixed_num) { return classify_work_points(n_in, fixed_num != 0, unground_down_fixed_num); }
	uint64_t eb_table_bytes(void) { return MULLS_EXB_TABLE_BYTES; }
	uint64_t eb_head_bytes(void) { return MULLS_EXB_HEAD_BYTES; }
	uint32_t eb_max_scans(void) { return MULLS_EXB_MAX_SCANS; }
	// out[3]: ground region, classify region, total
	void eb_scan_cost(uint32_t n, int prefilter, int normal_method, int fixed_num, int unground_down_fixed_num, uint32_t K, uint64_t *out)
	{
		const ScanCost c = extract_batch_scan_cost(n, prefilter != 0, normal_method, fixed_num != 0, unground_down_fixed_num, K);
		out[0] = c.gf, out[1] = c.cl, out[2] = c.total;
	}
	// ... of a scan that is voxel-down-sampled ahead of the ground filter (a sub-batch of one), and the ground arena it is measured against
	void eb_scan_cost_vox(uint32_t n, int prefilter, int voxels, int normal_method, int fixed_num, int unground_down_fixed_num, uint32_t K, uint64_t *out)
	{
		const ScanCost c = extract_batch_scan_cost(n, prefilter != 0, normal_method, fixed_num != 0, unground_down_fixed_num, K, voxels != 0);
		out[0] = c.gf, out[1] = c.cl, out[2] = c.total;
	}
	uint64_t eb_gf_total_vox(uint32_t n, int prefilter, int voxels, int normal_method) { return gf_layout(n, prefilter != 0, voxels != 0, normal_method).total; }
	// the cuts with at most max_scans scans per sub-batch (1: the scan-local steps)
	uint32_t eb_cuts_max(const uint64_t *bytes, uint32_t count, uint64_t limit, uint32_t max_scans, uint32_t *out)
	{
		std::vector<uint32_t> cuts;
		extract_batch_cuts(bytes, count, limit, &cuts, max_scans);
		for (size_t k = 0; k < cuts.size(); k++)
			out[k] = cuts[k];
		return (uint32_t)cuts.size();
	}
	uint32_t eb_ex_count(void) { return MULLS_EX_COUNT; }
	// out: MULLS_EX_COUNT offsets, where the selection indices start, the bytes the block needs
	void eb_block_layout(const uint32_t *cnt, uint64_t n_idx, uint64_t *out)
	{
		const BlockLayout b = block_layout(cnt, (size_t)n_idx);
		for (int k = 0; k < MULLS_EX_COUNT; k++)
			out[k] = b.off[k];
		out[MULLS_EX_COUNT] = b.o_idx, out[MULLS_EX_COUNT + 1] = b.need;
	}
	uint32_t eb_cuts(const uint64_t *bytes, uint32_t count, uint64_t limit, uint32_t *out)
	{
		std::vector<uint32_t> cuts;
		extract_batch_cuts(bytes, count, limit, &cuts);
		for (size_t k = 0; k < cuts.size(); k++)
			out[k] = cuts[k];
		return (uint32_t)cuts.size();
	}
	// cost: 3 words per scan as eb_scan_cost writes them; out: 2 words per scan (offsets of the ground and the classify region).  Returns the arena's bytes.
	uint64_t eb_offsets(const uint64_t *cost, uint32_t count, uint32_t first, uint32_t last, uint64_t *out)
	{
		std::vector<ScanCost> c(count);
		std::vector<ScanRegion> r(count);
		for (uint32_t b = 0; b < count; b++)
			c[b].gf = cost[3 * b], c[b].cl = cost[3 * b + 1], c[b].total = cost[3 * b + 2];
		const uint64_t bytes = extract_batch_offsets(c.data(), first, last, r.data());
		for (uint32_t b = first; b < last; b++)
			out[2 * b] = r[b].o_gf, out[2 * b + 1] = r[b].o_cl;
		return bytes;
	}
}

#ifdef EB_MAIN
// the properties tests/test_extract_batch.py asserts through the library, on the same inputs
#define EB_REQUIRE(cond)                                                \
	do                                                                  \
	{                                                                   \
		if (!(cond))                                                    \
		{                                                               \
			std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
			return 1;                                                   \
		}                                                               \
	} while (0)
int main()
{
	const uint32_t sizes[] = {6375, 0, 22400, 19182, 1025, 0, 964, 3125, 200, 500, 121000, 1};
	const uint32_t count = sizeof(sizes) / sizeof(sizes[0]);
	for (int shape = 0; shape < 2; shape++)
	{
		const int prefilter = shape, method = shape ? 3 : 0, fixed = shape, ufn = 3000;
		std::vector<uint64_t> cost(3 * count), bytes(count);
		for (uint32_t b = 0; b < count; b++)
		{
			eb_scan_cost(sizes[b], prefilter, method, fixed, ufn, 50, &cost[3 * b]);
			bytes[b] = cost[3 * b + 2];
			if (sizes[b])
			{
				EB_REQUIRE(cost[3 * b] == up256(eb_gf_total(sizes[b], prefilter, method)));
				EB_REQUIRE(cost[3 * b + 1] == up256(eb_cl_total(eb_work_points(sizes[b], fixed, ufn), 50, sizes[b])));
				EB_REQUIRE(cost[3 * b + 2] == cost[3 * b] + cost[3 * b + 1] + MULLS_EXB_TABLE_BYTES);
			}
			else
				EB_REQUIRE(cost[3 * b] == 0 && cost[3 * b + 1] == 0 && cost[3 * b + 2] == MULLS_EXB_TABLE_BYTES);
		}
		uint64_t all = MULLS_EXB_HEAD_BYTES;
		for (uint32_t b = 0; b < count; b++)
			all += bytes[b];
		const uint64_t limits[] = {1, bytes[0], bytes[0] + bytes[1] + bytes[2] + MULLS_EXB_HEAD_BYTES, all / 3, all - 1, all, ~(uint64_t)0};
		for (uint64_t limit : limits)
		{
			std::vector<uint32_t> cuts(count + 2);
			const uint32_t k = eb_cuts(bytes.data(), count, limit, cuts.data());
			EB_REQUIRE(k >= 2 && cuts[0] == 0 && cuts[k - 1] == count);
			for (uint32_t c = 0; c + 1 < k; c++)
			{
				EB_REQUIRE(cuts[c] < cuts[c + 1]);
				std::vector<uint64_t> off(2 * count);
				const uint64_t arena = eb_offsets(cost.data(), count, cuts[c], cuts[c + 1], off.data());
				EB_REQUIRE(arena <= limit || cuts[c + 1] == cuts[c] + 1);
				uint64_t at = MULLS_EXB_HEAD_BYTES + (uint64_t)MULLS_EXB_TABLE_BYTES * (cuts[c + 1] - cuts[c]);
				for (uint32_t b = cuts[c]; b < cuts[c + 1]; b++)
				{
					EB_REQUIRE(off[2 * b] % 256 == 0 && off[2 * b + 1] % 256 == 0);
					EB_REQUIRE(off[2 * b] == at && off[2 * b + 1] == at + cost[3 * b]);
					at += cost[3 * b] + cost[3 * b + 1];
				}
				EB_REQUIRE(at == arena);
			}
		}
	}
	// the voxel flag: never cheaper, and the ground arena gf_layout gives with it
	for (uint32_t n : sizes)
		for (int method = 0; method < 4; method++)
		{
			uint64_t with[3], without[3];
			eb_scan_cost_vox(n, 1, 1, method, 1, 3000, 50, with);
			eb_scan_cost_vox(n, 1, 0, method, 1, 3000, 50, without);
			EB_REQUIRE(with[0] >= without[0] && with[1] == without[1] && with[2] == with[0] + with[1] + MULLS_EXB_TABLE_BYTES);
			EB_REQUIRE(with[0] == (n ? up256(eb_gf_total_vox(n, 1, 1, method)) : 0u));
		}
	// the one-scan cut rule: `count` sub-batches whatever the limit
	{
		std::vector<uint64_t> bytes(count, MULLS_EXB_TABLE_BYTES);
		bytes[3] = (uint64_t)1 << 33;
		for (uint64_t limit : {(uint64_t)1, (uint64_t)1 << 20, ~(uint64_t)0})
		{
			std::vector<uint32_t> cuts(count + 2);
			EB_REQUIRE(eb_cuts_max(bytes.data(), count, limit, 1, cuts.data()) == count + 1);
			for (uint32_t b = 0; b <= count; b++)
				EB_REQUIRE(cuts[b] == b);
		}
	}
	// the block layout against the two forms it replaces: the offsets' loop, and the indices 128 bytes + their own size ahead of the end
	{
		const uint32_t counts[][3] = {{0, 0, 0}, {16, 0, 5}, {4097, 2049, 0}, {1, 1, 1}, {121000, 60500, 20000}}; // 16 records: 768 bytes, a multiple of 256 already
		for (const uint32_t *c : counts)
		{
			uint32_t cnt[MULLS_EX_COUNT];
			for (int k = 0; k < MULLS_EX_COUNT; k++)
				cnt[k] = c[k % 3] + (k > 8 ? (uint32_t)k : 0u) * (c[0] ? 1u : 0u);
			const uint64_t n_idx = c[1];
			uint64_t got[MULLS_EX_COUNT + 2], need = 0;
			eb_block_layout(cnt, n_idx, got);
			for (int k = 0; k < MULLS_EX_COUNT; k++)
			{
				EB_REQUIRE(got[k] == need && got[k] % 256 == 0);
				need += ((uint64_t)cnt[k] * MULLS_POINT_BYTES + 255) & ~(uint64_t)255;
			}
			need += n_idx * 4 + 256;
			EB_REQUIRE(got[MULLS_EX_COUNT + 1] == need && got[MULLS_EX_COUNT] == need - (n_idx * 4 + 128));
		}
	}
	std::vector<uint32_t> none(2);
	EB_REQUIRE(eb_cuts(nullptr, 0, 1, none.data()) == 1 && none[0] == 0);
	std::printf("extract_batch_harness: OK\n");
	return 0;
}
#endif
