// A stand-alone program over mulls_amd/csrc/fpfh_batch.h (the planner of mulls_coarse_reg_fpfhsac_batch: host code without HIP) for
// tests/test_fpfh_batch.py.  Numbers go out one line a record.
//   bytes iters n_src n_tgt                  -> problem_bytes cloud_bytes(n_src) cloud_bytes(n_tgt) HEAD_BYTES MAX_SLOTS MAX_POOL_BYTES
//   cuts limit iters (n_src n_tgt)...         -> the cuts of the problems into sub-batches (sub_batch_cuts as fpfh.cpp calls it)
//   pool limit iters counted n_src...         -> pool_bytes
//   stretches pool iters n_src...             -> a line a stretch: h0 n d0 bytes n_src_max
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../mulls_amd/csrc/fpfh_batch.h"

int main(int argc, char **argv)
{
	if (argc < 4)
		return 2;
	auto num = [&](int k) { return strtoull(argv[k], nullptr, 10); };
	if (!strcmp(argv[1], "bytes") && argc == 5)
	{
		printf("%llu %llu %llu %llu %u %llu\n", (unsigned long long)fpfh_batch::problem_bytes(num(3), num(4), num(2)), (unsigned long long)fpfh_batch::cloud_bytes(num(3)),
			   (unsigned long long)fpfh_batch::cloud_bytes(num(4)), (unsigned long long)fpfh_batch::HEAD_BYTES, fpfh_batch::MAX_SLOTS,
			   (unsigned long long)fpfh_batch::MAX_POOL_BYTES);
		return 0;
	}
	if (!strcmp(argv[1], "cuts"))
	{
		std::vector<uint64_t> bytes;
		for (int k = 4; k + 1 < argc; k += 2)
			bytes.push_back(fpfh_batch::problem_bytes(num(k), num(k + 1), num(3)));
		std::vector<uint32_t> cuts;
		sub_batch_cuts(bytes.data(), (uint32_t)bytes.size(), num(2), fpfh_batch::MAX_SLOTS, &cuts, fpfh_batch::HEAD_BYTES);
		for (uint32_t c : cuts)
			printf("%u\n", c);
		return 0;
	}
	std::vector<uint32_t> ns;
	if (!strcmp(argv[1], "pool"))
	{
		for (int k = 5; k < argc; k++)
			ns.push_back((uint32_t)num(k));
		printf("%llu\n", (unsigned long long)fpfh_batch::pool_bytes(ns.data(), (uint32_t)ns.size(), (uint32_t)num(3), num(4), num(2)));
		return 0;
	}
	if (!strcmp(argv[1], "stretches"))
	{
		for (int k = 4; k < argc; k++)
			ns.push_back((uint32_t)num(k));
		std::vector<fpfh_batch::Stretch> out;
		fpfh_batch::stretches(ns.data(), (uint32_t)ns.size(), (uint32_t)num(3), num(2), &out);
		for (const fpfh_batch::Stretch &S : out)
			printf("%u %u %llu %llu %u\n", S.h0, S.n, (unsigned long long)S.d0, (unsigned long long)S.bytes, S.n_src_max);
		return 0;
	}
	return 2;
}
