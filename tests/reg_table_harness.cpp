// reg_table_harness.cpp — the layout of a registration cell table (mulls_amd/csrc/reg_table.h) held on the CPU, as a program of its own: tests/test_reg_table.py
// builds it with -fsanitize=address,undefined and runs it.  For every n given on the command line, with and without the coordinate copy, from an arena
// that starts at 0 (the dry layout that sizes a problem) and from one that starts further on (the real one): the slot rule, the shift, every array
// 256-aligned, inside its own block and apart from every other, the arrays the device clears (k_reg_clear writes entries 0 .. slots - 1 of keys, count,
// start and fill) filling their blocks exactly, o_sorted = 0 when no copy is asked for, and the same byte count from both arenas.  Prints one line a
// case; exit status 1 with the failed expectation on stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mulls_amd/csrc/reg_table.h"
#include "../mulls_amd/csrc/subbatch.h"

namespace
{
struct Piece
{
	uint64_t at, bytes;
};
// hands out offsets as the hosts' arenas do and remembers every block
struct Arena
{
	uint64_t off;
	std::vector<Piece> taken;
	uint64_t operator()(uint64_t bytes)
	{
		const uint64_t at = off;
		off += up256(bytes);
		taken.push_back({at, bytes});
		return at;
	}
};

#define EXPECT(cond)                                                                                          \
	do                                                                                                        \
	{                                                                                                         \
		if (!(cond))                                                                                          \
		{                                                                                                     \
			std::fprintf(stderr, "n = %llu, sorted = %d, base = %llu: %s\n", (unsigned long long)n, (int)sorted, (unsigned long long)base, #cond); \
			std::exit(1);                                                                                     \
		}                                                                                                     \
	} while (0)

// -> the bytes the table took
uint64_t one(uint64_t n, bool sorted, uint64_t base)
{
	Arena arena{base, {}};
	RegTab T;
	std::memset(&T, 0xa5, sizeof(T)); // (what the layout does not set is the caller's; what it sets it sets whatever was there)
	reg_table_lay_out(T, n, 12345u * 256u, sorted, arena);
	EXPECT(T.n_cap == n && T.o_pts == 12345u * 256u);
	// the slot rule: the smallest power of two >= max(2 n, 1024), and the shift that leaves log2(slots) bits of a 64-bit mix
	EXPECT(T.slots >= 1024u && (T.slots & (T.slots - 1u)) == 0u && (uint64_t)T.slots >= 2 * n);
	EXPECT(T.slots == 1024u || (uint64_t)T.slots / 2 < 2 * n);
	EXPECT(T.shift < 64u && (1ull << (64u - T.shift)) == T.slots);
	EXPECT(T.slots % MULLS_REG_SEG == 0u);
	// every array: where it is, how many bytes the kernels may touch
	struct
	{
		const char *name;
		uint64_t at, bytes;
	} arrays[] = {{"cell", T.o_cell, 4 * n},		   {"list", T.o_list, 4 * n},			{"sorted", T.o_sorted, sorted ? 12 * n : 0},
				  {"keys", T.o_keys, 8ull * T.slots}, {"count", T.o_count, 4ull * T.slots}, {"start", T.o_start, 4ull * T.slots},
				  {"fill", T.o_fill, 4ull * T.slots}};
	EXPECT(sorted || T.o_sorted == 0);
	EXPECT(arena.taken.size() == (sorted ? 7u : 6u));
	size_t next = 0;
	for (const auto &a : arrays)
	{
		if (!sorted && !std::strcmp(a.name, "sorted"))
			continue;
		// the order of the arrays is the order of the blocks; an array is its block: same start, same bytes (so the cleared arrays fill theirs exactly)
		const Piece &p = arena.taken[next++];
		EXPECT(a.at == p.at && a.bytes == p.bytes);
		EXPECT(a.at % 256u == 0u && a.at >= base && a.at + a.bytes <= arena.off);
	}
	for (size_t i = 0; i < arena.taken.size(); i++)
		for (size_t k = i + 1; k < arena.taken.size(); k++)
		{
			const Piece &a = arena.taken[i], &b = arena.taken[k];
			EXPECT(a.at + a.bytes <= b.at || b.at + b.bytes <= a.at);
		}
	return arena.off - base;
}
} // namespace

int main(int argc, char **argv)
{
	int cases = 0;
	for (int k = 1; k < argc; k++)
	{
		const uint64_t n = std::strtoull(argv[k], nullptr, 10);
		for (int sorted = 0; sorted < 2; sorted++)
		{
			const uint64_t dry = one(n, sorted != 0, 0), real = one(n, sorted != 0, 7u * 256u), far = one(n, sorted != 0, 1ull << 33);
			if (dry != real || dry != far)
			{
				std::fprintf(stderr, "n = %llu, sorted = %d: the dry layout takes %llu bytes, the real one %llu and %llu\n", (unsigned long long)n, sorted,
							 (unsigned long long)dry, (unsigned long long)real, (unsigned long long)far);
				return 1;
			}
			std::printf("%llu %d %llu\n", (unsigned long long)n, sorted, (unsigned long long)dry);
			cases++;
		}
	}
	std::printf("ok %d\n", cases);
	return 0;
}
