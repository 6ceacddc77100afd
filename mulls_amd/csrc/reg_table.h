// reg_table.h — the cell table of the registrations (mulls_gicp, mulls_pcl_icp; mulls_fpfh, where a cloud stands for a problem): a hash table of occupied cells over one cloud, open addressing with
// linear probing over 64-bit packed cell coordinates, and the cloud's points in cell order.  The descriptor (written by the host, read by the kernels of
// k_reg_table.hip and by every kernel that walks a table), the per-problem head the table kernels and the methods' own kernels share, and the one
// function that lays a table out.  Host and device, without the HIP runtime, so that a harness under tests/ can hold the layout on the CPU.
#pragma once
#include <stdint.h>

#define MULLS_REG_SEG 1024u // threads of the one-workgroup-per-table scan; a table has a multiple of this many slots
#define MULLS_REG_TABS 3	// tables of a problem: table tb of problem p is tabs[MULLS_REG_TABS * p + tb]

enum RegCoordRule
{
	REG_COORD_CELL = 0, // floor((double)x * inv_edge): pcl_icp::cell_coord
	REG_COORD_VOXEL = 1 // floorf(x / resolution - 0.5f): gicp::voxel_coord
};
struct RegTab
{
	uint32_t n_cap;		   // the cloud's points before the crop: the bound of every per-point loop; 0: the table is not built
	uint32_t slots, shift; // a power of two >= max(2 n_cap, MULLS_REG_SEG); 64 - log2(slots)
	uint32_t cloud;		   // whose cropped count bounds the table: 0 the source's, 1 the target's (RegHead::n)
	uint32_t rule;		   // RegCoordRule
	uint32_t refuses;	   // a point outside the packed key's range refuses the problem (else it takes no part)
	uint32_t rebuilt;	   // cleared and built again while the problem runs: takes part only while it does
	float resolution;	   // REG_COORD_VOXEL
	double inv_edge;	   // REG_COORD_CELL
	uint64_t o_pts;		   // packed float xyz
	uint64_t o_cell, o_list; // per point: its slot; the points of every slot
	uint64_t o_sorted;		 // packed float xyz in the order of o_list; 0: no such copy
	uint64_t o_keys;		 // uint64 a slot: the packed cell coordinates, all ones where free
	uint64_t o_count, o_start, o_fill; // uint32 a slot: points, first entry in list, fill counter
};

// what the table kernels need to know of a problem, whichever method runs it; the method's begin and decide kernels keep it
struct RegHead
{
	int32_t status;					  // 0: the problem takes part (every method's *_ST_OK)
	uint32_t range;					  // set when a point of a refusing table lies outside the packed key's range
	int32_t running;				  // the method's State::running
	uint32_t n[2];					  // points after the crop: source, target
	uint32_t occupied[MULLS_REG_TABS]; // occupied slots of a table, once it has been scanned
};

// The slot rule and the order of a table's arrays, in this one place.  take(bytes) -> offset hands out the arena; the arrays cleared on the device
// (keys: 8 bytes a slot; count, start, fill: 4 bytes a slot) are cleared slot by slot, so nothing depends on where take puts them.
template <typename Take>
inline void reg_table_lay_out(RegTab &T, uint64_t n, uint64_t o_pts, bool sorted, Take &&take)
{
	uint32_t slots = MULLS_REG_SEG, lg = 10;
	while ((uint64_t)slots < 2 * n)
		slots <<= 1, lg++;
	T.n_cap = (uint32_t)n, T.slots = slots, T.shift = 64u - lg;
	T.o_pts = o_pts;
	T.o_cell = take(4 * n), T.o_list = take(4 * n);
	T.o_sorted = sorted ? take(12 * n) : 0;
	T.o_keys = take(8ull * slots);
	T.o_count = take(4ull * slots), T.o_start = take(4ull * slots), T.o_fill = take(4ull * slots);
}
