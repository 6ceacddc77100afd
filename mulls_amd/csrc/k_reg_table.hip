// k_reg_table.hip — the cell tables of mulls_gicp and mulls_pcl_icp (reg_table.h) built on the device (gfx950).  One launch of each kernel serves tables
// first .. first + count - 1 of every problem of a sub-batch: blockIdx.y (blockIdx.x for the scan, a workgroup per table) is the problem and the table.
// k_reg_clear empties a table, k_reg_cells gives every point its cell's slot (claimed by compare-and-swap) and counts, k_reg_offsets scans the counts,
// k_reg_scatter writes every slot's points to its list (and their coordinates in that order, for a table that keeps them).  Atomics place entries; the
// order inside a slot is arrival order until a kernel that needs one sorts it.  Every loop is bounded by a descriptor field or a constant.
#include <hip/hip_runtime.h>

#include "reg_device.h"
#include "reg_launch.h"

namespace
{
__global__ void __launch_bounds__(256) k_reg_clear(const RegTab *__restrict__ tabs, unsigned char *arena, const RegHead *__restrict__ head, int first, int count)
{
	const uint32_t p = blockIdx.y / count, tb = first + blockIdx.y % count;
	const RegTab T = tabs[MULLS_REG_TABS * p + tb];
	if (!table_live(head[p], T))
		return;
	const uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s >= T.slots)
		return;
	at<uint64_t>(arena, T.o_keys)[s] = EMPTY;
	at<uint32_t>(arena, T.o_count)[s] = 0u, at<uint32_t>(arena, T.o_start)[s] = 0u, at<uint32_t>(arena, T.o_fill)[s] = 0u;
}

__global__ void __launch_bounds__(256) k_reg_cells(const RegTab *__restrict__ tabs, unsigned char *arena, RegHead *head, int first, int count)
{
	const uint32_t p = blockIdx.y / count, tb = first + blockIdx.y % count;
	RegHead &H = head[p];
	const RegTab T = tabs[MULLS_REG_TABS * p + tb];
	if (!table_live(H, T))
		return;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= points_of(H, T))
		return;
	const float *P3 = at<const float>(arena, T.o_pts);
	int ok = 1;
	const int32_t c0 = table_coord(T, P3[3 * i], &ok), c1 = table_coord(T, P3[3 * i + 1], &ok), c2 = table_coord(T, P3[3 * i + 2], &ok);
	uint32_t found = NO_SLOT;
	if (ok)
		found = claim_slot(at<unsigned long long>(arena, T.o_keys), gicp::pack_coords(c0, c1, c2), T.slots, T.shift);
	else if (T.refuses)
		atomicOr(&H.range, 1u); // does not fit the packed key: refused by the host, never wrapped
	at<uint32_t>(arena, T.o_cell)[i] = found;
	if (found != NO_SLOT)
		atomicAdd(&at<uint32_t>(arena, T.o_count)[found], 1u);
}

__global__ void __launch_bounds__(MULLS_REG_SEG) k_reg_offsets(const RegTab *__restrict__ tabs, unsigned char *arena, RegHead *head, int first, int count)
{
	__shared__ uint32_t s_cnt[MULLS_REG_SEG], s_occ[MULLS_REG_SEG];
	const uint32_t p = blockIdx.x / count, tb = first + blockIdx.x % count;
	const RegTab T = tabs[MULLS_REG_TABS * p + tb];
	if (!table_live(head[p], T))
		return;
	const uint32_t cells = scan_counts(at<const uint32_t>(arena, T.o_count), at<uint32_t>(arena, T.o_start), T.slots, s_cnt, s_occ);
	if (threadIdx.x == 0)
		head[p].occupied[tb] = cells;
}

__global__ void __launch_bounds__(256) k_reg_scatter(const RegTab *__restrict__ tabs, unsigned char *arena, const RegHead *__restrict__ head, int first, int count)
{
	const uint32_t p = blockIdx.y / count, tb = first + blockIdx.y % count;
	const RegTab T = tabs[MULLS_REG_TABS * p + tb];
	if (!table_live(head[p], T))
		return;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= points_of(head[p], T))
		return;
	const uint32_t pos = list_point(at<const uint32_t>(arena, T.o_cell), at<const uint32_t>(arena, T.o_start), at<uint32_t>(arena, T.o_fill), at<uint32_t>(arena, T.o_list),
									 T.slots, T.n_cap, i);
	if (pos == NO_SLOT)
		return;
	if (T.o_sorted)
	{
		const float *P3 = at<const float>(arena, T.o_pts);
		float *Q3 = at<float>(arena, T.o_sorted);
		Q3[3 * pos] = P3[3 * i], Q3[3 * pos + 1] = P3[3 * i + 1], Q3[3 * pos + 2] = P3[3 * i + 2];
	}
}
} // namespace

hipError_t launch_reg_tables(hipStream_t st, const RegTab *tabs, uint32_t P, int first, int count, uint32_t n_max, uint32_t slots_max, unsigned char *arena,
							 RegHead *head)
{
	const uint32_t tables = (uint32_t)count * P;
	hipLaunchKernelGGL(k_reg_clear, dim3(blocks_of(slots_max, 256), tables), dim3(256), 0, st, tabs, arena, head, first, count);
	hipLaunchKernelGGL(k_reg_cells, dim3(blocks_of(n_max, 256), tables), dim3(256), 0, st, tabs, arena, head, first, count);
	hipLaunchKernelGGL(k_reg_offsets, dim3(tables), dim3(MULLS_REG_SEG), 0, st, tabs, arena, head, first, count);
	hipLaunchKernelGGL(k_reg_scatter, dim3(blocks_of(n_max, 256), tables), dim3(256), 0, st, tabs, arena, head, first, count);
	return hipGetLastError();
}
