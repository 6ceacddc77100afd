// reg_launch.h — the launch of the cell-table kernels (k_reg_table.hip) that gicp.cpp and pcl_icp.cpp share
#pragma once
#include <hip/hip_runtime_api.h>

#include "reg_table.h"

// Tables first .. first + count - 1 of every problem, each kernel launched once for all of them: the clear, cells, the scan, the scatter.
// n_max and slots_max bound those tables' points and slots over the sub-batch.
hipError_t launch_reg_tables(hipStream_t st, const RegTab *tabs, uint32_t P, int first, int count, uint32_t n_max, uint32_t slots_max, unsigned char *arena,
							 RegHead *head);
