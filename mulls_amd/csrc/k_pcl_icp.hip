// k_pcl_icp.hip — the device side of mulls_pcl_icp / mulls_pcl_icp_batch (gfx950).  One launch of each kernel serves every problem of a sub-batch:
// blockIdx.y is the problem for the per-point, per-slot and per-cell kernels, blockIdx.x for those that give a problem one workgroup.  The crop and the
// nearest-neighbour pass of the fitness are k_ndt.hip's.  Setup: tables of occupied cells (k_reg_table.hip, reg_table.h, with the coordinates
// copied into cell order) and, for Point2Plane, the normals: every cell's list sorted (k_pcl_icp_sort), then one
// workgroup per cell that merges its 27 lists through LDS tiles in ascending index (k_pcl_icp_normals).  A tick: the moved source re-binned when the
// correspondences are reciprocal, k_pcl_icp_search (the hot path: the exact nearest target point within the distance, 27 cells, ties by index),
// k_pcl_icp_recip, k_pcl_icp_accum (and k_pcl_icp_cross for Point2Point: the centroids come first) into strided partials, k_pcl_icp_decide (the tree,
// pcl_icp_math.h's step and stop rules on one lane, then the source moved by the whole workgroup).  Atomics place entries and count; they never decide
// an order of additions.  No kernel waits for another workgroup.  Every loop is bounded by a descriptor field, a launch argument or a constant.
#include <hip/hip_runtime.h>

#include "pcl_icp_launch.h"
#include "reg_device.h"

namespace
{
constexpr uint32_t NO_POINT = 0xffffffffu;
constexpr uint32_t TILE = MULLS_PCL_ICP_TILE;

__global__ void __launch_bounds__(64) k_pcl_icp_begin(const NdtRec *__restrict__ nrec, PclIcpRec *rec, RegHead *head, double *frames, uint32_t P)
{
	const uint32_t p = blockIdx.x * 64u + threadIdx.x;
	if (p >= P)
		return;
	PclIcpRec &R = rec[p];
	RegHead H{};
	H.n[0] = nrec[p].n_src, H.n[1] = nrec[p].n_tgt;
	R.n_fit = 0, R.fitness = 0.0, R.pad = 0;
	int status = PCL_ICP_ST_OK;
	if (nrec[p].status == NDT_ST_NONFINITE)
		status = PCL_ICP_ST_NONFINITE;
	else if (nrec[p].status != NDT_ST_OK || H.n[0] == 0 || H.n[1] == 0)
		status = PCL_ICP_ST_EMPTY;
	H.status = status;
	pcl_icp::State S;
	pcl_icp::begin(S);
	if (status != PCL_ICP_ST_OK)
		S.running = 0;
	R.S = S;
	H.running = S.running;
	head[p] = H;
	for (int k = 0; k < 9; k++)
		frames[12u * p + k] = S.R[k];
	for (int k = 0; k < 3; k++)
		frames[12u * p + 9 + k] = S.t[k];
}

// the moved source starts as the cropped source; a source point outside the cells' range refuses the problem
__global__ void __launch_bounds__(256) k_pcl_icp_copy(const PclIcpDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena, RegHead *head)
{
	const uint32_t p = blockIdx.y;
	RegHead &H = head[p];
	if (H.status != PCL_ICP_ST_OK)
		return;
	const PclIcpDesc &D = desc[p];
	const uint32_t ns = H.n[0] < D.n_src_cap ? H.n[0] : D.n_src_cap;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ns)
		return;
	const float *S3 = at<const float>(arena, D.o_src);
	float *M3 = at<float>(arena, D.o_mov);
	const float x = S3[3 * i], y = S3[3 * i + 1], z = S3[3 * i + 2];
	M3[3 * i] = x, M3[3 * i + 1] = y, M3[3 * i + 2] = z;
	int ok = 1;
	const double inv = tabs[MULLS_REG_TABS * p + PCL_ICP_TAB_TGT].inv_edge;
	(void)pcl_icp::cell_coord(x, inv, &ok), (void)pcl_icp::cell_coord(y, inv, &ok), (void)pcl_icp::cell_coord(z, inv, &ok);
	if (!ok)
		atomicOr(&H.range, 1u);
}

// one lane per occupied slot of the normals' table: its points' indices ascending
__global__ void __launch_bounds__(256) k_pcl_icp_sort(const RegTab *__restrict__ tabs, unsigned char *arena, const RegHead *__restrict__ head)
{
	const uint32_t p = blockIdx.y;
	const RegHead &H = head[p];
	const RegTab T = tabs[MULLS_REG_TABS * p + PCL_ICP_TAB_NRM];
	if (!table_live(H, T) || H.range)
		return;
	const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
	if (slot >= T.slots)
		return;
	const uint32_t n = at<const uint32_t>(arena, T.o_count)[slot];
	if (!n)
		return;
	const uint32_t first = at<const uint32_t>(arena, T.o_start)[slot];
	if (first >= T.n_cap || n > T.n_cap - first)
		return;
	sort_list(at<uint32_t>(arena, T.o_list) + first, n);
}

// The normals.  One workgroup per occupied cell; a thread per point of the cell (256 at a time).  The neighbours of those points lie in the 27 cells
// around it, whose sorted lists are merged window by window: a window is TILE consecutive target indices, the lists' entries inside it are flagged,
// compacted in index order into an LDS tile of coordinates, and every thread walks the tile.  So a point adds its neighbours in ascending index
// whatever their number; two passes (the sum, then the scatter about the mean), then pcl_icp_math.h's normal.
__global__ void __launch_bounds__(256) k_pcl_icp_normals(const PclIcpDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena, PclIcpOpts opt,
														 const RegHead *__restrict__ head)
{
	__shared__ uint32_t s_beg[27], s_end[27], s_cur[27], s_lo[27], s_hi[27];
	__shared__ uint32_t s_flag[TILE], s_wave[4];
	__shared__ float s_tile[TILE][3];
	const uint32_t p = blockIdx.y, slot = blockIdx.x, t = threadIdx.x;
	const RegHead &H = head[p];
	const RegTab T = tabs[MULLS_REG_TABS * p + PCL_ICP_TAB_NRM];
	if (!table_live(H, T) || H.range || slot >= T.slots)
		return;
	const uint32_t n = points_of(H, T);
	const uint64_t *keys = at<const uint64_t>(arena, T.o_keys);
	const uint32_t *start = at<const uint32_t>(arena, T.o_start), *count = at<const uint32_t>(arena, T.o_count), *list = at<const uint32_t>(arena, T.o_list);
	const uint32_t cnt = count[slot], first = start[slot];
	if (!cnt || first >= n || cnt > n - first)
		return;
	const float *P3 = at<const float>(arena, T.o_pts);
	float *N3 = at<float>(arena, desc[p].o_nrm);
	if (t < 27u)
	{
		const uint64_t key = keys[slot];
		const int32_t cx = (int32_t)(key & 0x1fffffu) - 1048576, cy = (int32_t)((key >> 21) & 0x1fffffu) - 1048576, cz = (int32_t)((key >> 42) & 0x1fffffu) - 1048576;
		uint32_t b = 0, e = 0;
		visit_cells(keys, T.slots, T.shift, cx, cy, cz, (int)t, (int)t + 1, [&](int, uint32_t s) { // (thread t: the t-th of the 27 lists)
			if (start[s] < n && count[s] <= n - start[s])
				b = start[s], e = b + count[s];
		});
		s_beg[t] = b, s_end[t] = e;
	}
	__syncthreads();
	for (uint32_t q0 = 0; q0 < cnt; q0 += 256u)
	{
		const bool have = q0 + t < cnt;
		uint32_t qi = have ? list[first + q0 + t] : 0u;
		qi = qi < n ? qi : 0u;
		const float qx = P3[3 * qi], qy = P3[3 * qi + 1], qz = P3[3 * qi + 2];
		double s[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0}, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
		uint32_t k = 0;
		for (int pass = 0; pass < 2; pass++)
		{
			if (t < 27u)
				s_cur[t] = s_beg[t];
			__syncthreads();
			for (uint32_t base = 0; base < n; base += TILE)
			{
				if (t < 27u)
				{
					// the first entry of the list at or above the window's end
					uint32_t lo = s_cur[t], hi = s_end[t];
					for (int it = 0; it < 32 && lo < hi; it++)
					{
						const uint32_t mid = lo + (hi - lo) / 2u;
						if (list[mid] < base + TILE)
							lo = mid + 1u;
						else
							hi = mid;
					}
					s_lo[t] = s_cur[t], s_hi[t] = lo, s_cur[t] = lo;
				}
				s_flag[t] = 0u;
				__syncthreads();
				uint32_t total = 0;
				for (int l = 0; l < 27; l++)
					total += s_hi[l] - s_lo[l];
				if (!total)
				{
					__syncthreads();
					continue;
				}
				for (int l = 0; l < 27; l++)
				{
					const uint32_t e = s_lo[l] + t;
					if (e < s_hi[l])
					{
						const uint32_t j = list[e];
						if (j >= base && j - base < TILE)
							s_flag[j - base] = 1u;
					}
				}
				__syncthreads();
				const bool present = s_flag[t] != 0u && base + t < n;
				const unsigned long long mask = __ballot(present);
				if ((t & 63u) == 0u)
					s_wave[t >> 6] = (uint32_t)__popcll(mask);
				__syncthreads();
				uint32_t off = 0, in_tile = 0;
				for (uint32_t w = 0; w < 4u; w++)
				{
					off += w < (t >> 6) ? s_wave[w] : 0u;
					in_tile += s_wave[w];
				}
				if (present)
				{
					const uint32_t pos = off + (uint32_t)__popcll(mask & ((1ull << (t & 63u)) - 1ull)), j = base + t;
					s_tile[pos][0] = P3[3 * j], s_tile[pos][1] = P3[3 * j + 1], s_tile[pos][2] = P3[3 * j + 2];
				}
				__syncthreads();
				for (uint32_t j = 0; j < in_tile && j < TILE; j++)
				{
					const float x = s_tile[j][0], y = s_tile[j][1], z = s_tile[j][2];
					if (!((double)pcl_icp::dist2(x, y, z, qx, qy, qz) <= opt.radius2))
						continue;
					if (pass == 0)
					{
						gicp::sum_add(s, (double)x, (double)y, (double)z);
						k++;
					}
					else
						gicp::scatter_add(S, m, (double)x, (double)y, (double)z);
				}
				__syncthreads();
			}
			if (pass == 0 && k >= 3u)
				gicp::mean_of(s, (int)k, m);
		}
		if (have)
		{
			float nv[3] = {0.577f, 0.577f, 0.577f};
			if (k >= 3u)
				pcl_icp::normal_of_scatter(S, (double)qx, (double)qy, (double)qz, nv);
			N3[3 * qi] = nv[0], N3[3 * qi + 1] = nv[1], N3[3 * qi + 2] = nv[2];
		}
	}
}

// The loop's hot path.  One lane per moved source point: the 27 cells around its own, every target point in them, the smallest by (float d2, index);
// no pair when the distance is above the threshold.
__global__ void __launch_bounds__(256) k_pcl_icp_search(const PclIcpDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena, PclIcpOpts opt,
														const PclIcpRec *__restrict__ rec, const RegHead *__restrict__ head)
{
	const uint32_t p = blockIdx.y;
	const RegHead &H = head[p];
	if (!rec[p].S.running || H.range)
		return;
	const PclIcpDesc &D = desc[p];
	const RegTab T = tabs[MULLS_REG_TABS * p + PCL_ICP_TAB_TGT];
	const uint32_t ns = H.n[0] < D.n_src_cap ? H.n[0] : D.n_src_cap, nt = points_of(H, T);
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ns)
		return;
	const float *M3 = at<const float>(arena, D.o_mov), *Q3 = at<const float>(arena, T.o_sorted);
	const float qx = M3[3 * i], qy = M3[3 * i + 1], qz = M3[3 * i + 2];
	const uint32_t *start = at<const uint32_t>(arena, T.o_start), *count = at<const uint32_t>(arena, T.o_count), *list = at<const uint32_t>(arena, T.o_list);
	int ok = 1;
	const int32_t cx = pcl_icp::cell_coord(qx, T.inv_edge, &ok), cy = pcl_icp::cell_coord(qy, T.inv_edge, &ok), cz = pcl_icp::cell_coord(qz, T.inv_edge, &ok);
	float best = __builtin_huge_valf();
	uint32_t bi = NO_POINT;
	if (ok)
		visit_cells(at<const uint64_t>(arena, T.o_keys), T.slots, T.shift, cx, cy, cz, 0, 27, [&](int, uint32_t slot) {
			const uint32_t b = start[slot], cnt = count[slot];
			if (b >= nt || cnt > nt - b)
				return;
			for (uint32_t j = b; j < b + cnt; j++)
			{
				const float d2 = pcl_icp::dist2(qx, qy, qz, Q3[3 * j], Q3[3 * j + 1], Q3[3 * j + 2]);
				const uint32_t m = list[j];
				if (m < nt && pcl_icp::before(d2, m, best, bi))
					best = d2, bi = m;
			}
		});
	if (bi != NO_POINT && (double)best > opt.thr2)
		bi = NO_POINT;
	at<int32_t>(arena, D.o_match)[i] = bi == NO_POINT ? -1 : (int32_t)bi;
	at<float>(arena, D.o_d2)[i] = bi == NO_POINT ? 0.f : best;
}

// The reciprocity test.  A source point that beats i at its target point m lies within d(i, m) <= the threshold of m: the 27 cells of the moved
// source around m's cell decide it.  i keeps its pair only if no moved source point is before it by (d2 to m, index).
__global__ void __launch_bounds__(256) k_pcl_icp_recip(const PclIcpDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena,
													   const PclIcpRec *__restrict__ rec, const RegHead *__restrict__ head)
{
	const uint32_t p = blockIdx.y;
	const RegHead &H = head[p];
	if (!rec[p].S.running || H.range)
		return;
	const PclIcpDesc &D = desc[p];
	const RegTab T = tabs[MULLS_REG_TABS * p + PCL_ICP_TAB_SRC];
	if (!T.n_cap)
		return;
	const RegTab &TT = tabs[MULLS_REG_TABS * p + PCL_ICP_TAB_TGT];
	const uint32_t ns = points_of(H, T), nt = points_of(H, TT);
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ns)
		return;
	int32_t *match = at<int32_t>(arena, D.o_match);
	const int32_t m = match[i];
	if (m < 0 || (uint32_t)m >= nt)
		return;
	const float di = at<const float>(arena, D.o_d2)[i];
	const float *G3 = at<const float>(arena, TT.o_pts), *Q3 = at<const float>(arena, T.o_sorted);
	const float tx = G3[3 * m], ty = G3[3 * m + 1], tz = G3[3 * m + 2];
	const uint32_t *start = at<const uint32_t>(arena, T.o_start), *count = at<const uint32_t>(arena, T.o_count), *list = at<const uint32_t>(arena, T.o_list);
	int ok = 1;
	const int32_t cx = pcl_icp::cell_coord(tx, T.inv_edge, &ok), cy = pcl_icp::cell_coord(ty, T.inv_edge, &ok), cz = pcl_icp::cell_coord(tz, T.inv_edge, &ok);
	bool beaten = false;
	if (ok)
		visit_cells(at<const uint64_t>(arena, T.o_keys), T.slots, T.shift, cx, cy, cz, 0, 27, [&](int, uint32_t slot) {
			const uint32_t b = start[slot], cnt = count[slot];
			if (b >= ns || cnt > ns - b)
				return;
			for (uint32_t j = b; j < b + cnt; j++)
				if (pcl_icp::before(pcl_icp::dist2(Q3[3 * j], Q3[3 * j + 1], Q3[3 * j + 2], tx, ty, tz), list[j], di, i))
					beaten = true;
		});
	if (beaten)
		match[i] = -1;
}

// Lane l of the problem's MULLS_NDT_TREE lanes takes the source points l, l + MULLS_NDT_TREE, ..: a pair's terms into the lane's sums.  Point2Plane:
// all 28.  Point2Point: the sums of the paired points and of d2; the cross-covariance follows in k_pcl_icp_cross.
__global__ void __launch_bounds__(256) k_pcl_icp_accum(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *__restrict__ rec,
													   const RegHead *__restrict__ head)
{
	const uint32_t p = blockIdx.y;
	const RegHead &H = head[p];
	if (!rec[p].S.running || H.range)
		return;
	const PclIcpDesc &D = desc[p];
	const uint32_t ns = H.n[0] < D.n_src_cap ? H.n[0] : D.n_src_cap, nt = H.n[1] < D.n_tgt_cap ? H.n[1] : D.n_tgt_cap;
	const float *M3 = at<const float>(arena, D.o_mov), *G3 = at<const float>(arena, D.o_tgt), *N3 = at<const float>(arena, D.o_nrm);
	const int32_t *match = at<const int32_t>(arena, D.o_match);
	const float *d2 = at<const float>(arena, D.o_d2);
	const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
	double acc[pcl_icp::N_SUMS];
#pragma unroll
	for (int k = 0; k < pcl_icp::N_SUMS; k++)
		acc[k] = 0.0;
	uint32_t hits = 0;
	for (uint32_t i = lane; i < ns; i += MULLS_NDT_TREE)
	{
		const int32_t m = match[i];
		if (m < 0 || (uint32_t)m >= nt)
			continue;
		const double s[3] = {(double)M3[3 * i], (double)M3[3 * i + 1], (double)M3[3 * i + 2]};
		const double g[3] = {(double)G3[3 * m], (double)G3[3 * m + 1], (double)G3[3 * m + 2]};
		if (opt.metric == pcl_icp::POINT2PLANE)
		{
			const double nv[3] = {(double)N3[3 * m], (double)N3[3 * m + 1], (double)N3[3 * m + 2]};
			pcl_icp::plane_term(s, g, nv, acc);
		}
		else
		{
#pragma unroll
			for (int a = 0; a < 3; a++)
				acc[pcl_icp::SUM_S + a] += s[a], acc[pcl_icp::SUM_T + a] += g[a];
		}
		acc[pcl_icp::SUM_D2] += (double)d2[i];
		hits++;
	}
	double *partial = at<double>(arena, D.o_partial);
#pragma unroll
	for (int k = 0; k < pcl_icp::N_SUMS; k++)
		partial[(uint32_t)k * MULLS_NDT_TREE + lane] = acc[k];
	at<uint32_t>(arena, D.o_hits)[lane] = hits;
}

// Point2Point's second pass.  Every workgroup takes the tree over the six sums itself (the same text as k_pcl_icp_decide's, so the same centroids),
// then its lanes add the products of the demeaned pairs.
__global__ void __launch_bounds__(256) k_pcl_icp_cross(const PclIcpDesc *__restrict__ desc, unsigned char *arena, const PclIcpRec *__restrict__ rec,
													   const RegHead *__restrict__ head)
{
	__shared__ double s_p[256];
	__shared__ double s_c[6];
	__shared__ uint32_t s_hits[256];
	const uint32_t p = blockIdx.y, t = threadIdx.x;
	const RegHead &H = head[p];
	if (!rec[p].S.running || H.range)
		return;
	const PclIcpDesc &D = desc[p];
	double *partial = at<double>(arena, D.o_partial);
	tree_of_sums(partial, 6, [](int) { return true; }, s_p, s_c);
	const double dn = (double)hits_of(at<const uint32_t>(arena, D.o_hits), s_hits);
	double c[6];
	for (int k = 0; k < 6; k++)
		c[k] = s_c[k] / dn;
	const uint32_t ns = H.n[0] < D.n_src_cap ? H.n[0] : D.n_src_cap, nt = H.n[1] < D.n_tgt_cap ? H.n[1] : D.n_tgt_cap;
	const float *M3 = at<const float>(arena, D.o_mov), *G3 = at<const float>(arena, D.o_tgt);
	const int32_t *match = at<const int32_t>(arena, D.o_match);
	const uint32_t lane = blockIdx.x * 256u + t;
	double acc[9];
#pragma unroll
	for (int k = 0; k < 9; k++)
		acc[k] = 0.0;
	for (uint32_t i = lane; i < ns; i += MULLS_NDT_TREE)
	{
		const int32_t m = match[i];
		if (m < 0 || (uint32_t)m >= nt)
			continue;
		const double sd[3] = {(double)M3[3 * i] - c[0], (double)M3[3 * i + 1] - c[1], (double)M3[3 * i + 2] - c[2]};
		const double gd[3] = {(double)G3[3 * m] - c[3], (double)G3[3 * m + 1] - c[4], (double)G3[3 * m + 2] - c[5]};
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int b = 0; b < 3; b++)
				acc[3 * a + b] += sd[a] * gd[b];
	}
#pragma unroll
	for (int k = 0; k < 9; k++)
		partial[(uint32_t)(pcl_icp::SUM_H + k) * MULLS_NDT_TREE + lane] = acc[k];
}

// one workgroup per problem: the tree over the sums, pcl_icp_math.h's advance on one lane, then the stored source moved by the step
__global__ void __launch_bounds__(256) k_pcl_icp_decide(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec, RegHead *head,
														double *frames, uint32_t *running, uint32_t *next)
{
	__shared__ double s_p[256];
	__shared__ double s_sum[pcl_icp::N_SUMS];
	__shared__ double s_step[12];
	__shared__ uint32_t s_hits[256];
	__shared__ int s_run, s_moved;
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	if (p == 0 && t == 0)
		*next = 0u; // (the next tick's count starts from 0)
	if (t == 0)
	{
		s_run = rec[p].S.running;
		if (s_run && head[p].range)
			rec[p].S.running = 0, head[p].running = 0, s_run = 0; // refused by the host
	}
	__syncthreads();
	if (!s_run)
		return;
	const PclIcpDesc &D = desc[p];
	// (Point2Point has no sums between the cross-covariance and the squared distances)
	tree_of_sums(at<const double>(arena, D.o_partial), pcl_icp::N_SUMS,
				 [&](int k) { return !(opt.metric == pcl_icp::POINT2POINT && k >= pcl_icp::SUM_H + 9 && k != pcl_icp::SUM_D2); }, s_p, s_sum);
	const uint32_t n_corr = hits_of(at<const uint32_t>(arena, D.o_hits), s_hits);
	if (t == 0)
	{
		PclIcpRec &R = rec[p];
		pcl_icp::State S = R.S;
		pcl_icp::advance(S, opt.metric, s_sum, n_corr, opt.max_iter_num, opt.transformation_epsilon, opt.euclidean_fitness_epsilon);
		R.S = S;
		head[p].running = S.running;
		for (int k = 0; k < 9; k++)
			frames[12u * p + k] = S.R[k], s_step[k] = S.Rs[k];
		for (int k = 0; k < 3; k++)
			frames[12u * p + 9 + k] = S.t[k], s_step[9 + k] = S.ts[k];
		s_moved = S.moved && S.running; // (a stopped problem's moved source is read by nobody)
		if (S.running)
			atomicAdd(running, 1u);
	}
	__syncthreads();
	if (!s_moved)
		return;
	const uint32_t ns = head[p].n[0] < D.n_src_cap ? head[p].n[0] : D.n_src_cap;
	float *M3 = at<float>(arena, D.o_mov);
	for (uint32_t i = t; i < ns; i += 256u)
		pcl_icp::move_stored(s_step, s_step + 9, M3 + 3 * i);
}

// the fitness: over the source points whose nearest squared distance is within the range, the mean; the strided partials and the tree as every sum here
__global__ void __launch_bounds__(256) k_pcl_icp_fitness(const PclIcpDesc *__restrict__ desc, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec,
														 const RegHead *__restrict__ head)
{
	__shared__ double s_p[256];
	__shared__ uint32_t s_hits[256];
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	PclIcpRec &R = rec[p];
	if (head[p].status != PCL_ICP_ST_OK)
		return;
	const PclIcpDesc &D = desc[p];
	const uint32_t ns = head[p].n[0] < D.n_src_cap ? head[p].n[0] : D.n_src_cap;
	const float *dist = at<const float>(arena, D.o_dist);
	double r[16];
	uint32_t h = 0;
#pragma unroll
	for (int m = 0; m < 16; m++)
	{
		double a = 0.0;
		for (uint32_t i = t + 256u * m; i < ns; i += MULLS_NDT_TREE)
			if ((double)dist[i] <= opt.fit_range)
				a += (double)dist[i], h++;
		r[m] = a;
	}
	const double sum = tree_of_partials(r, s_p);
	const uint32_t n_fit = sum_of_counts(h, s_hits);
	if (t == 0)
	{
		R.n_fit = n_fit;
		R.fitness = n_fit ? sum / (double)n_fit : DBL_MAX;
	}
}
} // namespace

hipError_t launch_pcl_icp_begin(hipStream_t st, const PclIcpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t n_src_max, unsigned char *arena, const NdtRec *nrec,
								PclIcpRec *rec, RegHead *head, double *frames)
{
	hipLaunchKernelGGL(k_pcl_icp_begin, dim3(blocks_of(P, 64)), dim3(64), 0, st, nrec, rec, head, frames, P);
	hipLaunchKernelGGL(k_pcl_icp_copy, dim3(blocks_of(n_src_max, 256), P), dim3(256), 0, st, desc, tabs, arena, head);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_normals(hipStream_t st, const PclIcpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t slots_max, unsigned char *arena, PclIcpOpts opt,
								  const RegHead *head)
{
	hipLaunchKernelGGL(k_pcl_icp_sort, dim3(blocks_of(slots_max, 256), P), dim3(256), 0, st, tabs, arena, head);
	hipLaunchKernelGGL(k_pcl_icp_normals, dim3(slots_max, P), dim3(256), 0, st, desc, tabs, arena, opt, head);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_search(hipStream_t st, const PclIcpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t n_src_max, unsigned char *arena, PclIcpOpts opt,
								 const PclIcpRec *rec, const RegHead *head)
{
	const dim3 grid(blocks_of(n_src_max, 256), P), block(256);
	hipLaunchKernelGGL(k_pcl_icp_search, grid, block, 0, st, desc, tabs, arena, opt, rec, head);
	if (opt.reciprocal)
		hipLaunchKernelGGL(k_pcl_icp_recip, grid, block, 0, st, desc, tabs, arena, rec, head);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_accum(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, const PclIcpRec *rec, const RegHead *head)
{
	const dim3 grid(MULLS_NDT_TREE / 256u, P), block(256);
	hipLaunchKernelGGL(k_pcl_icp_accum, grid, block, 0, st, desc, arena, opt, rec, head);
	if (opt.metric == pcl_icp::POINT2POINT)
		hipLaunchKernelGGL(k_pcl_icp_cross, grid, block, 0, st, desc, arena, rec, head);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_decide(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec, RegHead *head,
								 double *frames, uint32_t *running, uint32_t *next)
{
	hipLaunchKernelGGL(k_pcl_icp_decide, dim3(P), dim3(256), 0, st, desc, arena, opt, rec, head, frames, running, next);
	return hipGetLastError();
}
hipError_t launch_pcl_icp_fitness(hipStream_t st, const PclIcpDesc *desc, uint32_t P, unsigned char *arena, PclIcpOpts opt, PclIcpRec *rec, const RegHead *head)
{
	hipLaunchKernelGGL(k_pcl_icp_fitness, dim3(P), dim3(256), 0, st, desc, arena, opt, rec, head);
	return hipGetLastError();
}
