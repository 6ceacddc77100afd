// k_gicp.hip — the device side of mulls_gicp / mulls_gicp_batch (gfx950).  One launch of each kernel serves every problem of a sub-batch: blockIdx.y is the
// problem's table or cloud for the per-point and per-slot kernels, blockIdx.x the problem for those that give a problem one workgroup.  The crop and the
// fitness pass are k_ndt.hip's.  Setup: three tables of occupied cells per problem (k_reg_table.hip, reg_table.h), the exact
// k-nearest ring walk with the (d2, index) list in registers and the covariance tail (k_gicp_knn, the setup's hot path), a wave per query the walk did
// not certify (k_gicp_brute), one lane per voxel that sorts its points' indices and adds in that order (k_gicp_voxels) — atomics place entries, they never
// decide an order of additions.  Iteration: k_gicp_eval (the loop's hot path: 28 double sums per source point, strided partials) and k_gicp_decide (the
// tree, then the Cholesky step and the update of gicp_math.h on one lane) once per tick; a problem that has stopped returns at once.  No kernel waits
// for another workgroup.  Every loop is bounded by a descriptor field, a launch argument or a constant.
#include <hip/hip_runtime.h>

#include "gicp_launch.h"
#include "reg_device.h"
#include "sor_math.h"

namespace
{
// The k smallest (d2, index) pairs seen so far, ascending in slots CAP - k .. CAP - 1; the slots in front of them hold -inf, which no value passes, so
// one text serves every k <= CAP with static indices only: the list stays in registers.
template <int CAP>
struct KBest
{
	float d[CAP];
	uint32_t id[CAP];
	__device__ __forceinline__ void init(int k)
	{
#pragma unroll
		for (int j = 0; j < CAP; j++)
			d[j] = j < CAP - k ? -INFINITY : INFINITY, id[j] = j < CAP - k ? 0u : 0xffffffffu;
	}
	__device__ __forceinline__ float worst() const { return d[CAP - 1]; }
	__device__ __forceinline__ void insert(float v, uint32_t i)
	{
		if (!(v < d[CAP - 1] || (v == d[CAP - 1] && i < id[CAP - 1])))
			return;
		d[CAP - 1] = v, id[CAP - 1] = i;
#pragma unroll
		for (int j = CAP - 1; j > 0; j--)
		{
			const bool sw = d[j] < d[j - 1] || (d[j] == d[j - 1] && id[j] < id[j - 1]);
			const float a = d[j - 1], b = d[j];
			const uint32_t ia = id[j - 1], ib = id[j];
			d[j - 1] = sw ? b : a, d[j] = sw ? a : b;
			id[j - 1] = sw ? ib : ia, id[j] = sw ? ia : ib;
		}
	}
};

__global__ void __launch_bounds__(64) k_gicp_begin(const NdtRec *__restrict__ nrec, GicpRec *rec, RegHead *head, double *frames, GicpOpts opt, uint32_t P)
{
	const uint32_t p = blockIdx.x * 64u + threadIdx.x;
	if (p >= P)
		return;
	GicpRec &R = rec[p];
	RegHead H{};
	H.n[0] = nrec[p].n_src, H.n[1] = nrec[p].n_tgt;
	R.n_left[0] = R.n_left[1] = 0;
	int status = GICP_ST_OK;
	if (nrec[p].status == NDT_ST_NONFINITE)
		status = GICP_ST_NONFINITE;
	else if (nrec[p].status != NDT_ST_OK || H.n[0] < (uint32_t)opt.k || H.n[1] < (uint32_t)opt.k)
		status = GICP_ST_FEW;
	H.status = status;
	gicp::State S;
	gicp::begin(S, opt.start_rotvec);
	if (status != GICP_ST_OK)
		S.running = 0;
	R.S = S;
	H.running = S.running;
	head[p] = H;
	for (int k = 0; k < 9; k++)
		frames[12u * p + k] = S.R[k];
	for (int k = 0; k < 3; k++)
		frames[12u * p + 9 + k] = S.t[k];
}

// the tail of a neighbour query: the mean and the scatter of the k neighbours in the list's order, the PLANE covariance
template <int CAP>
__device__ __forceinline__ void covariance_tail(const KBest<CAP> &kb, int k, const float *__restrict__ P3, uint32_t n, double *out)
{
	double s[3] = {0.0, 0.0, 0.0}, m[3], S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
	for (int j = 0; j < CAP; j++)
		if (j >= CAP - k)
		{
			const uint32_t i = kb.id[j] < n ? kb.id[j] : 0u;
			gicp::sum_add(s, (double)P3[3 * i], (double)P3[3 * i + 1], (double)P3[3 * i + 2]);
		}
	gicp::mean_of(s, k, m);
#pragma unroll
	for (int j = 0; j < CAP; j++)
		if (j >= CAP - k)
		{
			const uint32_t i = kb.id[j] < n ? kb.id[j] : 0u;
			gicp::scatter_add(S, m, (double)P3[3 * i], (double)P3[3 * i + 1], (double)P3[3 * i + 2]);
		}
	double C[6];
	gicp::plane_covariance(S, C);
#pragma unroll
	for (int a = 0; a < 6; a++)
		out[a] = C[a];
}

// The setup's hot path.  One lane per point of a cloud, in cell order: Chebyshev rings around its cell until its k-th best is certainly nearer than
// anything unscanned (sor_certified), then the tail.  A query no ring certifies is left for k_gicp_brute.
template <int CAP>
__global__ void __launch_bounds__(256) k_gicp_knn(const GicpDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena, GicpOpts opt,
												  GicpRec *rec, const RegHead *__restrict__ head, uint32_t *max_left)
{
	const uint32_t p = blockIdx.y >> 1, c = blockIdx.y & 1u;
	GicpRec &R = rec[p];
	const RegHead &H = head[p];
	if (H.status != GICP_ST_OK || H.range)
		return;
	const RegTab T = tabs[MULLS_REG_TABS * p + c];
	const uint32_t n = H.n[c] < T.n_cap ? H.n[c] : T.n_cap;
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t >= n)
		return;
	const uint32_t *list = at<const uint32_t>(arena, T.o_list);
	const uint32_t qi = list[t] < n ? list[t] : 0u;
	const float *P3 = at<const float>(arena, T.o_pts);
	const float qx = P3[3 * qi], qy = P3[3 * qi + 1], qz = P3[3 * qi + 2];
	int ok = 1;
	// (the cell in double, so that the assignment's rounding is far below the certificate's margin, sor_math.h)
	const int32_t cx = pcl_icp::cell_coord(qx, T.inv_edge, &ok), cy = pcl_icp::cell_coord(qy, T.inv_edge, &ok), cz = pcl_icp::cell_coord(qz, T.inv_edge, &ok);
	const uint64_t *keys = at<const uint64_t>(arena, T.o_keys);
	const uint32_t *start = at<const uint32_t>(arena, T.o_start), *count = at<const uint32_t>(arena, T.o_count);
	KBest<CAP> kb;
	kb.init(opt.k);
	bool done = false;
	for (int ring = 0; ring <= MULLS_GICP_MAX_RING && !done; ring++)
	{
		for (int dz = -ring; dz <= ring; dz++)
			for (int dy = -ring; dy <= ring; dy++)
			{
				const bool face = dz == -ring || dz == ring || dy == -ring || dy == ring;
				const int stepx = face ? 1 : 2 * ring; // off the shell's faces only dx = -ring and dx = ring belong to the ring
				for (int dx = -ring; dx <= ring; dx += stepx)
				{
					const int32_t nx = cx + dx, ny = cy + dy, nz = cz + dz;
					if (!cell_in_range(nx, ny, nz))
						continue;
					const uint32_t slot = find_slot(keys, gicp::pack_coords(nx, ny, nz), T.slots, T.shift);
					if (slot == NO_SLOT)
						continue;
					const uint32_t b = start[slot], cnt = count[slot];
					if (b >= n || cnt > n - b)
						continue;
					for (uint32_t j = b; j < b + cnt; j++)
					{
						const uint32_t i = list[j] < n ? list[j] : 0u;
						kb.insert(sor_d2(P3[3 * i], P3[3 * i + 1], P3[3 * i + 2], qx, qy, qz), i);
					}
				}
			}
		done = ring >= 1 && sor_certified(kb.worst(), ring, opt.knn_edge);
	}
	if (done)
		covariance_tail<CAP>(kb, opt.k, P3, n, at<double>(arena, desc[p].o_cov[c]) + 6ull * qi);
	else
	{
		const uint32_t pos = atomicAdd(&R.n_left[c], 1u);
		if (pos < T.n_cap)
			at<uint32_t>(arena, desc[p].o_left[c])[pos] = qi;
		atomicMax(max_left, pos + 1u);
	}
}

// One wavefront per query the walk left.  Every lane keeps the k best of the points lane, lane + 64, ..; then k rounds, each taking the smallest pair
// above the one taken before over all the lanes' lists: the neighbours in (d2, index) order.  Lane 0 runs the tail.
template <int CAP>
__global__ void __launch_bounds__(64) k_gicp_brute(const GicpDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena, GicpOpts opt,
												   const GicpRec *__restrict__ rec, const RegHead *__restrict__ head)
{
	__shared__ uint32_t s_idx[CAP];
	const uint32_t p = blockIdx.y >> 1, c = blockIdx.y & 1u, lane = threadIdx.x;
	const GicpRec &R = rec[p];
	const RegHead &H = head[p];
	if (H.status != GICP_ST_OK || H.range)
		return;
	const RegTab T = tabs[MULLS_REG_TABS * p + c];
	const uint32_t n = H.n[c] < T.n_cap ? H.n[c] : T.n_cap;
	const uint32_t n_left = R.n_left[c] < T.n_cap ? R.n_left[c] : T.n_cap;
	if (blockIdx.x >= n_left)
		return;
	const uint32_t q = at<const uint32_t>(arena, desc[p].o_left[c])[blockIdx.x];
	const uint32_t qi = q < n ? q : 0u;
	const float *P3 = at<const float>(arena, T.o_pts);
	const float qx = P3[3 * qi], qy = P3[3 * qi + 1], qz = P3[3 * qi + 2];
	KBest<CAP> kb;
	kb.init(opt.k);
	for (uint32_t i = lane; i < n; i += 64u)
		kb.insert(sor_d2(P3[3 * i], P3[3 * i + 1], P3[3 * i + 2], qx, qy, qz), i);
	float pd = -INFINITY;
	uint32_t pi = 0;
	bool first = true;
	for (int round = 0; round < opt.k && round < CAP; round++)
	{
		float bd = INFINITY;
		uint32_t bi = 0xffffffffu;
#pragma unroll
		for (int j = 0; j < CAP; j++)
		{
			const float v = kb.d[j];
			const uint32_t i = kb.id[j];
			const bool above = v != -INFINITY && (first || v > pd || (v == pd && i > pi));
			const bool less = v < bd || (v == bd && i < bi);
			if (above && less)
				bd = v, bi = i;
		}
#pragma unroll
		for (int s = 32; s > 0; s >>= 1)
		{
			const float od = __shfl_xor(bd, s, 64);
			const uint32_t oi = __shfl_xor(bi, s, 64);
			if (od < bd || (od == bd && oi < bi))
				bd = od, bi = oi;
		}
		pd = bd, pi = bi, first = false;
		if (lane == 0)
			s_idx[round] = bi;
	}
	__syncthreads();
	if (lane != 0)
		return;
	const int k = opt.k < CAP ? opt.k : CAP;
	double s[3] = {0.0, 0.0, 0.0}, m[3], S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	for (int j = 0; j < k; j++)
	{
		const uint32_t i = s_idx[j] < n ? s_idx[j] : 0u;
		gicp::sum_add(s, (double)P3[3 * i], (double)P3[3 * i + 1], (double)P3[3 * i + 2]);
	}
	gicp::mean_of(s, k, m);
	for (int j = 0; j < k; j++)
	{
		const uint32_t i = s_idx[j] < n ? s_idx[j] : 0u;
		gicp::scatter_add(S, m, (double)P3[3 * i], (double)P3[3 * i + 1], (double)P3[3 * i + 2]);
	}
	double C[6];
	gicp::plane_covariance(S, C);
	double *out = at<double>(arena, desc[p].o_cov[c]) + 6ull * qi;
	for (int a = 0; a < 6; a++)
		out[a] = C[a];
}

// one lane per occupied slot of the voxel map: its points' indices ascending, the sums in that order, the voxel
__global__ void __launch_bounds__(256) k_gicp_voxels(const GicpDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena,
													 const RegHead *__restrict__ head)
{
	const uint32_t p = blockIdx.y;
	const RegHead &H = head[p];
	if (H.status != GICP_ST_OK || H.range)
		return;
	const RegTab T = tabs[MULLS_REG_TABS * p + GICP_TAB_VOXEL];
	const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
	if (slot >= T.slots)
		return;
	const uint32_t n = at<const uint32_t>(arena, T.o_count)[slot];
	if (!n)
		return;
	const uint32_t first = at<const uint32_t>(arena, T.o_start)[slot];
	if (first >= T.n_cap || n > T.n_cap - first)
		return;
	uint32_t *L = at<uint32_t>(arena, T.o_list) + first;
	sort_list(L, n);
	const float *P3 = at<const float>(arena, T.o_pts);
	const double *cov = at<const double>(arena, desc[p].o_cov[1]);
	double s[3] = {0.0, 0.0, 0.0}, q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	for (uint32_t k = 0; k < n; k++)
	{
		const uint32_t i = L[k] < T.n_cap ? L[k] : 0u;
		s[0] += (double)P3[3 * i], s[1] += (double)P3[3 * i + 1], s[2] += (double)P3[3 * i + 2];
#pragma unroll
		for (int a = 0; a < 6; a++)
			q[a] += cov[6ull * i + a];
	}
	double *V = at<double>(arena, desc[p].o_vox) + 9ull * first;
	const double dn = (double)n;
	V[0] = s[0] / dn, V[1] = s[1] / dn, V[2] = s[2] / dn;
#pragma unroll
	for (int a = 0; a < 6; a++)
		V[3 + a] = q[a] / dn;
}

// The loop's hot path.  Lane l of the problem's MULLS_NDT_TREE lanes takes the source points l, l + MULLS_NDT_TREE, ..: the point under (R, t) in double,
// the voxel of its float rounding, the 3 x 3 algebra of gicp_math.h into the lane's 28 sums.  The frame's 12 doubles are read from LDS.
__global__ void __launch_bounds__(256) k_gicp_eval(const GicpDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena, GicpOpts opt,
												   const GicpRec *__restrict__ rec, const RegHead *__restrict__ head)
{
	__shared__ double s_F[12];
	const uint32_t p = blockIdx.y;
	const GicpRec &R = rec[p];
	if (!R.S.running)
		return;
	if (threadIdx.x < 9)
		s_F[threadIdx.x] = R.S.R[threadIdx.x];
	else if (threadIdx.x < 12)
		s_F[threadIdx.x] = R.S.t[threadIdx.x - 9];
	__syncthreads();
	const GicpDesc &D = desc[p];
	const RegTab T = tabs[MULLS_REG_TABS * p + GICP_TAB_VOXEL];
	const RegTab &TS = tabs[MULLS_REG_TABS * p + GICP_TAB_KNN_SRC];
	const uint32_t n = head[p].n[0] < TS.n_cap ? head[p].n[0] : TS.n_cap;
	const float *S3 = at<const float>(arena, TS.o_pts);
	const double *cov = at<const double>(arena, D.o_cov[0]);
	const uint64_t *keys = at<const uint64_t>(arena, T.o_keys);
	const uint32_t *start = at<const uint32_t>(arena, T.o_start);
	const double *vox = at<const double>(arena, D.o_vox);
	const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
	double acc[28];
#pragma unroll
	for (int k = 0; k < 28; k++)
		acc[k] = 0.0;
	uint32_t hits = 0;
	for (uint32_t i = lane; i < n; i += MULLS_NDT_TREE)
	{
		double ap[3];
		gicp::move_point(s_F, s_F + 9, S3[3 * i], S3[3 * i + 1], S3[3 * i + 2], ap);
		int ok = 1;
		const int32_t c0 = gicp::voxel_coord((float)ap[0], opt.resolution, &ok), c1 = gicp::voxel_coord((float)ap[1], opt.resolution, &ok),
					  c2 = gicp::voxel_coord((float)ap[2], opt.resolution, &ok);
		if (!ok)
			continue;
		const uint32_t slot = find_slot(keys, gicp::pack_coords(c0, c1, c2), T.slots, T.shift);
		if (slot == NO_SLOT)
			continue;
		const uint32_t vi = start[slot];
		if (vi >= T.n_cap)
			continue;
		double CA[6], V[9];
#pragma unroll
		for (int a = 0; a < 6; a++)
			CA[a] = cov[6ull * i + a];
#pragma unroll
		for (int a = 0; a < 9; a++)
			V[a] = vox[9ull * vi + a];
		double a28[28];
#pragma unroll
		for (int k = 0; k < 28; k++)
			a28[k] = 0.0;
		gicp::point_term(ap, CA, V, V + 3, s_F, a28);
#pragma unroll
		for (int k = 0; k < 28; k++)
			acc[k] += a28[k];
		hits++;
	}
	double *partial = at<double>(arena, D.o_partial);
#pragma unroll
	for (int k = 0; k < 28; k++)
		partial[(uint32_t)k * MULLS_NDT_TREE + lane] = acc[k];
	at<uint32_t>(arena, D.o_hits)[lane] = hits;
}

__global__ void __launch_bounds__(256) k_gicp_decide(const GicpDesc *__restrict__ desc, unsigned char *arena, GicpOpts opt, GicpRec *rec, RegHead *head,
													 double *frames, uint32_t *running, uint32_t *next)
{
	__shared__ double s_p[256];
	__shared__ double s_sum[28];
	__shared__ uint32_t s_hits[256];
	__shared__ int s_run;
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	if (p == 0 && t == 0)
		*next = 0u; // (the next tick's count starts from 0)
	if (t == 0)
		s_run = rec[p].S.running;
	__syncthreads();
	if (!s_run)
		return;
	const GicpDesc &D = desc[p];
	tree_of_sums(at<const double>(arena, D.o_partial), 28, [](int) { return true; }, s_p, s_sum);
	const uint32_t n_corr = hits_of(at<const uint32_t>(arena, D.o_hits), s_hits);
	if (t != 0)
		return;
	GicpRec &R = rec[p];
	gicp::State S = R.S;
	gicp::advance(S, s_sum, n_corr, opt.max_iterations, opt.rotation_epsilon, opt.transformation_epsilon);
	R.S = S;
	head[p].running = S.running;
	for (int k = 0; k < 9; k++)
		frames[12u * p + k] = S.R[k];
	for (int k = 0; k < 3; k++)
		frames[12u * p + 9 + k] = S.t[k];
	if (S.running)
		atomicAdd(running, 1u);
}
} // namespace

hipError_t launch_gicp_begin(hipStream_t st, uint32_t P, const NdtRec *nrec, GicpRec *rec, RegHead *head, double *frames, GicpOpts opt)
{
	hipLaunchKernelGGL(k_gicp_begin, dim3(blocks_of(P, 64)), dim3(64), 0, st, nrec, rec, head, frames, opt, P);
	return hipGetLastError();
}
hipError_t launch_gicp_knn(hipStream_t st, const GicpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t n_max, unsigned char *arena, GicpOpts opt, GicpRec *rec,
						   const RegHead *head, uint32_t *max_left)
{
	const dim3 grid(blocks_of(n_max, 256), 2u * P), block(256);
	if (opt.k <= 8)
		hipLaunchKernelGGL(k_gicp_knn<8>, grid, block, 0, st, desc, tabs, arena, opt, rec, head, max_left);
	else if (opt.k <= 20)
		hipLaunchKernelGGL(k_gicp_knn<20>, grid, block, 0, st, desc, tabs, arena, opt, rec, head, max_left);
	else
		hipLaunchKernelGGL(k_gicp_knn<32>, grid, block, 0, st, desc, tabs, arena, opt, rec, head, max_left);
	return hipGetLastError();
}
hipError_t launch_gicp_brute(hipStream_t st, const GicpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t max_left, unsigned char *arena, GicpOpts opt,
							 const GicpRec *rec, const RegHead *head)
{
	if (!max_left)
		return hipSuccess;
	const dim3 grid(max_left, 2u * P), block(64);
	if (opt.k <= 8)
		hipLaunchKernelGGL(k_gicp_brute<8>, grid, block, 0, st, desc, tabs, arena, opt, rec, head);
	else if (opt.k <= 20)
		hipLaunchKernelGGL(k_gicp_brute<20>, grid, block, 0, st, desc, tabs, arena, opt, rec, head);
	else
		hipLaunchKernelGGL(k_gicp_brute<32>, grid, block, 0, st, desc, tabs, arena, opt, rec, head);
	return hipGetLastError();
}
hipError_t launch_gicp_voxels(hipStream_t st, const GicpDesc *desc, const RegTab *tabs, uint32_t P, uint32_t slots_max, unsigned char *arena, const RegHead *head)
{
	hipLaunchKernelGGL(k_gicp_voxels, dim3(blocks_of(slots_max, 256), P), dim3(256), 0, st, desc, tabs, arena, head);
	return hipGetLastError();
}
hipError_t launch_gicp_eval(hipStream_t st, const GicpDesc *desc, const RegTab *tabs, uint32_t P, unsigned char *arena, GicpOpts opt, const GicpRec *rec,
							const RegHead *head)
{
	hipLaunchKernelGGL(k_gicp_eval, dim3(MULLS_NDT_TREE / 256u, P), dim3(256), 0, st, desc, tabs, arena, opt, rec, head);
	return hipGetLastError();
}
hipError_t launch_gicp_decide(hipStream_t st, const GicpDesc *desc, uint32_t P, unsigned char *arena, GicpOpts opt, GicpRec *rec, RegHead *head, double *frames,
							  uint32_t *running, uint32_t *next)
{
	hipLaunchKernelGGL(k_gicp_decide, dim3(P), dim3(256), 0, st, desc, arena, opt, rec, head, frames, running, next);
	return hipGetLastError();
}
