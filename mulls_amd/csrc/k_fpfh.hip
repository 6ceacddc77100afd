// k_fpfh.hip — the device side of mulls_fpfh and mulls_coarse_reg_fpfhsac (gfx950).  The descriptor: blockIdx.y is the cloud, so the source's and the
// target's descriptors come from one launch set.  The cell tables are k_reg_table.hip's (edge r (1 + 2^-20), r the feature radius); k_fpfh_sort puts
// every cell's list in ascending index and k_fpfh_gather copies coordinates and normals into that order.  k_fpfh_spfh: a wave per query point, its lanes
// stride over the candidates of the 27 cells, the pair features count into 33 integer LDS counters of the wave.  k_fpfh_hist: a wave per point again;
// a lane per bin holds a double sum; the neighbours are found 64 at a time and added in the fixed order: the 27 cells with x fastest, ascending index
// inside a cell.  SAC-IA: k_fpfh_similar (a wave per sample, its list of the k nearest target descriptors sorted across the lanes' registers),
// k_fpfh_models (ransac_math.h's three-pair fit), mulls_ndt's nearest-target pass for a chunk of hypotheses, k_fpfh_errors (strided partials and the
// tree), k_fpfh_pick.  Atomics count in LDS or set a flag; they never decide an order of additions.  No kernel waits for another workgroup.  Every loop
// is bounded by a descriptor field, a launch argument or a constant.
#include <hip/hip_runtime.h>

#include "fpfh_device.h"
#include "fpfh_launch.h"
#include "ransac_math.h"
#include "reg_device.h"

namespace
{
constexpr uint32_t NO_POINT = 0xffffffffu;
constexpr uint32_t WAVES = 4; // of a 256-thread workgroup: query points (or samples) of one workgroup

__global__ void __launch_bounds__(256) k_fpfh_check(const FpfhDesc *__restrict__ desc, const unsigned char *arena, RegHead *head)
{
	const uint32_t c = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
	const FpfhDesc &D = desc[c];
	if (i >= D.n)
		return;
	const float *P3 = reinterpret_cast<const float *>(arena + D.o_pts), *N3 = reinterpret_cast<const float *>(arena + D.o_nrm);
	float s = 0.f;
	for (int k = 0; k < 3; k++)
		s += (P3[3 * i + k] - P3[3 * i + k]) + (N3[3 * i + k] - N3[3 * i + k]); // 0 when all six are finite, else NaN
	if (!(s == 0.f))
		atomicOr(&head[c].range, MULLS_FPFH_NONFINITE);
}

// one lane per occupied slot: its points' indices ascending; a cell of more than MULLS_FPFH_MAX_CELL_POINTS refuses the cloud instead
__global__ void __launch_bounds__(256) k_fpfh_sort(const RegTab *__restrict__ tabs, unsigned char *arena, RegHead *head)
{
	const uint32_t c = blockIdx.y;
	RegHead &H = head[c];
	const RegTab T = tabs[MULLS_REG_TABS * c];
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
	if (n > MULLS_FPFH_MAX_CELL_POINTS)
	{
		atomicOr(&H.range, MULLS_FPFH_CELL_FULL); // (the kernels after this one see the flag and do nothing)
		return;
	}
	sort_list(at<uint32_t>(arena, T.o_list) + first, n);
}

// the coordinates and normals in the order of the sorted lists
__global__ void __launch_bounds__(256) k_fpfh_gather(const FpfhDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena,
													 const RegHead *__restrict__ head)
{
	const uint32_t c = blockIdx.y;
	const RegHead &H = head[c];
	const RegTab T = tabs[MULLS_REG_TABS * c];
	if (!table_live(H, T) || H.range)
		return;
	const FpfhDesc &D = desc[c];
	const uint32_t n = points_of(H, T), pos = blockIdx.x * 256u + threadIdx.x;
	if (pos >= n)
		return;
	const uint32_t j = at<const uint32_t>(arena, T.o_list)[pos];
	if (j >= n)
		return;
	const float *P3 = at<const float>(arena, D.o_pts), *N3 = at<const float>(arena, D.o_nrm);
	float *Q3 = at<float>(arena, D.o_cpts), *M3 = at<float>(arena, D.o_cnrm);
	for (int k = 0; k < 3; k++)
		Q3[3 * pos + k] = P3[3 * j + k], M3[3 * pos + k] = N3[3 * j + k];
}

// lanes 0 .. 26 of a wave: the list ranges of the 27 cells around point i's own (x fastest), empty where a cell is not occupied
__device__ __forceinline__ void cell_ranges(const RegTab &T, const unsigned char *arena, const float *p, bool have, uint32_t n, uint32_t lane, uint32_t *s_b, uint32_t *s_e)
{
	if (lane >= 27u)
		return;
	uint32_t b = 0, e = 0;
	int ok = 1;
	const int32_t cx = pcl_icp::cell_coord(p[0], T.inv_edge, &ok), cy = pcl_icp::cell_coord(p[1], T.inv_edge, &ok), cz = pcl_icp::cell_coord(p[2], T.inv_edge, &ok);
	if (have && ok)
	{
		const uint32_t *start = reinterpret_cast<const uint32_t *>(arena + T.o_start), *count = reinterpret_cast<const uint32_t *>(arena + T.o_count);
		visit_cells(reinterpret_cast<const uint64_t *>(arena + T.o_keys), T.slots, T.shift, cx, cy, cz, (int)lane, (int)lane + 1, [&](int, uint32_t s) {
			if (start[s] < n && count[s] <= n - start[s])
				b = start[s], e = b + count[s];
		});
	}
	s_b[lane] = b, s_e[lane] = e;
}

// SPFH.  A wave per query point p: every point of the 27 cells within the radius counts into k; every such point but p itself gives a pair feature,
// whose three bins count into the wave's 33 LDS counters.
__global__ void __launch_bounds__(256) k_fpfh_spfh(const FpfhDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena, double r2,
												   const RegHead *__restrict__ head)
{
	__shared__ uint32_t s_cnt[WAVES][MULLS_FPFH_DIMS], s_b[WAVES][27], s_e[WAVES][27], s_k[WAVES];
	const uint32_t c = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const RegHead &H = head[c];
	const RegTab T = tabs[MULLS_REG_TABS * c];
	if (!table_live(H, T) || H.range)
		return;
	const FpfhDesc &D = desc[c];
	const uint32_t n = points_of(H, T), i = blockIdx.x * WAVES + w;
	const bool have = i < n;
	const float *P3 = at<const float>(arena, D.o_pts), *N3 = at<const float>(arena, D.o_nrm);
	const float *Q3 = at<const float>(arena, D.o_cpts), *M3 = at<const float>(arena, D.o_cnrm);
	const uint32_t *list = at<const uint32_t>(arena, T.o_list);
	const uint32_t ii = have ? i : 0u;
	const float p[3] = {P3[3 * ii], P3[3 * ii + 1], P3[3 * ii + 2]}, np[3] = {N3[3 * ii], N3[3 * ii + 1], N3[3 * ii + 2]};
	if (lane < MULLS_FPFH_DIMS)
		s_cnt[w][lane] = 0u;
	if (lane == 0u)
		s_k[w] = 0u;
	cell_ranges(T, arena, p, have, n, lane, s_b[w], s_e[w]);
	__syncthreads();
	uint32_t k = 0;
	for (int l = 0; l < 27; l++)
	{
		const uint32_t b = s_b[w][l], e = s_e[w][l];
		for (uint32_t j = b + lane; j < e; j += 64u)
		{
			const float q[3] = {Q3[3 * j], Q3[3 * j + 1], Q3[3 * j + 2]};
			if (!((double)pcl_icp::dist2(q[0], q[1], q[2], p[0], p[1], p[2]) <= r2))
				continue;
			k++;
			if (list[j] == i)
				continue;
			const float nq[3] = {M3[3 * j], M3[3 * j + 1], M3[3 * j + 2]};
			double f[3];
			int bin[3];
			if (fpfh::pair_feature(p, np, q, nq, f) && fpfh::bins_of(f, bin))
			{
				atomicAdd(&s_cnt[w][bin[0]], 1u);
				atomicAdd(&s_cnt[w][MULLS_FPFH_BINS + bin[1]], 1u);
				atomicAdd(&s_cnt[w][2 * MULLS_FPFH_BINS + bin[2]], 1u);
			}
		}
	}
	if (k)
		atomicAdd(&s_k[w], k);
	__syncthreads();
	if (!have)
		return;
	if (lane < MULLS_FPFH_DIMS)
		at<float>(arena, D.o_spfh)[(size_t)MULLS_FPFH_DIMS * i + lane] = fpfh::spfh_of_count(s_cnt[w][lane], s_k[w]);
	if (lane == 0u)
		at<uint32_t>(arena, D.o_k)[i] = s_k[w];
}

// FPFH.  A wave per point p; lane b < 33 holds the double sum of bin b.  The candidates of a cell are tested 64 at a time; those within the radius and
// not at distance 0 are then added one by one in the order of the list, every lane reading its own float of the neighbour's SPFH row.
__global__ void __launch_bounds__(256) k_fpfh_hist(const FpfhDesc *__restrict__ desc, const RegTab *__restrict__ tabs, unsigned char *arena, double r2,
												   const RegHead *__restrict__ head)
{
	__shared__ double s_acc[WAVES][MULLS_FPFH_DIMS];
	__shared__ uint32_t s_b[WAVES][27], s_e[WAVES][27];
	const uint32_t c = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const RegHead &H = head[c];
	const RegTab T = tabs[MULLS_REG_TABS * c];
	if (!table_live(H, T) || H.range)
		return;
	const FpfhDesc &D = desc[c];
	const uint32_t n = points_of(H, T), i = blockIdx.x * WAVES + w;
	const bool have = i < n;
	const float *P3 = at<const float>(arena, D.o_pts), *Q3 = at<const float>(arena, D.o_cpts), *spfh = at<const float>(arena, D.o_spfh);
	const uint32_t *list = at<const uint32_t>(arena, T.o_list);
	const uint32_t ii = have ? i : 0u;
	const float p[3] = {P3[3 * ii], P3[3 * ii + 1], P3[3 * ii + 2]};
	cell_ranges(T, arena, p, have, n, lane, s_b[w], s_e[w]);
	__syncthreads();
	double acc = 0.0;
	for (int l = 0; l < 27; l++)
	{
		const uint32_t b = s_b[w][l], e = s_e[w][l];
		for (uint32_t base = b; base < e; base += 64u)
		{
			const uint32_t j = base + lane;
			float d2 = 0.f;
			uint32_t m = NO_POINT;
			bool in = false;
			if (j < e)
			{
				d2 = pcl_icp::dist2(Q3[3 * j], Q3[3 * j + 1], Q3[3 * j + 2], p[0], p[1], p[2]);
				m = list[j];
				in = (double)d2 <= r2 && d2 != 0.f && m < n;
			}
			unsigned long long mask = __ballot(in);
			while (mask)
			{
				const int t = __ffsll((long long)mask) - 1;
				mask &= mask - 1ull;
				const float dd = __shfl(d2, t);
				const uint32_t mm = __shfl(m, t);
				if (lane < MULLS_FPFH_DIMS)
					acc += (double)spfh[(size_t)MULLS_FPFH_DIMS * mm + lane] * (1.0 / (double)dd);
			}
		}
	}
	if (lane < MULLS_FPFH_DIMS)
		s_acc[w][lane] = acc;
	__syncthreads();
	if (!have || lane >= 3u)
		return;
	float out[MULLS_FPFH_BINS];
	fpfh::normalise(&s_acc[w][MULLS_FPFH_BINS * lane], out);
	float *hist = at<float>(arena, D.o_hist) + (size_t)MULLS_FPFH_DIMS * i + MULLS_FPFH_BINS * lane;
	for (int b = 0; b < MULLS_FPFH_BINS; b++)
		hist[b] = out[b];
}

// Similar features: a wave per sample (fpfh_device.h has the text, as it has that of the four kernels below)
__global__ void __launch_bounds__(256) k_fpfh_similar(const float *__restrict__ src_hist, const float *__restrict__ tgt_hist, const int32_t *__restrict__ samples,
													  const int32_t *__restrict__ ranks, uint32_t n_samples, uint32_t n_src, uint32_t n_tgt, uint32_t k_eff, int32_t *corr)
{
	const uint32_t s = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (s >= n_samples)
		return;
	fpfh_dev::similar_wave(src_hist, tgt_hist, samples, ranks, s, n_src, n_tgt, k_eff, lane, corr);
}

__global__ void __launch_bounds__(256) k_fpfh_models(const float *__restrict__ src, const float *__restrict__ tgt, const int32_t *__restrict__ samples,
													 const int32_t *__restrict__ corr, uint32_t n_hyp, uint32_t n_src, uint32_t n_tgt, double *frames)
{
	const uint32_t h = blockIdx.x * 256u + threadIdx.x;
	if (h >= n_hyp)
		return;
	fpfh_dev::model_of(src, tgt, samples + 3 * h, corr + 3 * h, n_src, n_tgt, frames + 12u * h);
}

__global__ void __launch_bounds__(256) k_fpfh_slots(NdtDesc base, uint32_t n_src, uint32_t n_tgt, uint32_t n, NdtDesc *desc, NdtRec *rec)
{
	const uint32_t h = blockIdx.x * 256u + threadIdx.x;
	if (h >= n)
		return;
	fpfh_dev::slot_of(base, n_src, n_tgt, base.o_dist + 4ull * n_src * h, desc + h, rec + h);
}

// one workgroup per hypothesis: the error terms of its source points by the strided-partial rule
__global__ void __launch_bounds__(256) k_fpfh_errors(const NdtDesc *__restrict__ desc, uint32_t n_src, const unsigned char *arena, float thr, int huber, double *err)
{
	__shared__ double s_p[256];
	const uint32_t h = blockIdx.x;
	const double sum = fpfh_dev::error_sum(reinterpret_cast<const float *>(arena + desc[h].o_dist), n_src, thr, huber, s_p);
	if (threadIdx.x == 0)
		err[h] = sum;
}

// one workgroup: the first hypothesis by fpfh::error_before: the lowest error, the first among equals, a NaN error after every number
__global__ void __launch_bounds__(256) k_fpfh_pick(const double *__restrict__ err, const double *__restrict__ frames, uint32_t n_hyp, FpfhSacOut *out)
{
	__shared__ double s_e[256];
	__shared__ uint32_t s_i[256];
	fpfh_dev::pick_into(err, frames, n_hyp, out, s_e, s_i);
}
} // namespace

hipError_t launch_fpfh_features(hipStream_t st, const FpfhDesc *desc, const RegTab *tabs, uint32_t C, uint32_t n_max, uint32_t slots_max, unsigned char *arena,
								double r2, RegHead *head)
{
	hipLaunchKernelGGL(k_fpfh_check, dim3(blocks_of(n_max, 256), C), dim3(256), 0, st, desc, arena, head);
	if (hipError_t e = launch_reg_tables(st, tabs, C, 0, 1, n_max, slots_max, arena, head))
		return e;
	hipLaunchKernelGGL(k_fpfh_sort, dim3(blocks_of(slots_max, 256), C), dim3(256), 0, st, tabs, arena, head);
	hipLaunchKernelGGL(k_fpfh_gather, dim3(blocks_of(n_max, 256), C), dim3(256), 0, st, desc, tabs, arena, head);
	hipLaunchKernelGGL(k_fpfh_spfh, dim3(blocks_of(n_max, WAVES), C), dim3(256), 0, st, desc, tabs, arena, r2, head);
	hipLaunchKernelGGL(k_fpfh_hist, dim3(blocks_of(n_max, WAVES), C), dim3(256), 0, st, desc, tabs, arena, r2, head);
	return hipGetLastError();
}
hipError_t launch_fpfh_similar(hipStream_t st, const float *src_hist, const float *tgt_hist, const int32_t *samples, const int32_t *ranks, uint32_t n_samples,
							   uint32_t n_src, uint32_t n_tgt, uint32_t k_eff, int32_t *corr)
{
	hipLaunchKernelGGL(k_fpfh_similar, dim3(blocks_of(n_samples, WAVES)), dim3(256), 0, st, src_hist, tgt_hist, samples, ranks, n_samples, n_src, n_tgt, k_eff, corr);
	return hipGetLastError();
}
hipError_t launch_fpfh_models(hipStream_t st, const float *src, const float *tgt, const int32_t *samples, const int32_t *corr, uint32_t n_hyp, uint32_t n_src,
							  uint32_t n_tgt, double *frames)
{
	hipLaunchKernelGGL(k_fpfh_models, dim3(blocks_of(n_hyp, 256)), dim3(256), 0, st, src, tgt, samples, corr, n_hyp, n_src, n_tgt, frames);
	return hipGetLastError();
}
hipError_t launch_fpfh_slots(hipStream_t st, NdtDesc base, uint32_t n_src, uint32_t n_tgt, uint32_t n, NdtDesc *desc, NdtRec *rec)
{
	hipLaunchKernelGGL(k_fpfh_slots, dim3(blocks_of(n, 256)), dim3(256), 0, st, base, n_src, n_tgt, n, desc, rec);
	return hipGetLastError();
}
hipError_t launch_fpfh_errors(hipStream_t st, const NdtDesc *desc, uint32_t n, uint32_t n_src, unsigned char *arena, float thr, int huber, double *err)
{
	hipLaunchKernelGGL(k_fpfh_errors, dim3(n), dim3(256), 0, st, desc, n_src, arena, thr, huber, err);
	return hipGetLastError();
}
hipError_t launch_fpfh_pick(hipStream_t st, const double *err, const double *frames, uint32_t n_hyp, FpfhSacOut *out)
{
	hipLaunchKernelGGL(k_fpfh_pick, dim3(1), dim3(256), 0, st, err, frames, n_hyp, out);
	return hipGetLastError();
}
