// k_ransac.hip — the RANSAC coarse-registration solver (CRegistration::coarse_reg_ransac, cregistration.hpp:605-661) for gfx950.
//   k_ransac_models  one lane per hypothesis: float centroids and H of its three pairs, Horn's 4 x 4 by cyclic Jacobi in double
//   k_ransac_score   one wave per four hypotheses: the lanes stride over the pairs, the models sit in scalar registers
//   k_ransac_select  the inlier mask of one model
//   k_ransac_refine  one workgroup: a round of PCL's refineModel — fit to the previous inliers, select, exact median by radix select
//   k_rb_*           the same four steps for the problems of a sub-batch of mulls_coarse_reg_ransac_batch, read from a descriptor table (ransac_batch.h):
//                    the second grid axis is the problem (refine: a job list), the arithmetic is the __device__ functions the kernels above call
// The pairs' points are staged by pair_stage.h (k_pair_gather.hip gathers device-resident clouds).
// Every float / double expression is written in the order include/mulls_hip.h and DESIGN.md section 7 define (built with -ffp-contract=off):
// tests/ransac_restated.py reproduces the bits.
#include <hip/hip_runtime.h>

#include "ransac_launch.h"
#include "ransac_math.h"

namespace
{
constexpr int WAVE = 64;
constexpr int SCORE_THREADS = 256;
constexpr int HYP_PER_WAVE = 4;
constexpr int HYP_PER_BLOCK = (SCORE_THREADS / WAVE) * HYP_PER_WAVE;
constexpr int RT = (int)MULLS_RANSAC_REFINE_THREADS;

// squared distance of T (s, 1) to (t, 1), float
__device__ __forceinline__ float resid2(const float *m, const float4 s, const float4 t)
{
	const float px = ((m[0] * s.x + m[1] * s.y) + m[2] * s.z) + m[3];
	const float py = ((m[4] * s.x + m[5] * s.y) + m[6] * s.z) + m[7];
	const float pz = ((m[8] * s.x + m[9] * s.y) + m[10] * s.z) + m[11];
	const float dx = px - t.x, dy = py - t.y, dz = pz - t.z;
	return (dx * dx + dy * dy) + dz * dz;
}

// the rigid transform of the three pairs tri[0 .. 2]
__device__ __forceinline__ RansacModel sample_model(const float4 *src, const float4 *tgt, const int32_t *tri)
{
	float s[3][3], t[3][3];
#pragma unroll
	for (int k = 0; k < 3; k++)
	{
		const int32_t i = tri[k];
		const float4 a = src[i], b = tgt[i];
		s[k][0] = a.x, s[k][1] = a.y, s[k][2] = a.z;
		t[k][0] = b.x, t[k][1] = b.y, t[k][2] = b.z;
	}
	RansacModel M;
	fit_three_pairs(s, t, M.m);
	return M;
}

__global__ void __launch_bounds__(256) k_ransac_models(const float4 *src, const float4 *tgt, const int32_t *triples, uint32_t n_hyp, RansacModel *models)
{
	const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
	if (h >= n_hyp)
		return;
	models[h] = sample_model(src, tgt, triples + 3u * h);
}

__global__ void __launch_bounds__(SCORE_THREADS) k_ransac_score(const float4 *__restrict__ src, const float4 *__restrict__ tgt, uint32_t n,
																 const RansacModel *__restrict__ models, uint32_t n_hyp, double thresh, uint32_t *__restrict__ counts)
{
	// the wave's number, made scalar: the models' loads become scalar loads and the 48 coefficients live in SGPRs
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x % WAVE;
	const uint32_t h0 = blockIdx.x * HYP_PER_BLOCK + wave * HYP_PER_WAVE;
	if (h0 >= n_hyp)
		return;
	float m[HYP_PER_WAVE][12];
#pragma unroll
	for (int j = 0; j < HYP_PER_WAVE; j++)
	{
		const uint32_t h = min(h0 + (uint32_t)j, n_hyp - 1u);
#pragma unroll
		for (int k = 0; k < 12; k++)
			m[j][k] = models[h].m[k];
	}
	uint32_t c[HYP_PER_WAVE] = {0, 0, 0, 0};
	for (uint32_t i = lane; i < n; i += WAVE)
	{
		const float4 s = src[i], t = tgt[i];
#pragma unroll
		for (int j = 0; j < HYP_PER_WAVE; j++)
			c[j] += (double)resid2(m[j], s, t) < thresh ? 1u : 0u;
	}
#pragma unroll
	for (int j = 0; j < HYP_PER_WAVE; j++)
	{
		uint32_t v = c[j];
#pragma unroll
		for (int off = WAVE / 2; off > 0; off >>= 1)
			v += __shfl_xor(v, off, WAVE);
		if (lane == 0 && h0 + (uint32_t)j < n_hyp)
			counts[h0 + j] = v;
	}
}

// pair i's entry of the inlier mask of *model, and the wave's share of their count
__device__ __forceinline__ void select_pair(const float4 *src, const float4 *tgt, uint32_t n, const RansacModel *model, double thresh, uint8_t *mask, uint32_t *count,
											 uint32_t i)
{
	float m[12];
#pragma unroll
	for (int k = 0; k < 12; k++)
		m[k] = model->m[k];
	bool in = false;
	if (i < n)
	{
		in = (double)resid2(m, src[i], tgt[i]) < thresh;
		mask[i] = in ? 1 : 0;
	}
	const unsigned long long b = __ballot(in);
	if (threadIdx.x % WAVE == 0 && b)
		atomicAdd(count, (uint32_t)__popcll(b));
}

__global__ void __launch_bounds__(256) k_ransac_select(const float4 *src, const float4 *tgt, uint32_t n, const RansacModel *model, double thresh, uint8_t *mask,
														uint32_t *count)
{
	select_pair(src, tgt, n, model, thresh, mask, count, blockIdx.x * blockDim.x + threadIdx.x);
}

// sum of v over the workgroup in the defined order: the RT per-thread values by a pairwise tree, p[t] += p[t + s] for s = RT / 2, ..., 1
__device__ double block_tree_sum(double v, double *red)
{
	const int t = threadIdx.x;
	__syncthreads(); // (red may still be read by the previous sum)
	red[t] = v;
	__syncthreads();
	for (int s = RT / 2; s > 0; s >>= 1)
	{
		if (t < s)
			red[t] = red[t] + red[t + s];
		__syncthreads();
	}
	return red[0];
}

// one round of refineModel by one workgroup of RT threads (its shared state is the block's): fit, select, radix-select median
__device__ __forceinline__ void refine_round(const float4 *src, const float4 *tgt, uint32_t n, const uint8_t *mask_prev, uint8_t *mask_new, float *d2, double thresh,
											  RansacRound *out)
{
	__shared__ double red[RT];
	__shared__ uint32_t hist[256];
	__shared__ uint32_t sh_n_prev, sh_n_new, sh_changed, sh_prefix, sh_rank;
	const uint32_t t = threadIdx.x;
	if (t == 0)
		sh_n_prev = 0, sh_n_new = 0, sh_changed = 0;
	__syncthreads();
	// centroids: thread t adds the pairs t, t + RT, ... of the previous inlier set in ascending order
	double a[6] = {0, 0, 0, 0, 0, 0};
	uint32_t cnt = 0;
	for (uint32_t i = t; i < n; i += RT)
		if (mask_prev[i])
		{
			const float4 s = src[i], g = tgt[i];
			a[0] = a[0] + (double)s.x, a[1] = a[1] + (double)s.y, a[2] = a[2] + (double)s.z;
			a[3] = a[3] + (double)g.x, a[4] = a[4] + (double)g.y, a[5] = a[5] + (double)g.z;
			cnt++;
		}
	if (cnt)
		atomicAdd(&sh_n_prev, cnt);
	double cen[6];
	for (int k = 0; k < 6; k++)
		cen[k] = block_tree_sum(a[k], red);
	const uint32_t n_prev = sh_n_prev; // (block_tree_sum's barriers order the atomics before this read)
	const double nd = (double)n_prev;
	for (int k = 0; k < 6; k++)
		cen[k] = cen[k] / nd;
	double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	for (uint32_t i = t; i < n; i += RT)
		if (mask_prev[i])
		{
			const float4 s = src[i], g = tgt[i];
			const double sd[3] = {(double)s.x - cen[0], (double)s.y - cen[1], (double)s.z - cen[2]};
			const double gd[3] = {(double)g.x - cen[3], (double)g.y - cen[4], (double)g.z - cen[5]};
#pragma unroll
			for (int r = 0; r < 3; r++)
#pragma unroll
				for (int c = 0; c < 3; c++)
					h[r * 3 + c] = h[r * 3 + c] + sd[r] * gd[c];
		}
	double H[9];
	for (int k = 0; k < 9; k++)
		H[k] = block_tree_sum(h[k], red);
	float m[12];
	horn_fit(H, cen, cen + 3, m); // every thread the same arithmetic on the same numbers
	// select
	uint32_t n_in = 0, diff = 0;
	for (uint32_t i = t; i < n; i += RT)
	{
		const float r2 = resid2(m, src[i], tgt[i]);
		const bool in = (double)r2 < thresh;
		d2[i] = r2;
		mask_new[i] = in ? 1 : 0;
		n_in += in ? 1u : 0u;
		diff |= (in ? 1u : 0u) ^ (mask_prev[i] ? 1u : 0u);
	}
	if (n_in)
		atomicAdd(&sh_n_new, n_in);
	if (diff)
		atomicOr(&sh_changed, 1u);
	__syncthreads();
	const uint32_t n_new = sh_n_new;
	// the selected squared distances' element of rank n_new / 2: they are not negative, so their bit patterns order as they do; four 8-bit digits
	if (t == 0)
		sh_prefix = 0, sh_rank = n_new >> 1;
	for (int level = 0; level < 4 && n_new; level++)
	{
		const int shift = 24 - 8 * level;
		hist[t & 255u] = 0; // RT == 256
		__syncthreads();
		const uint32_t prefix = sh_prefix, himask = level ? 0xffffffffu << (shift + 8) : 0u;
		for (uint32_t i = t; i < n; i += RT)
			if (mask_new[i])
			{
				const uint32_t b = __float_as_uint(d2[i]);
				if ((b & himask) == prefix)
					atomicAdd(&hist[(b >> shift) & 255u], 1u);
			}
		__syncthreads();
		if (t == 0)
		{
			uint32_t r = sh_rank, d = 0;
			for (; d < 255u; d++)
			{
				if (r < hist[d])
					break;
				r -= hist[d];
			}
			sh_rank = r;
			sh_prefix = prefix | (d << shift);
		}
		__syncthreads();
	}
	if (t == 0)
	{
		for (int k = 0; k < 12; k++)
			out->T.m[k] = m[k];
		out->n_new = n_new;
		out->changed = sh_changed;
		out->median = n_new ? __uint_as_float(sh_prefix) : 0.0f;
		out->n_prev = n_prev;
	}
}

__global__ void __launch_bounds__(RT) k_ransac_refine(const float4 *src, const float4 *tgt, uint32_t n, const uint8_t *mask_prev, uint8_t *mask_new, float *d2,
													   double thresh, RansacRound *out)
{
	refine_round(src, tgt, n, mask_prev, mask_new, d2, thresh, out);
}

// ---- the steps for a sub-batch: blockIdx.y (refine: a job) names the problem, its descriptor the places in the arena
template <typename T>
__device__ __forceinline__ T *at(unsigned char *arena, uint64_t off)
{
	return reinterpret_cast<T *>(arena + off);
}

__global__ void __launch_bounds__(256) k_rb_models(const RansacBatchDesc *desc, unsigned char *arena)
{
	const RansacBatchDesc &D = desc[blockIdx.y];
	const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
	if (h >= D.n_hyp)
		return;
	at<RansacModel>(arena, D.models)[h] = sample_model(at<const float4>(arena, D.src), at<const float4>(arena, D.tgt), at<const int32_t>(arena, D.tri) + 3u * h);
}

// k_ransac_score's body on a problem's arrays.  A workgroup belongs to one problem (blockIdx.y): its 16 hypotheses are the problem's, the 4-per-wave and
// 16-per-block tails are the problem's own n_hyp; the problem's and the wave's numbers are made scalar, so the descriptor and the models arrive by scalar loads
__global__ void __launch_bounds__(SCORE_THREADS) k_rb_score(const RansacBatchDesc *__restrict__ desc, unsigned char *arena, double thresh)
{
	const uint32_t b = __builtin_amdgcn_readfirstlane(blockIdx.y);
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x % WAVE;
	const uint32_t n = desc[b].n, n_hyp = desc[b].n_hyp, h0 = blockIdx.x * HYP_PER_BLOCK + wave * HYP_PER_WAVE;
	if (h0 >= n_hyp)
		return;
	const float4 *__restrict__ src = at<const float4>(arena, desc[b].src), *__restrict__ tgt = at<const float4>(arena, desc[b].tgt);
	const RansacModel *__restrict__ models = at<const RansacModel>(arena, desc[b].models);
	uint32_t *__restrict__ counts = at<uint32_t>(arena, desc[b].counts);
	float m[HYP_PER_WAVE][12];
#pragma unroll
	for (int j = 0; j < HYP_PER_WAVE; j++)
	{
		const uint32_t h = min(h0 + (uint32_t)j, n_hyp - 1u);
#pragma unroll
		for (int k = 0; k < 12; k++)
			m[j][k] = models[h].m[k];
	}
	uint32_t c[HYP_PER_WAVE] = {0, 0, 0, 0};
	for (uint32_t i = lane; i < n; i += WAVE)
	{
		const float4 s = src[i], t = tgt[i];
#pragma unroll
		for (int j = 0; j < HYP_PER_WAVE; j++)
			c[j] += (double)resid2(m[j], s, t) < thresh ? 1u : 0u;
	}
#pragma unroll
	for (int j = 0; j < HYP_PER_WAVE; j++)
	{
		uint32_t v = c[j];
#pragma unroll
		for (int off = WAVE / 2; off > 0; off >>= 1)
			v += __shfl_xor(v, off, WAVE);
		if (lane == 0 && h0 + (uint32_t)j < n_hyp)
			counts[h0 + j] = v;
	}
}

// the winner's mask (buffer 0) and, in the problem's winner record, its model and count (the host has zeroed the records)
__global__ void __launch_bounds__(256) k_rb_select(const RansacBatchDesc *desc, unsigned char *arena, double thresh, RansacRound *win)
{
	const RansacBatchDesc &D = desc[blockIdx.y];
	if (!D.n_hyp || blockIdx.x * blockDim.x >= D.n)
		return;
	const RansacModel *model = at<const RansacModel>(arena, D.models) + D.best;
	select_pair(at<const float4>(arena, D.src), at<const float4>(arena, D.tgt), D.n, model, thresh, at<uint8_t>(arena, D.mask), &win[blockIdx.y].n_new,
				blockIdx.x * blockDim.x + threadIdx.x);
	if (blockIdx.x == 0 && threadIdx.x < 12u)
		win[blockIdx.y].T.m[threadIdx.x] = model->m[threadIdx.x];
}

__global__ void __launch_bounds__(RT) k_rb_refine(const RansacBatchDesc *desc, const RansacBatchJob *jobs, unsigned char *arena)
{
	const RansacBatchJob J = jobs[blockIdx.x];
	const RansacBatchDesc &D = desc[J.problem];
	uint8_t *mask = at<uint8_t>(arena, D.mask);
	refine_round(at<const float4>(arena, D.src), at<const float4>(arena, D.tgt), D.n, mask + (size_t)J.prev * D.mask_stride, mask + (size_t)J.next * D.mask_stride,
				 at<float>(arena, D.d2), J.thresh, at<RansacRound>(arena, D.round));
}
} // namespace

hipError_t launch_ransac_models(hipStream_t st, const float4 *src, const float4 *tgt, const int32_t *triples, uint32_t n_hyp, RansacModel *models)
{
	hipLaunchKernelGGL(k_ransac_models, dim3((n_hyp + 255u) / 256u), dim3(256), 0, st, src, tgt, triples, n_hyp, models);
	return hipGetLastError();
}

hipError_t launch_ransac_score(hipStream_t st, const float4 *src, const float4 *tgt, uint32_t n, const RansacModel *models, uint32_t n_hyp, double thresh,
							   uint32_t *counts)
{
	hipLaunchKernelGGL(k_ransac_score, dim3((n_hyp + HYP_PER_BLOCK - 1u) / HYP_PER_BLOCK), dim3(SCORE_THREADS), 0, st, src, tgt, n, models, n_hyp, thresh, counts);
	return hipGetLastError();
}

hipError_t launch_ransac_select(hipStream_t st, const float4 *src, const float4 *tgt, uint32_t n, const RansacModel *model, double thresh, uint8_t *mask,
								uint32_t *count)
{
	hipLaunchKernelGGL(k_ransac_select, dim3((n + 255u) / 256u), dim3(256), 0, st, src, tgt, n, model, thresh, mask, count);
	return hipGetLastError();
}

hipError_t launch_ransac_refine(hipStream_t st, const float4 *src, const float4 *tgt, uint32_t n, const uint8_t *mask_prev, uint8_t *mask_new, float *d2,
								double thresh, RansacRound *out)
{
	hipLaunchKernelGGL(k_ransac_refine, dim3(1), dim3(RT), 0, st, src, tgt, n, mask_prev, mask_new, d2, thresh, out);
	return hipGetLastError();
}

// ---- the sub-batch: grids of (blocks of the largest problem) x (problems); a block past its problem's end returns
hipError_t launch_ransac_batch_models(hipStream_t st, const RansacBatchDesc *desc, uint32_t count, uint32_t n_hyp_max, unsigned char *arena)
{
	hipLaunchKernelGGL(k_rb_models, dim3((n_hyp_max + 255u) / 256u, count), dim3(256), 0, st, desc, arena);
	return hipGetLastError();
}

hipError_t launch_ransac_batch_score(hipStream_t st, const RansacBatchDesc *desc, uint32_t count, uint32_t n_hyp_max, unsigned char *arena, double thresh)
{
	hipLaunchKernelGGL(k_rb_score, dim3((n_hyp_max + HYP_PER_BLOCK - 1u) / HYP_PER_BLOCK, count), dim3(SCORE_THREADS), 0, st, desc, arena, thresh);
	return hipGetLastError();
}

hipError_t launch_ransac_batch_select(hipStream_t st, const RansacBatchDesc *desc, uint32_t count, uint32_t n_max, unsigned char *arena, double thresh, RansacRound *win)
{
	hipLaunchKernelGGL(k_rb_select, dim3((n_max + 255u) / 256u, count), dim3(256), 0, st, desc, arena, thresh, win);
	return hipGetLastError();
}

hipError_t launch_ransac_batch_refine(hipStream_t st, const RansacBatchDesc *desc, const RansacBatchJob *jobs, uint32_t n_jobs, unsigned char *arena)
{
	hipLaunchKernelGGL(k_rb_refine, dim3(n_jobs), dim3(RT), 0, st, desc, jobs, arena);
	return hipGetLastError();
}
