// fpfh_device.h — SAC-IA's device steps as __device__ functions, one text for the kernels of one problem (k_fpfh.hip, whose launch arguments are the
// problem's sizes) and the kernels of many (k_fpfh_batch.hip, which read the sizes from a per-problem table): the similar features of a sample, the
// model of a hypothesis, the slot of a hypothesis in the nearest-target pass, its error, and the pick.  Every loop is bounded by an argument or a constant.
#pragma once
#include <hip/hip_runtime.h>

#include "fpfh_launch.h"
#include "ransac_math.h"
#include "reg_device.h"

namespace fpfh_dev
{
constexpr uint32_t NO_POINT = 0xffffffffu;

// Similar features.  A wave per sample s: lane l keeps the l-th smallest (d2, index) seen so far in registers.  64 target descriptors a step, a lane
// each; a candidate before the list's entry of rank k_eff - 1 is inserted by a shift across the lanes.  Every lane of the wave calls this.
__device__ __forceinline__ void similar_wave(const float *__restrict__ src_hist, const float *__restrict__ tgt_hist, const int32_t *__restrict__ samples,
											 const int32_t *__restrict__ ranks, uint32_t s, uint32_t n_src, uint32_t n_tgt, uint32_t k_eff, uint32_t lane, int32_t *corr)
{
	if (k_eff == 0u || k_eff > 64u)
		return;
	const uint32_t si = (uint32_t)samples[s] < n_src ? (uint32_t)samples[s] : 0u;
	float a[MULLS_FPFH_DIMS];
#pragma unroll
	for (int k = 0; k < MULLS_FPFH_DIMS; k++)
		a[k] = src_hist[(size_t)MULLS_FPFH_DIMS * si + k];
	float ld = __builtin_huge_valf();
	uint32_t li = NO_POINT;
	for (uint32_t base = 0; base < n_tgt; base += 64u)
	{
		const uint32_t t = base + lane;
		float cd = __builtin_huge_valf();
		uint32_t ci = NO_POINT;
		if (t < n_tgt)
		{
			cd = fpfh::desc_dist2(a, tgt_hist + (size_t)MULLS_FPFH_DIMS * t), ci = t;
		}
		unsigned long long mask = __ballot(pcl_icp::before(cd, ci, __shfl(ld, (int)k_eff - 1), __shfl(li, (int)k_eff - 1)));
		while (mask)
		{
			const int c = __ffsll((long long)mask) - 1;
			mask &= mask - 1ull;
			const float xd = __shfl(cd, c);
			const uint32_t xi = __shfl(ci, c);
			if (!pcl_icp::before(xd, xi, __shfl(ld, (int)k_eff - 1), __shfl(li, (int)k_eff - 1)))
				continue;
			const uint32_t pos = (uint32_t)__popcll(__ballot(pcl_icp::before(ld, li, xd, xi))); // (the list is sorted: those before are its first pos lanes)
			const float pd = __shfl_up(ld, 1);
			const uint32_t pi = __shfl_up(li, 1);
			if (lane == pos)
				ld = xd, li = xi;
			else if (lane > pos)
				ld = pd, li = pi;
		}
	}
	const uint32_t r = (uint32_t)ranks[s] < k_eff ? (uint32_t)ranks[s] : 0u;
	const uint32_t pick = __shfl(li, (int)r);
	if (lane == 0u)
		corr[s] = pick < n_tgt ? (int32_t)pick : -1;
}

// the model of one hypothesis: samples[0 .. 2] and corr[0 .. 2] are its three pairs, frame its 12 doubles
__device__ __forceinline__ void model_of(const float *__restrict__ src, const float *__restrict__ tgt, const int32_t *__restrict__ samples,
										 const int32_t *__restrict__ corr, uint32_t n_src, uint32_t n_tgt, double *frame)
{
	float s[3][3], t[3][3];
	for (int k = 0; k < 3; k++)
	{
		const uint32_t i = (uint32_t)samples[k] < n_src ? (uint32_t)samples[k] : 0u, m = (uint32_t)corr[k] < n_tgt ? (uint32_t)corr[k] : 0u;
		for (int a = 0; a < 3; a++)
			s[k][a] = src[3 * i + a], t[k][a] = tgt[3 * m + a];
	}
	float M[12];
	fit_three_pairs(s, t, M);
	for (int r = 0; r < 3; r++)
	{
		for (int a = 0; a < 3; a++)
			frame[3 * r + a] = (double)M[4 * r + a];
		frame[9 + r] = (double)M[4 * r + 3];
	}
}

// the descriptor and the record of one slot of the nearest-target pass: base with its distances at o_dist
__device__ __forceinline__ void slot_of(const NdtDesc &base, uint32_t n_src, uint32_t n_tgt, uint64_t o_dist, NdtDesc *desc, NdtRec *rec)
{
	NdtDesc d = base;
	d.o_dist = o_dist;
	*desc = d;
	rec->status = NDT_ST_OK, rec->n_src = n_src, rec->n_tgt = n_tgt, rec->fitness = 0.0;
}

// a workgroup of 256: the error terms of n_src distances by the strided-partial rule; the sum is thread 0's
__device__ __forceinline__ double error_sum(const float *__restrict__ dist, uint32_t n_src, float thr, int huber, double *s_p)
{
	const uint32_t t = threadIdx.x;
	double r[16];
#pragma unroll
	for (int m = 0; m < 16; m++)
	{
		double a = 0.0;
		for (uint32_t i = t + 256u * m; i < n_src; i += MULLS_NDT_TREE)
			a += fpfh::error_term(dist[i], thr, huber);
		r[m] = a;
	}
	return tree_of_partials(r, s_p);
}

// a workgroup of 256: the first of n_hyp hypotheses by fpfh::error_before: the lowest error, the first among equals, a NaN error after every number.
// -> the winner (every thread), its error in s_e[0]
__device__ __forceinline__ uint32_t pick_first(const double *__restrict__ err, uint32_t n_hyp, double *s_e, uint32_t *s_i)
{
	const uint32_t t = threadIdx.x;
	double be = 0.0;
	uint32_t bi = NO_POINT;
	for (uint32_t h = t; h < n_hyp; h += 256u)
		if (bi == NO_POINT || fpfh::error_before(err[h], h, be, bi))
			be = err[h], bi = h;
	s_e[t] = be, s_i[t] = bi;
	__syncthreads();
	for (uint32_t w = 128; w >= 1; w >>= 1)
	{
		if (t < w)
		{
			const double oe = s_e[t + w];
			const uint32_t oi = s_i[t + w];
			if (oi != NO_POINT && (s_i[t] == NO_POINT || fpfh::error_before(oe, oi, s_e[t], s_i[t])))
				s_e[t] = oe, s_i[t] = oi;
		}
		__syncthreads();
	}
	return s_i[0] < n_hyp ? s_i[0] : 0u;
}
// ... and the winner into out
__device__ __forceinline__ void pick_into(const double *__restrict__ err, const double *__restrict__ frames, uint32_t n_hyp, FpfhSacOut *out, double *s_e, uint32_t *s_i)
{
	const uint32_t t = threadIdx.x, best = pick_first(err, n_hyp, s_e, s_i);
	if (t == 0)
		out->best = (int32_t)best, out->pad = 0, out->error = s_e[0];
	if (t < 12)
		out->frame[t] = frames[12u * best + t];
}
} // namespace fpfh_dev
