// fpfh_math.h — the arithmetic of mulls_fpfh and mulls_coarse_reg_fpfhsac (include/mulls_hip.h has the definition this file follows), one text for
// the device kernels (k_fpfh.hip), the host (fpfh.cpp) and a CPU build (tests/fpfh_math_harness.cpp, which tests/test_fpfh.py holds against the numpy
// restatement bit for bit): the pair feature, the bins, SPFH from integer counts, the normalisation of the weighted sum, SAC-IA's two error functions
// and, for the host only, its draw sequence.
#pragma once
#include <math.h>
#include <stdint.h>

#include "detmath.h"

#define MULLS_FPFH_BINS 11
#define MULLS_FPFH_DIMS 33

namespace fpfh
{
MULLS_HD inline double dot3(const double *u, const double *v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
MULLS_HD inline void cross3(const double *u, const double *v, double *o)
{
	o[0] = u[1] * v[2] - u[2] * v[1];
	o[1] = u[2] * v[0] - u[0] * v[2];
	o[2] = u[0] * v[1] - u[1] * v[0];
}

// The pair feature of p (normal np) and q (normal nq): f[0] = f1 (the angle), f[1] = f2, f[2] = f3; false: the pair adds nothing.
MULLS_HD inline bool pair_feature(const float *p, const float *np, const float *q, const float *nq, double *f)
{
	double dp[3] = {(double)q[0] - (double)p[0], (double)q[1] - (double)p[1], (double)q[2] - (double)p[2]};
	const double f4 = sqrt(dot3(dp, dp));
	if (f4 == 0.0)
		return false;
	const double a[3] = {(double)np[0], (double)np[1], (double)np[2]}, b[3] = {(double)nq[0], (double)nq[1], (double)nq[2]};
	const double a1 = dot3(a, dp) / f4, a2 = dot3(b, dp) / f4;
	const bool swap = fabs(a1) < fabs(a2); // acos|a1| > acos|a2|
	const double *n1 = swap ? b : a, *n2 = swap ? a : b;
	if (swap)
		dp[0] = -dp[0], dp[1] = -dp[1], dp[2] = -dp[2];
	f[2] = swap ? -a2 : a1;
	double v[3], w[3];
	cross3(dp, n1, v);
	const double nv = sqrt(dot3(v, v));
	if (nv == 0.0)
		return false;
	v[0] = v[0] / nv, v[1] = v[1] / nv, v[2] = v[2] / nv;
	cross3(n1, v, w);
	f[1] = dot3(v, n2);
	f[0] = mulls::det::atan2_cr(dot3(w, n2), dot3(n1, n2));
	return true;
}

MULLS_HD inline int clamp_bin(double x)
{
	const double b = floor(x);
	return b < 0.0 ? 0 : (b > (double)(MULLS_FPFH_BINS - 1) ? MULLS_FPFH_BINS - 1 : (int)b);
}
// the three bins of a feature (each 0 .. 10); false: a NaN feature, the pair adds nothing
MULLS_HD inline bool bins_of(const double *f, int *b)
{
	if (f[0] != f[0] || f[1] != f[1] || f[2] != f[2])
		return false;
	const double pi = 0x1.921fb54442d18p+1, inv_2pi = 1.0 / (2.0 * pi);
	b[0] = clamp_bin(11.0 * ((f[0] + pi) * inv_2pi));
	b[1] = clamp_bin(11.0 * ((f[1] + 1.0) * 0.5));
	b[2] = clamp_bin(11.0 * ((f[2] + 1.0) * 0.5));
	return true;
}
// one SPFH value from its integer count and the neighbourhood's size k (the point itself included)
MULLS_HD inline float spfh_of_count(uint32_t count, uint32_t k) { return k <= 1u ? 0.f : (float)(((double)count * 100.0) / (double)(k - 1u)); }
// one sub-histogram: the 11 weighted sums -> the 11 output values
MULLS_HD inline void normalise(const double *acc, float *out)
{
	double s = acc[0];
	for (int b = 1; b < MULLS_FPFH_BINS; b++)
		s = s + acc[b];
	for (int b = 0; b < MULLS_FPFH_BINS; b++)
	{
		const float h = s != 0.0 ? (float)(acc[b] * (100.0 / s)) : 0.f;
		out[b] = (h - h == 0.f) ? h : 0.f; // (not finite: 0)
	}
}
// the squared distance of two descriptors: the 33 differences squared and added in bin order, in float
MULLS_HD inline float desc_dist2(const float *a, const float *b)
{
	float s = 0.f;
	for (int k = 0; k < MULLS_FPFH_DIMS; k++)
	{
		const float d = a[k] - b[k];
		s = s + d * d;
	}
	return s;
}
// SAC-IA's error of one source point: e the float squared distance to its nearest target point, thr the (unsquared) range
MULLS_HD inline double error_term(float e, float thr, int huber)
{
	const double E = (double)e, T = (double)thr;
	if (huber)
		return E <= T ? (0.5 * E) * E : (0.5 * T) * (2.0 * fabs(E) - T);
	return E <= T ? E / T : 1.0;
}
// the order of SAC-IA's hypotheses: the lower error first, equal errors by the lower index, a NaN error after every number (NaNs among themselves by index)
MULLS_HD inline bool error_before(double ea, uint32_t ia, double eb, uint32_t ib)
{
	const bool na = ea != ea, nb = eb != eb;
	if (na != nb)
		return nb;
	if (!na && ea != eb)
		return ea < eb;
	return ia < ib;
}
} // namespace fpfh

// ---- host only ----
#include <random>
#include <vector>
namespace fpfh
{
// SAC-IA's draws, every iteration up front: samples[3 it + s] the source indices, ranks[3 it + s] the rank among the similar features.
// xyz: the source's packed coordinates.  -> min_sample_distance as the halving rule left it.
inline float draw_all(const float *xyz, uint32_t n_src, uint32_t k_eff, int nr_samples, int iterations, float min_sample_distance, uint32_t seed,
					  std::vector<int32_t> &samples, std::vector<int32_t> &ranks)
{
	std::mt19937 eng(seed);
	samples.assign((size_t)iterations * nr_samples, 0), ranks.assign((size_t)iterations * nr_samples, 0);
	float min_d = min_sample_distance;
	for (int it = 0; it < iterations; it++)
	{
		int32_t *S = samples.data() + (size_t)it * nr_samples;
		uint64_t rejected = 0;
		for (int have = 0; have < nr_samples;)
		{
			const uint32_t i = (uint32_t)(eng() % n_src);
			bool ok = true;
			for (int k = 0; k < have && ok; k++)
			{
				const uint32_t j = (uint32_t)S[k];
				const float dx = xyz[3 * i] - xyz[3 * j], dy = xyz[3 * i + 1] - xyz[3 * j + 1], dz = xyz[3 * i + 2] - xyz[3 * j + 2];
				ok = i != j && !(sqrtf((dx * dx + dy * dy) + dz * dz) < min_d);
			}
			if (ok)
			{
				S[have++] = (int32_t)i;
				rejected = 0;
			}
			else if (++rejected >= 3ull * n_src)
			{
				min_d = 0.5f * min_d;
				rejected = 0;
			}
		}
		for (int s = 0; s < nr_samples; s++)
			ranks[(size_t)it * nr_samples + s] = (int32_t)(eng() % k_eff);
	}
	return min_d;
}
} // namespace fpfh
