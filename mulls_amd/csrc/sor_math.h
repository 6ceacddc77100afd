// sor_math.h — the arithmetic of the statistical outlier removal (include/mulls_hip.h: mulls_sor_filter), one text for the device
// kernels (k_sor.hip) and for a CPU build (tests/sor_harness.cpp, which tests/test_sor.py holds against the numpy restatement bit for bit): the distance
// expression, the k-best insertion, the mean-distance expression and the order of the statistics' sums.  Built with -ffp-contract=off on both sides.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SOR_HD __host__ __device__ __forceinline__
#define SOR_UNROLL _Pragma("unroll")
#else
#define SOR_HD inline
#define SOR_UNROLL
#endif

#define MULLS_SOR_MAX_K 64			  // mean_k's ceiling: the largest k-best capacity is MULLS_SOR_MAX_K + 1
#define MULLS_SOR_MAX_POINTS 16777216u // 2^24: the size ceiling of mulls_sor_filter
#define MULLS_SOR_PARTIALS 16384u	  // the statistics' strided partial sums: part of the definition, not a tuning knob

// squared distance, float, L2_Simple's order
SOR_HD float sor_d2(float ax, float ay, float az, float bx, float by, float bz)
{
	const float dx = ax - bx, dy = ay - by, dz = az - bz;
	return (dx * dx + dy * dy) + dz * dz;
}

// The kk = mean_k + 1 smallest values seen so far, ascending in a[CAP - kk .. CAP - 1]; the slots in front of them hold -inf, which no value passes, so
// one text serves every kk <= CAP with static indices only (the list stays in registers).  Only the multiset of the inserted values matters.
template <int CAP>
struct SorKBest
{
	float a[CAP];
	SOR_HD void init(int kk)
	{
		SOR_UNROLL
		for (int j = 0; j < CAP; j++)
			a[j] = j < CAP - kk ? -INFINITY : INFINITY;
	}
	SOR_HD float worst() const { return a[CAP - 1]; }
	SOR_HD void insert(float v)
	{
		if (!(v < a[CAP - 1]))
			return;
		a[CAP - 1] = v;
		SOR_UNROLL
		for (int j = CAP - 1; j > 0; j--)
		{
			const float lo = fminf(a[j - 1], a[j]), hi = fmaxf(a[j - 1], a[j]);
			a[j - 1] = lo, a[j] = hi;
		}
	}
	// dist = (float)(sum of sqrt((double)d2) over the mean_k values behind the smallest, ascending, / mean_k)
	SOR_HD float mean_dist(int kk) const
	{
		double s = 0.0;
		SOR_UNROLL
		for (int j = 1; j < CAP; j++)
			if (j > CAP - kk)
				s += sqrt((double)a[j]);
		return (float)(s / (double)(kk - 1));
	}
};

// the same expression over an ascending list d2[0 .. kk - 1] in memory (the leftover kernel's selection)
SOR_HD float sor_mean_dist_list(const float *d2, int kk)
{
	double s = 0.0;
	for (int j = 1; j < kk; j++)
		s += sqrt((double)d2[j]);
	return (float)(s / (double)(kk - 1));
}

// Statistics, the defined order: partial p (p < MULLS_SOR_PARTIALS) adds the terms of i = p, p + P, p + 2 P, ... in ascending i;
// then a pairwise tree, half = P / 2, P / 4, ..., 1: s[p] += s[p + half] for p < half; the sum is s[0].
SOR_HD void sor_partial(const float *dist, uint32_t n, uint32_t p, double *sum, double *sq)
{
	double s = 0.0, q = 0.0;
	for (uint64_t i = p; i < n; i += MULLS_SOR_PARTIALS)
	{
		const float d = dist[i];
		s += (double)d;
		q += (double)(d * d);
	}
	*sum = s, *sq = q;
}
SOR_HD void sor_tree_step(double *s, uint32_t half, uint32_t p) { s[p] += s[p + half]; }
// mean, stddev, threshold out of the two sums
SOR_HD void sor_statistics(double sum, double sq_sum, uint32_t n, double std_mul, double out[3])
{
	const double mean = sum / (double)n;
	const double variance = (sq_sum - sum * sum / (double)n) / ((double)n - 1.0);
	const double stddev = sqrt(variance);
	out[0] = mean, out[1] = stddev, out[2] = mean + std_mul * stddev;
}
// removed iff (double)dist > threshold (a NaN threshold keeps every point)
SOR_HD bool sor_keeps(float dist, double threshold) { return !((double)dist > threshold); }

// Cell coordinate of the uniform grid, in double so that the assignment's rounding is far below the certificate's margin: monotone in x.
SOR_HD int64_t sor_cell(float x, double lo, double inv_edge) { return (int64_t)floor(((double)x - lo) * inv_edge); }
// A query that scanned every cell of Chebyshev ring <= R around its own holds everything nearer than R * edge: its kk-th best is certain when
// its squared value is at most (R * edge)^2 less a margin of 2^-18 relative, which covers the float rounding of the distances (< 2^-21 relative) and the
// double rounding of the cell assignment (< 2^-30 of a cell for coordinates below 2^21).
SOR_HD bool sor_certified(float kth_d2, int R, double edge)
{
	const double r = (double)R * edge;
	return (double)kth_d2 <= r * r * (1.0 - 1.0 / 262144.0);
}
