// Test harness: C entry points around mulls_amd/csrc/sor_math.h (the arithmetic the kernels of mulls_sor_filter run), built for the CPU so that
// tests/test_sor.py can hold it against tests/sor_restated.py without a device.
#include <vector>

#include "../mulls_amd/csrc/sor_math.h"

namespace
{
template <int CAP>
float kbest_mean(const float *q, const float *pts, uint32_t n, int kk, float *worst)
{
	SorKBest<CAP> kb;
	kb.init(kk);
	for (uint32_t i = 0; i < n; i++)
		kb.insert(sor_d2(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], q[0], q[1], q[2]));
	*worst = kb.worst();
	return kb.mean_dist(kk);
}
} // namespace

extern "C"
{
	// dist[i] of every point of a cloud (x, y, z triples) by exhaustive insertion into the k-best list of capacity cap (9, 17, 33 or 65)
	int sh_mean_dists(const float *pts, uint32_t n, int mean_k, int cap, float *dist, float *worst)
	{
		const int kk = mean_k + 1;
		if (kk > cap)
			return -1;
		for (uint32_t i = 0; i < n; i++)
		{
			const float *q = pts + 3 * i;
			if (cap == 9)
				dist[i] = kbest_mean<9>(q, pts, n, kk, worst + i);
			else if (cap == 17)
				dist[i] = kbest_mean<17>(q, pts, n, kk, worst + i);
			else if (cap == 33)
				dist[i] = kbest_mean<33>(q, pts, n, kk, worst + i);
			else if (cap == 65)
				dist[i] = kbest_mean<65>(q, pts, n, kk, worst + i);
			else
				return -1;
		}
		return 0;
	}
	float sh_mean_dist_list(const float *d2, int kk) { return sor_mean_dist_list(d2, kk); }
	// sum and sq_sum in the defined order, then mean, stddev, threshold: out[5]
	void sh_statistics(const float *dist, uint32_t n, double std_mul, double *out)
	{
		std::vector<double> s(2 * MULLS_SOR_PARTIALS);
		for (uint32_t p = 0; p < MULLS_SOR_PARTIALS; p++)
			sor_partial(dist, n, p, &s[p], &s[MULLS_SOR_PARTIALS + p]);
		for (uint32_t half = MULLS_SOR_PARTIALS / 2u; half > 0u; half >>= 1)
			for (uint32_t p = 0; p < half; p++)
			{
				sor_tree_step(s.data(), half, p);
				sor_tree_step(s.data() + MULLS_SOR_PARTIALS, half, p);
			}
		out[0] = s[0], out[1] = s[MULLS_SOR_PARTIALS];
		sor_statistics(out[0], out[1], n, std_mul, out + 2);
	}
	int sh_keeps(float dist, double threshold) { return sor_keeps(dist, threshold) ? 1 : 0; }
	int sh_certified(float kth, int R, double edge) { return sor_certified(kth, R, edge) ? 1 : 0; }
	long long sh_cell(float x, double lo, double inv_edge) { return (long long)sor_cell(x, lo, inv_edge); }
	unsigned sh_constants(int which) { return which == 0 ? MULLS_SOR_MAX_K : which == 1 ? MULLS_SOR_MAX_POINTS : MULLS_SOR_PARTIALS; }
}
