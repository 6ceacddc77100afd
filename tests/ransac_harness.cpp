// Test harness: C entry points around mulls_amd/csrc/ransac_math.h and ransac_host.h (the estimator the kernels run, and the host half of
// mulls_coarse_reg_ransac), built for the CPU so that tests/test_ransac.py can hold them against tests/ransac_restated.py without a device.
#include <cstring>

#include "../mulls_amd/csrc/ransac_host.h"
#include "../mulls_amd/csrc/ransac_math.h"

extern "C"
{
	void rh_horn(const double H[9], const double cs[3], const double ct[3], float out[12]) { horn_fit(H, cs, ct, out); }
	double rh_sample_dist_thresh(const float *xyzw, uint32_t n) { return sample_dist_thresh(xyzw, n); }
	int rh_draws(const float *xyzw, uint32_t n, uint32_t want, int32_t *out)
	{
		std::vector<int32_t> t;
		draw_triples(xyzw, n, want, t);
		if (!t.empty())
			std::memcpy(out, t.data(), t.size() * sizeof(int32_t));
		return (int)(t.size() / 3);
	}
	void rh_sequential(const uint32_t *counts, uint32_t n_hyp, uint32_t n, int max_iter, int out[2]) { ransac_sequential_rule(counts, n_hyp, n, max_iter, out, out + 1); }
	// refine_control over a script of rounds: n_new / changed / median per round (the last entry repeats when the script runs out).
	// out: rounds, failed, oscillating, final_mask, n_inliers; log[3 r ..]: prev, next of round r and whether its threshold equals thresholds[r] exactly
	void rh_refine(double noise_bound, uint32_t n_in, const uint32_t *n_new, const int32_t *changed, const float *median, int n_script, int out[5], int *log,
				   double *thresholds, int log_cap)
	{
		RefineOutcome o;
		int r = 0;
		refine_control(noise_bound, n_in, o, [&](int prev, int next, double thresh, RefineStep &s) -> int {
			const int k = r < n_script ? r : n_script - 1;
			s.n_new = n_new[k], s.changed = changed[k] != 0, s.median = median[k];
			if (r < log_cap)
				log[2 * r] = prev, log[2 * r + 1] = next, thresholds[r] = thresh;
			r++;
			return 0;
		});
		out[0] = o.rounds, out[1] = o.failed, out[2] = o.oscillating, out[3] = o.final_mask, out[4] = (int)o.n_inliers;
	}
}
