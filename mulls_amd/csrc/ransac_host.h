// ransac_host.h — the sequential, host-side parts of the RANSAC coarse registration (include/mulls_hip.h), free of HIP so that a CPU
// build can be held against the numpy restatement (tests/ransac_harness.cpp, tests/test_ransac.py): PCL's sample sequence and its threshold, PCL's sequential
// stopping rule over the hypotheses' counts, and the control flow of PCL's refineModel around a caller-supplied round.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <limits>
#include <random>
#include <vector>

// eigenvalues of a symmetric 3 x 3 (a6 = xx xy xz yy yz zz) by cyclic Jacobi on the upper triangle in double: the diagonal it ends with, in place
inline void jacobi3_eigenvalues(const double a6[6], double lam[3])
{
	double A[3][3] = {{a6[0], a6[1], a6[2]}, {a6[1], a6[3], a6[4]}, {a6[2], a6[4], a6[5]}};
	for (int sweep = 0; sweep < 60; sweep++)
	{
		const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
		if (off < 1e-300)
			break;
		for (int p = 0; p < 2; p++)
			for (int q = p + 1; q < 3; q++)
			{
				if (A[p][q] == 0.0)
					continue;
				const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
				const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
				const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
				for (int k = 0; k < 3; k++) // A <- A J
				{
					const double akp = A[k][p], akq = A[k][q];
					A[k][p] = cs * akp - sn * akq;
					A[k][q] = sn * akp + cs * akq;
				}
				for (int k = 0; k < 3; k++) // A <- J^T A
				{
					const double apk = A[p][k], aqk = A[q][k];
					A[p][k] = cs * apk - sn * aqk;
					A[q][k] = sn * apk + cs * aqk;
				}
				for (int r = 0; r < 3; r++) // the upper triangle is the matrix
					for (int c2 = r + 1; c2 < 3; c2++)
						A[c2][r] = A[r][c2];
			}
	}
	lam[0] = A[0][0], lam[1] = A[1][1], lam[2] = A[2][2];
}

// SampleConsensusModelRegistration::computeSampleDistanceThreshold: (mean of the square roots of the covariance's eigenvalues)^2
inline double sample_dist_thresh(const float *xyzw, uint32_t n)
{
	float accu[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	for (uint32_t i = 0; i < n; i++)
	{
		const float x = xyzw[4 * i], y = xyzw[4 * i + 1], z = xyzw[4 * i + 2];
		accu[0] += x * x;
		accu[1] += x * y;
		accu[2] += x * z;
		accu[3] += y * y;
		accu[4] += y * z;
		accu[5] += z * z;
		accu[6] += x;
		accu[7] += y;
		accu[8] += z;
	}
	const float nf = static_cast<float>(n);
	for (int k = 0; k < 9; k++)
		accu[k] /= nf;
	const float cov[6] = {accu[0] - accu[6] * accu[6], accu[1] - accu[6] * accu[7], accu[2] - accu[6] * accu[8],
						  accu[3] - accu[7] * accu[7], accu[4] - accu[7] * accu[8], accu[5] - accu[8] * accu[8]};
	double a6[6], lam[3];
	for (int k = 0; k < 6; k++)
		a6[k] = (double)cov[k];
	jacobi3_eigenvalues(a6, lam);
	double th = ((std::sqrt(lam[0]) + std::sqrt(lam[1])) + std::sqrt(lam[2])) / 3.0;
	return th * th;
}

inline float dist4(const float *a, const float *b)
{
	const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2], dw = a[3] - b[3];
	return (dx * dx + dz * dz) + (dy * dy + dw * dw); // Eigen's four-float packet reduction
}

// PCL's sample sequence: up to `want` triples; fewer when 1000 draws in a row give no good sample (the loop ends there)
inline void draw_triples(const float *xyzw, uint32_t n, uint32_t want, std::vector<int32_t> &triples)
{
	triples.clear();
	triples.reserve((size_t)want * 3u);
	const double thresh = sample_dist_thresh(xyzw, n);
	std::mt19937 eng(12345u);
	std::vector<int32_t> shuffled(n);
	for (uint32_t i = 0; i < n; i++)
		shuffled[i] = (int32_t)i;
	for (uint32_t h = 0; h < want; h++)
	{
		bool good = false;
		for (int check = 0; check < 1000 && !good; check++)
		{
			for (uint32_t i = 0; i < 3; i++)
				std::swap(shuffled[i], shuffled[i + (uint32_t)((eng() >> 1) % (uint32_t)(n - i))]);
			const float *p0 = xyzw + 4 * (size_t)shuffled[0], *p1 = xyzw + 4 * (size_t)shuffled[1], *p2 = xyzw + 4 * (size_t)shuffled[2];
			good = (double)dist4(p1, p0) > thresh && (double)dist4(p2, p0) > thresh && (double)dist4(p2, p1) > thresh;
		}
		if (!good)
			return;
		triples.insert(triples.end(), shuffled.begin(), shuffled.begin() + 3);
	}
}

// RandomSampleConsensus::computeModel's loop (ransac.hpp) over the counts of the n_hyp hypotheses that have a sample: std::log / std::pow as PCL calls them
inline void ransac_sequential_rule(const uint32_t *counts, uint32_t n_hyp, uint32_t n, int max_iter_num, int *iterations_out, int *best_out)
{
	int iterations = 0, n_best = -INT_MAX, best_it = -1;
	double k = 1.0;
	const double log_probability = std::log(1.0 - 0.99), one_over_indices = 1.0 / static_cast<double>(n);
	while ((double)iterations < k)
	{
		if ((uint32_t)iterations >= n_hyp) // getSamples found no good sample: "No samples could be selected!"
			break;
		const int c = (int)counts[iterations];
		if (c > n_best)
		{
			n_best = c;
			best_it = iterations;
			const double w = static_cast<double>(n_best) * one_over_indices;
			double p_no_outliers = 1.0 - std::pow(w, 3.0);
			p_no_outliers = std::max(std::numeric_limits<double>::epsilon(), p_no_outliers);
			p_no_outliers = std::min(1.0 - std::numeric_limits<double>::epsilon(), p_no_outliers);
			k = log_probability / std::log(p_no_outliers);
		}
		++iterations;
		if (iterations > max_iter_num)
			break;
	}
	*iterations_out = iterations;
	*best_out = best_it;
}

// what one refinement round reports: the size of the new inlier set, whether it differs from the previous one, its squared distances' element of rank size / 2
struct RefineStep
{
	uint32_t n_new = 0;
	bool changed = false;
	float median = 0;
};
struct RefineOutcome
{
	int rounds = 0;
	bool failed = false;	  // an empty selection, or still changing after 1000 rounds
	bool oscillating = false; // a 2-cycle of the set sizes: PCL returns true WITHOUT installing the refined model — the unrefined model and inliers stay
	int final_mask = 0;		  // the buffer that holds the final inlier set (not oscillating, not failed)
	uint32_t n_inliers = 0;
};
// RandomSampleConsensus::refineModel(3.0, 1000) (sac.h), as a state that is fed one round at a time: the one statement of its control flow.  Inlier sets live
// in three buffers: 0 holds the unrefined model's and is never written, 1 and 2 take the rounds' sets in turn.  refine_begin, then per round: fit the set in
// buffer prev, select within refine_threshold() (squared) into buffer next, and refine_feed what the round reports; it answers whether another round runs
// (prev / next / the threshold are then the next round's) or the refinement has ended (o is complete).  mulls_coarse_reg_ransac_batch keeps one state per
// problem, as its problems stand at different rounds.
struct RefineState
{
	double thr_sqr = 0, error_threshold = 0;
	int prev = 0, next = 1;
	uint32_t prev_size = 0;
	std::vector<uint32_t> sizes;
	RefineOutcome o;
};
inline void refine_begin(RefineState &s, double noise_bound, uint32_t n_in)
{
	s.thr_sqr = noise_bound * noise_bound;
	s.error_threshold = noise_bound;
	s.prev = 0, s.next = 1;
	s.prev_size = n_in;
	s.sizes.clear();
	s.o = RefineOutcome();
}
inline double refine_threshold(const RefineState &s) { return s.error_threshold * s.error_threshold; }
inline bool refine_feed(RefineState &s, const RefineStep &step)
{
	const double sigma_sqr = 3.0 * 3.0;
	s.o.rounds++;
	s.sizes.push_back(s.prev_size);
	uint32_t new_size = step.n_new;
	if (!new_size) // PCL fits the same set again until its round limit, and fails: the outcome without the rounds
	{
		s.o.failed = true;
		return false;
	}
	const double variance = 2.1981 * (double)step.median; // computeVariance
	s.error_threshold = std::sqrt(std::min(s.thr_sqr, sigma_sqr * variance));
	std::swap(s.prev_size, new_size);
	s.prev = s.next;
	s.next = s.prev == 1 ? 2 : 1;
	bool inlier_changed = step.changed;
	if (new_size != s.prev_size)
	{
		const size_t m = s.sizes.size();
		if (m >= 4 && s.sizes[m - 1] == s.sizes[m - 3] && s.sizes[m - 2] == s.sizes[m - 4])
		{
			s.o.oscillating = true;
			return false;
		}
		inlier_changed = true;
	}
	if (inlier_changed && s.o.rounds < 1000)
		return true;
	s.o.failed = inlier_changed;
	s.o.final_mask = s.prev;
	s.o.n_inliers = s.prev_size;
	return false;
}
// the same as a loop around round(prev, next, thresh, step): one launch and one wait per round in the single call; non-zero = error
template <typename Round>
int refine_control(double noise_bound, uint32_t n_in, RefineOutcome &o, Round &&round)
{
	RefineState s;
	refine_begin(s, noise_bound, n_in);
	for (bool more = true; more;)
	{
		RefineStep step;
		o = s.o;
		if (int rc = round(s.prev, s.next, refine_threshold(s), step))
			return rc;
		more = refine_feed(s, step);
	}
	o = s.o;
	return 0;
}
