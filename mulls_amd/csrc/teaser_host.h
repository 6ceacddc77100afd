// teaser_host.h — the host half of mulls_coarse_reg_teaser (teaser.cpp): the exact maximum-clique search on the compacted bit matrix, the witness of the
// greedy lower bound, and TEASER's scalar TLS estimator for the translation.  No HIP in here: tests/teaser_harness.cpp compiles this file for the CPU and
// tests/test_teaser.py holds it against the numpy restatement.  include/mulls_hip.h has the definition.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "teaser_math.h"

// an m x W bit matrix, W = ceil(m / 64): bit j of row i = edge {i, j}, zero diagonal, no bit at or above m
struct TeaserBits
{
	uint32_t m = 0, W = 0;
	const uint64_t *rows = nullptr;
	const uint64_t *row(uint32_t i) const { return rows + (size_t)i * W; }
};

// The greedy clique of vertex v (what k_teaser_greedy counts): v, then again and again the smallest vertex adjacent to all members so far.
inline void teaser_greedy_clique(const TeaserBits &G, uint32_t v, std::vector<uint32_t> &out)
{
	std::vector<uint64_t> p(G.row(v), G.row(v) + G.W);
	out.assign(1, v);
	for (uint32_t step = 0; step < G.m; step++)
	{
		uint32_t w = 0;
		while (w < G.W && !p[w])
			w++;
		if (w == G.W)
			break;
		const uint32_t u = w * 64u + (uint32_t)__builtin_ctzll(p[w]);
		const uint64_t *r = G.row(u);
		for (uint32_t k = 0; k < G.W; k++)
			p[k] &= r[k];
		out.push_back(u);
	}
	std::sort(out.begin(), out.end());
}

// The lexicographically smallest maximum clique among cliques of at least `lb` vertices: a depth-first search that extends the current clique by its
// candidates in ascending order (so cliques are met in lexicographic order and the first of a size is the smallest of that size), accepts strict
// improvements only, and cuts a node when its clique plus a greedy colouring of its candidates cannot improve.  It visits at most `budget` nodes.
struct TeaserSearch
{
	TeaserBits G;
	uint64_t budget = 0, nodes = 0;
	bool aborted = false;
	uint32_t best = 0; // a clique must have more vertices than this to be accepted
	std::vector<uint32_t> best_clique, cur;
	std::vector<std::vector<uint64_t>> pool; // the candidate set of every depth, and two sets for the colouring
	std::vector<uint64_t> q, u;

	static uint32_t count(const std::vector<uint64_t> &s)
	{
		uint32_t c = 0;
		for (uint64_t w : s)
			c += (uint32_t)__builtin_popcountll(w);
		return c;
	}
	// does a greedy colouring of p need more than `room` colours?  (colour classes are independent sets: a clique takes one vertex of each at most)
	bool colours_exceed(const std::vector<uint64_t> &p, uint32_t room)
	{
		q = p;
		for (uint32_t colours = 0;;)
		{
			uint32_t w0 = 0;
			while (w0 < G.W && !q[w0])
				w0++;
			if (w0 == G.W)
				return false;
			if (++colours > room)
				return true;
			u = q;
			for (uint32_t w = w0; w < G.W; w++)
				while (u[w])
				{
					const uint32_t b = (uint32_t)__builtin_ctzll(u[w]), v = w * 64u + b;
					q[w] &= ~(1ull << b);
					u[w] &= ~(1ull << b);
					const uint64_t *r = G.row(v);
					for (uint32_t k = w; k < G.W; k++)
						u[k] &= ~r[k];
				}
		}
	}
	void expand(uint32_t depth)
	{
		if (++nodes > budget)
		{
			aborted = true;
			return;
		}
		uint32_t left = count(pool[depth]);
		if (!left)
		{
			if (cur.size() > best)
				best = (uint32_t)cur.size(), best_clique = cur;
			return;
		}
		if (cur.size() + left <= best || (cur.size() < best && !colours_exceed(pool[depth], best - (uint32_t)cur.size())))
			return;
		if (pool.size() < depth + 2u)
			pool.resize(depth + 2u, std::vector<uint64_t>(G.W));
		for (uint32_t w = 0; w < G.W; w++)
			while (pool[depth][w])
			{
				if (cur.size() + left <= best)
					return;
				left--;
				const uint32_t b = (uint32_t)__builtin_ctzll(pool[depth][w]), v = w * 64u + b;
				pool[depth][w] &= ~(1ull << b); // what is left are the candidates above v
				const uint64_t *r = G.row(v);
				for (uint32_t k = 0; k < G.W; k++)
					pool[depth + 1u][k] = k < w ? 0ull : (pool[depth][k] & r[k]);
				cur.push_back(v);
				expand(depth + 1u);
				cur.pop_back();
				if (aborted)
					return;
			}
	}
	// witness: a clique of lb vertices (ascending), used when the budget ends the search before it has accepted one
	void run(const TeaserBits &g, uint32_t lb, const std::vector<uint32_t> &witness, uint64_t node_budget)
	{
		G = g, budget = node_budget, nodes = 0, aborted = false;
		best = lb ? lb - 1u : 0u;
		best_clique.clear(), cur.clear();
		pool.assign(2, std::vector<uint64_t>(G.W));
		for (uint32_t i = 0; i < G.m; i++)
			pool[0][i >> 6] |= 1ull << (i & 63u);
		expand(0);
		if (best_clique.empty())
			best_clique = witness;
	}
};

// TEASER's scalar TLS estimator with one range for all values: the estimate and nothing else (the caller derives the inliers).
//   endpoints x - range (opening) and x + range (closing), sorted by (value, opening before closing, index);
//   running sums over the consensus set, updated in that order; the candidate after each endpoint is sum(w x) / sum(w), w = 1 / range^2;
//   its cost is the consensus residual plus the ranges of the excluded; the first strictly smallest cost wins, a NaN never; none: 0.
inline double teaser_tls(const double *x, uint32_t n, double range)
{
	struct End
	{
		double v;
		int closing;
		uint32_t i;
	};
	std::vector<End> e(2u * (size_t)n);
	for (uint32_t i = 0; i < n; i++)
		e[2u * i] = End{x[i] - range, 0, i}, e[2u * i + 1u] = End{x[i] + range, 1, i};
	std::sort(e.begin(), e.end(), [](const End &a, const End &b) {
		if (a.v < b.v || b.v < a.v)
			return a.v < b.v;
		if (a.closing != b.closing)
			return a.closing < b.closing;
		return a.i < b.i;
	});
	const double w = 1.0 / (range * range);
	double excluded = 0.0;
	for (uint32_t i = 0; i < n; i++)
		excluded = excluded + range;
	double sw = 0.0, swx = 0.0, swx2 = 0.0, best = INFINITY, est = 0.0;
	for (const End &p : e)
	{
		const double xi = x[p.i], wx = w * xi;
		if (!p.closing)
			sw = sw + w, swx = swx + wx, swx2 = swx2 + wx * xi, excluded = excluded - range;
		else
			sw = sw - w, swx = swx - wx, swx2 = swx2 - wx * xi, excluded = excluded + range;
		const double xhat = swx / sw;
		const double cost = (((sw * xhat) * xhat + swx2) - (2.0 * swx) * xhat) + excluded;
		if (cost < best)
			best = cost, est = xhat;
	}
	return est;
}

// translation of the clique's C points under R (row-major): per axis x_c = t_c - (R s_c), the TLS estimate; inliers are within range on all three axes.
// s, t: C x 4 floats (x, y, z, unused).
inline uint32_t teaser_translation(const float *s, const float *t, uint32_t C, const double *R, double range, double *that)
{
	std::vector<double> x((size_t)3 * C);
	for (uint32_t c = 0; c < C; c++)
	{
		const double sx = (double)s[4u * c], sy = (double)s[4u * c + 1u], sz = (double)s[4u * c + 2u];
		for (int a = 0; a < 3; a++)
			x[(size_t)a * C + c] = (double)t[4u * c + a] - ((R[3 * a] * sx + R[3 * a + 1] * sy) + R[3 * a + 2] * sz);
	}
	for (int a = 0; a < 3; a++)
		that[a] = teaser_tls(x.data() + (size_t)a * C, C, range);
	uint32_t n_in = 0;
	for (uint32_t c = 0; c < C; c++)
		n_in += (fabs(x[c] - that[0]) <= range && fabs(x[(size_t)C + c] - that[1]) <= range && fabs(x[2u * (size_t)C + c] - that[2]) <= range) ? 1u : 0u;
	return n_in;
}
