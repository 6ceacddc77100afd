// Test harness: C entry points around mulls_amd/csrc/teaser_math.h and teaser_host.h (the arithmetic the kernels run, and the host half of
// mulls_coarse_reg_teaser), with plain CPU loops in the place of the device steps (graph, core numbers, greedy bound, compaction, the GNC passes), built for
// the CPU so that tests/test_teaser.py can hold them against tests/teaser_restated.py without a device.
#include <chrono>
#include <cstring>

#include "../mulls_amd/csrc/teaser_host.h"
#include "../mulls_amd/csrc/teaser_math.h"

namespace
{
const uint32_t P = MULLS_TEASER_PARTIALS;

void measurement(const float *cs, const float *ct, uint32_t C, uint64_t k, double *a, double *b)
{
	uint32_t ia, ib;
	teaser_decode(k, C, &ia, &ib);
	for (int d = 0; d < 3; d++)
	{
		a[d] = (double)cs[4u * ib + d] - (double)cs[4u * ia + d];
		b[d] = (double)ct[4u * ib + d] - (double)ct[4u * ia + d];
	}
}

// the GNC loop as teaser.cpp drives it, the kernels' passes as loops over the partial index
int gnc_cpu(const float *cs, const float *ct, uint32_t C, double nb2, TeaserGnc &S, uint64_t *n_rot)
{
	const uint64_t M = (uint64_t)C * (C - 1u) / 2u;
	std::vector<double> w((size_t)M, 1.0), part((size_t)9u * P);
	int iters = 0;
	std::memset(&S, 0, sizeof(S));
	for (int it = 0; it < MULLS_TEASER_GNC_MAX_ITER; it++)
	{
		for (uint32_t p = 0; p < P; p++)
		{
			double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
			for (uint64_t k = p; k < M; k += P)
			{
				double a[3], b[3];
				measurement(cs, ct, C, k, a, b);
				for (int r = 0; r < 3; r++)
					for (int c = 0; c < 3; c++)
						h[r * 3 + c] = h[r * 3 + c] + (w[k] * a[r]) * b[c];
			}
			for (int q = 0; q < 9; q++)
				part[(size_t)q * P + p] = h[q];
		}
		double H[9];
		for (int q = 0; q < 9; q++)
			H[q] = teaser_tree_host(part.data() + (size_t)q * P);
		if (it > 0)
			teaser_gnc_next(&S);
		teaser_horn_rot(H, S.R);
		double mx = 0.0;
		for (uint32_t p = 0; p < P; p++)
		{
			double cost = 0.0;
			for (uint64_t k = p; k < M; k += P)
			{
				double a[3], b[3];
				measurement(cs, ct, C, k, a, b);
				const double r = teaser_resid(S.R, a, b);
				cost = cost + w[k] * r;
				if (r > mx)
					mx = r;
			}
			part[p] = cost;
		}
		teaser_gnc_decide(&S, it, teaser_tree_host(part.data()), mx, nb2);
		iters = it + 1;
		if (S.stop == 1u)
			break;
		uint32_t cnt = 0;
		for (uint64_t k = 0; k < M; k++)
		{
			double a[3], b[3];
			measurement(cs, ct, C, k, a, b);
			w[k] = teaser_weight(teaser_resid(S.R, a, b), S.mu, nb2);
			cnt += w[k] >= 0.5 ? 1u : 0u;
		}
		S.n_inlier = cnt;
		if (S.stop)
			break;
	}
	*n_rot = S.stop == 1u ? M : (uint64_t)S.n_inlier;
	return iters;
}

// core numbers by the plain sequential peeling (remove a vertex of the smallest current degree)
void cores_cpu(const TeaserBits &G, std::vector<uint32_t> &core)
{
	const uint32_t n = G.m;
	std::vector<uint32_t> deg(n);
	std::vector<char> alive(n, 1);
	for (uint32_t i = 0; i < n; i++)
		for (uint32_t w = 0; w < G.W; w++)
			deg[i] += (uint32_t)__builtin_popcountll(G.row(i)[w]);
	core.assign(n, 0);
	uint32_t k = 0;
	for (uint32_t done = 0; done < n; done++)
	{
		uint32_t v = n;
		for (uint32_t i = 0; i < n; i++)
			if (alive[i] && (v == n || deg[i] < deg[v]))
				v = i;
		k = std::max(k, deg[v]);
		core[v] = k;
		alive[v] = 0;
		for (uint32_t j = 0; j < n; j++)
			if (alive[j] && ((G.row(v)[j >> 6] >> (j & 63u)) & 1ull))
				deg[j]--;
	}
}
} // namespace

extern "C"
{
	void th_horn(const double H[9], double R[9]) { teaser_horn_rot(H, R); }
	double th_weight(double r, double mu, double nb2) { return teaser_weight(r, mu, nb2); }
	double th_tls(const double *x, uint32_t n, double range) { return teaser_tls(x, n, range); }
	int th_edge(const float *si, const float *ti, const float *sj, const float *tj, double beta) { return teaser_edge(si, ti, sj, tj, beta) ? 1 : 0; }

	// the search on a given m x ceil(m / 64) bit matrix with the greedy lower bound of teaser.cpp; out: size, nodes, exact, lb
	void th_search(const uint64_t *rows, uint32_t m, uint64_t budget, int32_t *clique, uint64_t out[4])
	{
		TeaserBits G;
		G.m = m, G.W = (m + 63u) / 64u, G.rows = rows;
		uint32_t lb = 0, lb_v = 0;
		std::vector<uint32_t> c, witness;
		for (uint32_t v = 0; v < m; v++)
		{
			teaser_greedy_clique(G, v, c);
			if (c.size() > lb)
				lb = (uint32_t)c.size(), lb_v = v, witness = c;
		}
		(void)lb_v;
		TeaserSearch S;
		S.run(G, lb, witness, budget);
		for (size_t k = 0; k < S.best_clique.size(); k++)
			clique[k] = (int32_t)S.best_clique[k];
		out[0] = S.best_clique.size(), out[1] = S.nodes, out[2] = S.aborted ? 0 : 1, out[3] = lb;
	}

	// GNC on given clique points (C x 4 floats each); ints: iterations, stop, rotation inliers; dbl: cost, mu, R[9]
	void th_gnc(const float *cs, const float *ct, uint32_t C, double nb2, int64_t ints[3], double dbl[11])
	{
		TeaserGnc S;
		uint64_t n_rot = 0;
		ints[0] = gnc_cpu(cs, ct, C, nb2, S, &n_rot);
		ints[1] = S.stop, ints[2] = (int64_t)n_rot;
		dbl[0] = S.cost, dbl[1] = S.mu;
		std::memcpy(dbl + 2, S.R, sizeof(S.R));
	}

	// the whole of mulls_coarse_reg_teaser on packed x, y, z, w floats.  ints: status, max_core, n_edges, clique_size, clique_exact, clique_nodes,
	// gnc_iterations, n_rotation_inliers, n_translation_inliers, kept vertices; dbl: cost, search seconds, T[16] column-major
	void th_solve(const float *src, const float *tgt, uint32_t n, float noise_bound, int min_inlier, uint64_t budget, int64_t ints[10], double dbl[18],
				  int32_t *clique_out)
	{
		for (int k = 0; k < 10; k++)
			ints[k] = 0;
		ints[0] = -1;
		dbl[0] = dbl[1] = 0.0;
		for (int k = 0; k < 16; k++)
			dbl[2 + k] = (k % 5 == 0) ? 1.0 : 0.0;
		if (n <= 3u)
			return;
		const uint32_t W = (n + 63u) / 64u;
		const double nb = (double)noise_bound, beta = (2.0 * nb) * sqrt(1.0);
		std::vector<uint64_t> adj((size_t)n * W, 0ull);
		uint64_t deg_sum = 0;
		for (uint32_t i = 0; i < n; i++)
			for (uint32_t j = 0; j < n; j++)
				if (i != j && teaser_edge(src + 4u * i, tgt + 4u * i, src + 4u * j, tgt + 4u * j, beta))
					adj[(size_t)i * W + (j >> 6)] |= 1ull << (j & 63u), deg_sum++;
		ints[2] = (int64_t)(deg_sum / 2u);
		TeaserBits G;
		G.m = n, G.W = W, G.rows = adj.data();
		std::vector<uint32_t> core, c;
		cores_cpu(G, core);
		uint32_t max_core = 0, lb = 0, lb_v = 0;
		for (uint32_t v = 0; v < n; v++)
		{
			max_core = std::max(max_core, core[v]);
			teaser_greedy_clique(G, v, c);
			if (c.size() > lb)
				lb = (uint32_t)c.size(), lb_v = v;
		}
		ints[1] = max_core;
		ints[4] = 1;
		std::vector<uint32_t> clique;
		std::vector<uint32_t> keep;
		if (lb <= 1u)
			clique.assign(1, 0u);
		else
		{
			uint32_t witness_at = 0;
			for (uint32_t i = 0; i < n; i++)
				if (core[i] + 1u >= lb)
				{
					if (i == lb_v)
						witness_at = (uint32_t)keep.size();
					keep.push_back(i);
				}
			const uint32_t m = (uint32_t)keep.size(), Wm = (m + 63u) / 64u;
			std::vector<uint64_t> sub((size_t)m * Wm, 0ull);
			for (uint32_t r = 0; r < m; r++)
				for (uint32_t q = 0; q < m; q++)
					if ((adj[(size_t)keep[r] * W + (keep[q] >> 6)] >> (keep[q] & 63u)) & 1ull)
						sub[(size_t)r * Wm + (q >> 6)] |= 1ull << (q & 63u);
			TeaserBits Gs;
			Gs.m = m, Gs.W = Wm, Gs.rows = sub.data();
			const auto tic = std::chrono::steady_clock::now();
			std::vector<uint32_t> witness;
			teaser_greedy_clique(Gs, witness_at, witness);
			TeaserSearch S;
			S.run(Gs, lb, witness, budget);
			dbl[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - tic).count();
			ints[5] = (int64_t)S.nodes;
			ints[4] = S.aborted ? 0 : 1;
			ints[9] = m;
			for (uint32_t v : S.best_clique)
				clique.push_back(keep[v]);
		}
		const uint32_t C = (uint32_t)clique.size();
		ints[3] = C;
		for (uint32_t k = 0; k < C; k++)
			clique_out[k] = (int32_t)clique[k];
		if (C <= 1u)
			return;
		std::vector<float> cs((size_t)4u * C), ct((size_t)4u * C);
		for (uint32_t k = 0; k < C; k++)
		{
			std::memcpy(&cs[4u * k], src + 4u * clique[k], 16);
			std::memcpy(&ct[4u * k], tgt + 4u * clique[k], 16);
		}
		double nb2 = nb * nb;
		if (nb2 < 1e-16)
			nb2 = 1e-2;
		TeaserGnc S;
		uint64_t n_rot = 0;
		ints[6] = gnc_cpu(cs.data(), ct.data(), C, nb2, S, &n_rot);
		ints[7] = (int64_t)n_rot;
		dbl[0] = S.cost;
		double that[3];
		ints[8] = teaser_translation(cs.data(), ct.data(), C, S.R, nb, that);
		const long long mi = min_inlier;
		ints[0] = (long long)n_rot >= 2 * mi ? 1 : ((long long)n_rot >= mi ? 0 : -1);
		if (ints[0] >= 0)
			for (int r = 0; r < 3; r++)
			{
				for (int c2 = 0; c2 < 3; c2++)
					dbl[2 + c2 * 4 + r] = S.R[r * 3 + c2];
				dbl[2 + 12 + r] = that[r];
			}
	}
}
