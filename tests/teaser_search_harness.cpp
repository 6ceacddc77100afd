// Test harness: mulls_amd/csrc/teaser_search.h (the scheme of the device clique search of mulls_coarse_reg_teaser: plan, phase control, one worker's
// launch restated for a scalar machine) behind a serial executor that runs the tasks in a chosen order — forward, reverse or shuffled — on a few workers
// with a small quota, so that tasks are kept across launches, and optionally "stale": no task ever sees another task's incumbent or lowest rank.  Built
// for the CPU so that tests/test_teaser_search.py can hold the scheme against the numpy restatement without a device.  The steps in front of the search
// (core numbers, greedy bound, compaction) are plain loops, as in tests/teaser_harness.cpp.
#include <cstring>
#include <random>

#include "../mulls_amd/csrc/teaser_search.h"

namespace
{
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

struct SerialExec
{
	TeaserScalar S;
	TeaserSearchCtl ctl;
	std::vector<TeaserWorker> workers;
	std::vector<uint32_t> order; // the queue: every rank once
	size_t pos = 0;
	uint32_t quota = 0, witness_at = 0;

	int begin(int phase, uint32_t bound)
	{
		std::memset(&ctl, 0, sizeof(ctl));
		ctl.bound = bound, ctl.best_rank = MULLS_TEASER_NO_RANK;
		S.ctl = &ctl, S.phase = phase, S.omega = bound;
		for (TeaserWorker &w : workers)
			w = TeaserWorker();
		pos = 0;
		return 0;
	}
	int launch(TeaserSearchCtl *out)
	{
		for (TeaserWorker &w : workers)
			S.launch(w, quota, [&](uint32_t *rank) {
				while (pos < order.size())
				{
					*rank = order[pos++];
					if (S.stale || !S.phase || *rank < ctl.best_rank) // (a task above the lowest rank that succeeded is not started)
						return true;
				}
				return false;
			});
		*out = ctl;
		return 0;
	}
	int clique(uint32_t rank, std::vector<uint32_t> *out)
	{
		for (const TeaserWorker &w : workers)
			if (w.s.found == rank)
			{
				*out = w.list;
				return 0;
			}
		return MULLS_TEASER_SEARCH_FAILED;
	}
	int witness(std::vector<uint32_t> *out)
	{
		teaser_greedy_clique(S.G, witness_at, *out);
		return 0;
	}
};

// the steps in front of the search, kept for the next call on the same matrix (the tests run one graph in many orders)
struct Prepared
{
	uint64_t hash = 0;
	uint32_t n = 0xffffffffu, lb = 0, lb_v = 0, max_core = 0, witness_at = 0;
	std::vector<uint32_t> keep, later;
	std::vector<uint64_t> sub;
};
const Prepared &prepare(const uint64_t *rows, uint32_t n)
{
	static Prepared Q;
	TeaserBits G;
	G.m = n, G.W = (n + 63u) / 64u, G.rows = rows;
	uint64_t hash = 1469598103934665603ull;
	for (size_t k = 0; k < (size_t)n * G.W; k++)
		hash = (hash ^ rows[k]) * 1099511628211ull;
	if (Q.n == n && Q.hash == hash)
		return Q;
	Q = Prepared();
	Q.n = n, Q.hash = hash;
	std::vector<uint32_t> core, c;
	cores_cpu(G, core);
	for (uint32_t v = 0; v < n; v++)
	{
		Q.max_core = std::max(Q.max_core, core[v]);
		teaser_greedy_clique(G, v, c);
		if (c.size() > Q.lb)
			Q.lb = (uint32_t)c.size(), Q.lb_v = v;
	}
	if (Q.lb <= 1u)
		return Q;
	for (uint32_t i = 0; i < n; i++)
		if (core[i] + 1u >= Q.lb)
		{
			if (i == Q.lb_v)
				Q.witness_at = (uint32_t)Q.keep.size();
			Q.keep.push_back(i);
		}
	const uint32_t m = (uint32_t)Q.keep.size(), Wm = (m + 63u) / 64u;
	Q.sub.assign((size_t)m * Wm, 0ull), Q.later.assign(m, 0u);
	for (uint32_t r = 0; r < m; r++)
		for (uint32_t q = 0; q < m; q++)
			if ((rows[(size_t)Q.keep[r] * G.W + (Q.keep[q] >> 6)] >> (Q.keep[q] & 63u)) & 1ull)
				Q.sub[(size_t)r * Wm + (q >> 6)] |= 1ull << (q & 63u), Q.later[r] += q > r ? 1u : 0u;
	return Q;
}
} // namespace

extern "C"
{
	// The scheme on a given n x ceil(n / 64) bit matrix, with the steps of teaser.cpp in front of it.  order_mode 0: forward, 1: reverse, 2: shuffled by `seed`.
	// clique: original numbering.  out: size, nodes, exact, lb, omega, tasks, launches, kept vertices, the vertex that gave lb; returns 0 or the control's error
	int ts_search(const uint64_t *rows, uint32_t n, uint64_t budget, int order_mode, uint32_t seed, int stale, uint32_t n_workers, uint32_t quota, int32_t *clique,
				  uint64_t out[9])
	{
		const Prepared &Q = prepare(rows, n);
		const uint32_t lb = Q.lb, max_core = Q.max_core, m = (uint32_t)Q.keep.size(), Wm = (m + 63u) / 64u;
		const std::vector<uint32_t> &keep = Q.keep;
		for (int k = 0; k < 9; k++)
			out[k] = 0;
		out[3] = lb, out[8] = Q.lb_v;
		if (lb <= 1u)
		{
			clique[0] = 0, out[0] = 1, out[2] = 1;
			return 0;
		}
		TeaserPlan P;
		teaser_plan(Q.later.data(), m, lb, max_core, P);
		SerialExec ex;
		ex.S.G.m = m, ex.S.G.W = Wm, ex.S.G.rows = Q.sub.data();
		ex.S.P = &P, ex.S.stale = stale != 0;
		ex.workers.resize(std::max(1u, n_workers));
		ex.quota = std::max(1u, quota), ex.witness_at = Q.witness_at;
		ex.order.resize(P.n_tasks);
		for (uint32_t k = 0; k < P.n_tasks; k++)
			ex.order[k] = order_mode == 1 ? P.n_tasks - 1u - k : k;
		if (order_mode == 2)
		{
			std::mt19937 rng(seed);
			for (uint32_t k = P.n_tasks; k > 1u; k--) // (Fisher-Yates with the generator's own bits: the same order wherever this is built)
				std::swap(ex.order[k - 1u], ex.order[rng() % k]);
		}
		TeaserSearchOutcome res;
		const int rc = teaser_search_control(ex, P, max_core, budget, res);
		if (rc)
			return rc;
		for (size_t k = 0; k < res.clique.size(); k++)
			clique[k] = (int32_t)keep[res.clique[k]];
		out[0] = res.clique.size(), out[1] = res.nodes, out[2] = res.exact ? 1 : 0, out[4] = res.omega, out[5] = P.n_tasks, out[6] = res.launches, out[7] = m;
		return 0;
	}
}
