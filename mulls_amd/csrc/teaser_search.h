// teaser_search.h — the scheme of the device form of mulls_coarse_reg_teaser's exact maximum-clique search (MULLS_OPT_TEASER_DEVICE_SEARCH): the plan
// (which tasks there are), the words the workers share, a scalar restatement of what one worker does in one launch (k_teaser_clique.hip runs the same
// steps with a set spread over the lanes of a wave) and the phase control, written once against an executor: teaser.cpp plugs in the device, and
// tests/teaser_search_harness.cpp a serial executor that runs the tasks in any order.  No HIP in here.  DESIGN.md section 7.4 has the reasoning.
//
// Input: the compacted m x W bit matrix of the kept vertices (ascending original numbers: lexicographic order is the same in both numberings), the
// greedy bound lb (a clique of lb vertices exists) and the largest core number (no clique has more than max_core + 1 vertices).
//
// Tasks are clique prefixes in lexicographic rank order: a root v with the candidates N+(v) = the kept neighbours above v, or, where a root has more
// than MULLS_TEASER_SPLIT_MIN candidates, its depth-2 children (v, u), u the k-th candidate.  A root with fewer than lb - 1 candidates has no task.
// The rule is a function of the graph alone.
//
// Phase A finds the size: a shared incumbent starts at lb, a task is a depth-first branch and bound (cuts: clique + candidates, clique + greedy
// colouring of the candidates — the host search's two) that raises it with an atomic maximum; only the final incumbent, omega, leaves the phase.
// It is skipped where lb == max_core + 1.  Phase B finds the list: every task is a decision search for a clique of omega vertices in ascending
// candidate order; the first it meets is the smallest list with the task's prefix, and the smallest list of all is the one of the lowest rank that
// has any.  A shared word holds the lowest rank that succeeded (atomic minimum); tasks above it are not started, or abandoned.  Task r* is never
// abandoned and its search reads nothing shared, so its list does not depend on who finished first.  A stale read of either word only costs work.
//
// Every launch ends: a worker enters at most `quota` tree nodes per launch and keeps an unfinished task as a stack (one candidate set per depth) for
// the next launch.  Between launches the host reads TeaserSearchCtl and applies the node budget.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "teaser_host.h"

#define MULLS_TEASER_SPLIT_MIN 32u		  // a root with more candidates than this is split into its depth-2 children
#define MULLS_TEASER_SEARCH_QUOTA 256u	  // tree nodes a worker enters per launch (a first value: DESIGN.md section 7.4, "Measured")
#define MULLS_TEASER_SEARCH_WORKERS 2048u // wavefronts of a launch: 8 per CU of an MI355X
#define MULLS_TEASER_SEARCH_STACK_BYTES (256ull << 20) // the workers' stacks together stay below this: where a stack is deep and wide, fewer workers run
#define MULLS_TEASER_NO_RANK 0xffffffffu

// the words the workers share and the host reads back after every launch
struct TeaserSearchCtl
{
	uint32_t next;		// tasks drawn so far (atomic add)
	uint32_t bound;		// phase A: the incumbent (atomic maximum)
	uint32_t best_rank; // phase B: the lowest rank of a task that found a clique of omega vertices (atomic minimum)
	uint32_t saves;		// workers that have left a launch with an unfinished task, over all launches of the phase
	unsigned long long nodes; // tree nodes entered, over all launches of the phase
	uint32_t error;		// a worker met a state the plan excludes (a stack deeper than max_core + 2, a split child that does not exist)
	uint32_t pad;
};
// what a worker keeps between launches, next to its stack (levels x W words) and its clique so far (levels vertices)
struct TeaserWorkerState
{
	uint32_t active, rank, depth, base; // an unfinished task: its rank, the vertices of its clique so far, those of its prefix
	uint32_t found;						// phase B: the rank of the task whose clique of omega vertices this worker's list holds, or MULLS_TEASER_NO_RANK
	uint32_t pad[3];
};

struct TeaserPlan
{
	uint32_t m = 0, W = 0, lb = 0, levels = 0, n_tasks = 0;
	std::vector<uint32_t> first; // m + 1: first[v] = the rank of root v's first task; first[v + 1] - first[v] = 0, 1 (the root) or its candidate count
};
// later[v] = the kept neighbours of v above v
inline void teaser_plan(const uint32_t *later, uint32_t m, uint32_t lb, uint32_t max_core, TeaserPlan &P)
{
	P.m = m, P.W = (m + 63u) / 64u, P.lb = lb, P.levels = max_core + 2u;
	P.first.assign((size_t)m + 1u, 0u);
	uint32_t n = 0; // (at most m (m - 1) / 2 < 2^25)
	for (uint32_t v = 0; v < m; v++)
	{
		P.first[v] = n;
		if (later[v] + 1u >= lb)
			n += later[v] > MULLS_TEASER_SPLIT_MIN ? later[v] : 1u;
	}
	P.first[m] = n, P.n_tasks = n;
}
// workers of a launch: as many as the stacks' memory allows, one at least
inline uint32_t teaser_plan_workers(const TeaserPlan &P)
{
	const unsigned long long per = (unsigned long long)P.levels * P.W * 8u;
	return (uint32_t)std::max<unsigned long long>(1u, std::min<unsigned long long>(MULLS_TEASER_SEARCH_WORKERS, MULLS_TEASER_SEARCH_STACK_BYTES / per));
}

// ---- one worker, one launch, restated for a scalar machine
struct TeaserWorker
{
	TeaserWorkerState s = {0, 0, 0, 0, MULLS_TEASER_NO_RANK, {0, 0, 0}};
	std::vector<uint64_t> slab; // levels x W
	std::vector<uint32_t> cur;	// levels
	std::vector<uint32_t> list; // phase B: the clique of task s.found (a serial executor may hand a worker a lower rank after a higher one: the lower list stays)
	uint32_t own_bound = 0, own_rank = MULLS_TEASER_NO_RANK; // "stale" mode: what this task has seen of the shared words — its own updates only
};

struct TeaserScalar
{
	TeaserBits G;
	const TeaserPlan *P = nullptr;
	TeaserSearchCtl *ctl = nullptr;
	int phase = 0;		// 0: A, 1: B
	uint32_t omega = 0; // phase B's target
	bool stale = false; // a task never sees what another task wrote
	std::vector<uint64_t> p, q, u;

	static uint32_t count(const std::vector<uint64_t> &s)
	{
		uint32_t c = 0;
		for (uint64_t w : s)
			c += (uint32_t)__builtin_popcountll(w);
		return c;
	}
	static bool lowest(const std::vector<uint64_t> &s, uint32_t *v)
	{
		for (size_t w = 0; w < s.size(); w++)
			if (s[w])
			{
				*v = (uint32_t)w * 64u + (uint32_t)__builtin_ctzll(s[w]);
				return true;
			}
		return false;
	}
	static void keep_above(std::vector<uint64_t> &s, uint32_t v)
	{
		for (uint32_t w = 0; w < (v >> 6); w++)
			s[w] = 0;
		s[v >> 6] &= ~((2ull << (v & 63u)) - 1ull);
	}
	// does a greedy colouring of s need more than `room` colours?  (TeaserSearch::colours_exceed)
	bool colours_exceed(const std::vector<uint64_t> &s, uint32_t room)
	{
		q = s;
		for (uint32_t colours = 0;;)
		{
			uint32_t v;
			if (!lowest(q, &v))
				return false;
			if (++colours > room)
				return true;
			u = q;
			while (lowest(u, &v))
			{
				q[v >> 6] &= ~(1ull << (v & 63u));
				u[v >> 6] &= ~(1ull << (v & 63u));
				const uint64_t *r = G.row(v);
				for (uint32_t k = 0; k < G.W; k++)
					u[k] &= ~r[k];
			}
		}
	}
	uint32_t read_bound(const TeaserWorker &w) const { return stale ? w.own_bound : ctl->bound; }
	uint32_t read_rank(const TeaserWorker &w) const { return stale ? w.own_rank : ctl->best_rank; }

	// the task of a rank: its prefix into w.cur, its candidates into p
	bool start(TeaserWorker &w, uint32_t rank)
	{
		const std::vector<uint32_t> &first = P->first;
		const uint32_t v = (uint32_t)(std::upper_bound(first.begin(), first.end(), rank) - first.begin()) - 1u;
		p.assign(G.row(v), G.row(v) + G.W);
		keep_above(p, v);
		w.cur[0] = v, w.s.base = 1;
		if (first[v + 1u] - first[v] > 1u)
		{
			uint32_t c = 0;
			for (uint32_t k = rank - first[v];; k--)
			{
				if (!lowest(p, &c))
					return false;
				if (!k)
					break;
				p[c >> 6] &= ~(1ull << (c & 63u));
			}
			keep_above(p, c);
			const uint64_t *r = G.row(c);
			for (uint32_t k = 0; k < G.W; k++)
				p[k] &= r[k];
			w.cur[1] = c, w.s.base = 2;
		}
		w.s.active = 1, w.s.rank = rank, w.s.depth = w.s.base;
		w.own_bound = P->lb, w.own_rank = MULLS_TEASER_NO_RANK;
		return true;
	}

	// draw: bool(uint32_t *rank), the next task of the queue (false: none is left for this worker in this launch)
	template <class Draw>
	void launch(TeaserWorker &w, uint32_t quota, Draw draw)
	{
		const uint32_t W = G.W, levels = P->levels;
		w.slab.resize((size_t)levels * W), w.cur.resize(levels);
		uint32_t nodes = 0;
		bool saved = false;
		p.assign(W, 0);
		if (w.s.active)
			p.assign(w.slab.begin() + (size_t)w.s.depth * W, w.slab.begin() + (size_t)(w.s.depth + 1u) * W);
		for (;;)
		{
			if (!w.s.active)
			{
				uint32_t rank;
				if (!draw(&rank))
					break;
				if (!start(w, rank))
				{
					ctl->error = 1, w.s.active = 0;
					break;
				}
			}
			uint32_t &depth = w.s.depth;
			if (nodes >= quota) // the task goes on in the next launch
			{
				std::copy(p.begin(), p.end(), w.slab.begin() + (size_t)depth * W);
				saved = true;
				break;
			}
			nodes++;
			uint32_t goal;
			if (phase)
			{
				if (w.s.rank > read_rank(w))
				{
					w.s.active = 0;
					continue;
				}
				goal = omega;
				if (depth >= goal)
				{
					ctl->best_rank = std::min(ctl->best_rank, w.s.rank), w.own_rank = w.s.rank;
					if (w.s.rank < w.s.found)
						w.s.found = w.s.rank, w.list.assign(w.cur.begin(), w.cur.begin() + goal);
					w.s.active = 0;
					continue;
				}
			}
			else
			{
				goal = read_bound(w) + 1u;
				if (depth >= goal)
				{
					ctl->bound = std::max(ctl->bound, depth), w.own_bound = std::max(w.own_bound, depth);
					goal = depth + 1u;
				}
			}
			uint32_t need = goal - depth;
			bool cut = count(p) < need;
			if (!cut && depth + 1u >= levels)
				cut = true, ctl->error = 1;
			if (!cut && need >= 2u)
				cut = !colours_exceed(p, need - 1u);
			if (cut)
			{
				for (;;) // back to the deepest level that still has enough candidates
				{
					if (depth == w.s.base)
					{
						w.s.active = 0;
						break;
					}
					depth--;
					p.assign(w.slab.begin() + (size_t)depth * W, w.slab.begin() + (size_t)(depth + 1u) * W);
					if (!phase)
						goal = read_bound(w) + 1u;
					need = goal > depth ? goal - depth : 1u;
					if (count(p) >= need)
						break;
				}
				if (!w.s.active)
					continue;
			}
			uint32_t v = 0;
			lowest(p, &v); // (p is not empty: count(p) >= need >= 1)
			p[v >> 6] &= ~(1ull << (v & 63u));
			std::copy(p.begin(), p.end(), w.slab.begin() + (size_t)depth * W); // what is left at this depth are the candidates above v
			w.cur[depth] = v;
			const uint64_t *r = G.row(v);
			for (uint32_t k = 0; k < W; k++)
				p[k] &= r[k];
			depth++;
		}
		ctl->nodes += nodes;
		ctl->saves += saved ? 1u : 0u;
	}
};

// ---- the phase control
// Exec:  int begin(int phase, uint32_t bound)             reset the queue, the workers and the shared words (phase A: the incumbent = bound; B: omega = bound)
//        int launch(TeaserSearchCtl *ctl)                 one launch, then the shared words
//        int clique(uint32_t rank, std::vector<uint32_t> *out)   the list the worker that finished task `rank` holds (kept numbering, ascending)
//        int witness(std::vector<uint32_t> *out)          the greedy bound's witness: teaser_greedy_clique of the vertex that gave lb
// each returns 0 or an error code that the control passes on
struct TeaserSearchOutcome
{
	std::vector<uint32_t> clique; // kept numbering, ascending
	unsigned long long nodes = 0;
	uint32_t omega = 0, launches = 0;
	bool exact = false;
};
#define MULLS_TEASER_SEARCH_FAILED (-1) // the shared words report a state the plan excludes

template <class Exec>
int teaser_search_control(Exec &ex, const TeaserPlan &P, uint32_t max_core, unsigned long long budget, TeaserSearchOutcome &out)
{
	out = TeaserSearchOutcome();
	out.omega = P.lb;
	unsigned long long before = 0;
	TeaserSearchCtl ctl = {};
	bool abandoned = false;
	for (int phase = P.lb == max_core + 1u ? 1 : 0; phase < 2 && !abandoned; phase++)
	{
		if (int rc = ex.begin(phase, out.omega))
			return rc;
		for (uint32_t saves = 0;;)
		{
			if (int rc = ex.launch(&ctl))
				return rc;
			out.launches++;
			out.nodes = before + ctl.nodes;
			if (ctl.error)
				return MULLS_TEASER_SEARCH_FAILED;
			if (out.nodes > budget)
			{
				abandoned = true;
				break;
			}
			if (ctl.saves == saves) // every worker left because the queue had nothing for it
				break;
			saves = ctl.saves;
		}
		before = out.nodes;
		if (!phase)
			out.omega = ctl.bound;
	}
	if (abandoned)
	{
		out.omega = P.lb;
		return ex.witness(&out.clique);
	}
	if (ctl.best_rank == MULLS_TEASER_NO_RANK)
		return MULLS_TEASER_SEARCH_FAILED; // (a clique of omega vertices exists: phase A met one, or the witness is one)
	out.exact = true;
	return ex.clique(ctl.best_rank, &out.clique);
}
