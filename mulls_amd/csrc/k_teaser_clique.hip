// k_teaser_clique.hip — the exact maximum-clique search of mulls_coarse_reg_teaser on the device (MULLS_OPT_TEASER_DEVICE_SEARCH) for gfx950.
//   k_teaser_later    a wave per kept vertex: how many kept neighbours lie above it (the plan's input, teaser_search.h)
//   k_teaser_clique   one launch of the search: a wave is a worker; it takes up the task it kept from the launch before or draws ranks from the shared
//                     counter, and walks the task's tree depth-first until it has entered `quota` nodes
//   k_teaser_witness  one wave: the greedy clique of one vertex as a list (what an abandoned search returns)
// teaser_search.h has the scheme, the shared words and a scalar restatement of k_teaser_clique (TeaserScalar::launch) that the CPU tests run; this file
// follows it step by step.  A set of up to 8192 kept vertices is W <= 128 words: lane l holds the words l and l + 64, as k_teaser_greedy does.  The
// stack (one set per depth) and the clique so far live in the worker's slab of global memory; a lane reads back only words it wrote itself.
//
// Between workgroups only monotone words are shared: the task counter (add), the incumbent (max), the lowest rank (min), read with relaxed agent-scope
// loads.  A stale value costs work and changes no result; no wave ever waits for another, and every loop below is bounded by the size of a set, the
// depth of the stack or the quota.
#include <hip/hip_runtime.h>

#include "teaser_launch.h"

namespace
{
constexpr int WAVE = 64;
typedef unsigned long long u64;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
	for (int off = WAVE / 2; off > 0; off >>= 1)
		v += __shfl_xor(v, off, WAVE);
	return v;
}
__device__ __forceinline__ u64 bcast64(u64 x, int l)
{
	const uint32_t lo = __shfl((uint32_t)x, l, WAVE), hi = __shfl((uint32_t)(x >> 32), l, WAVE);
	return (u64)lo | ((u64)hi << 32);
}
__device__ __forceinline__ uint32_t relaxed_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// one lane asks, every lane gets the same answer: the control flow below stays uniform
__device__ __forceinline__ uint32_t shared_word(const uint32_t *p, uint32_t lane)
{
	uint32_t v = 0;
	if (lane == 0)
		v = relaxed_load(p);
	return __shfl(v, 0, WAVE);
}

struct Set
{
	u64 a, b; // words lane and lane + 64
};
__device__ __forceinline__ Set load_row(const uint64_t *rows, uint32_t W, uint32_t v, uint32_t lane)
{
	Set r;
	r.a = lane < W ? rows[(size_t)v * W + lane] : 0ull;
	r.b = lane + WAVE < W ? rows[(size_t)v * W + lane + WAVE] : 0ull;
	return r;
}
__device__ __forceinline__ void store_set(uint64_t *row, uint32_t W, const Set &p, uint32_t lane)
{
	if (lane < W)
		row[lane] = p.a;
	if (lane + WAVE < W)
		row[lane + WAVE] = p.b;
}
__device__ __forceinline__ uint32_t set_count(const Set &p) { return wave_sum((uint32_t)__popcll(p.a) + (uint32_t)__popcll(p.b)); }
// the smallest member; false: the set is empty
__device__ __forceinline__ bool set_lowest(const Set &p, uint32_t *v)
{
	const u64 b0 = __ballot(p.a != 0ull), b1 = __ballot(p.b != 0ull);
	if (!b0 && !b1)
		return false;
	const int l = b0 ? __ffsll((long long)b0) - 1 : __ffsll((long long)b1) - 1;
	const u64 word = bcast64(b0 ? p.a : p.b, l);
	*v = ((b0 ? 0u : (uint32_t)WAVE) + (uint32_t)l) * 64u + (uint32_t)__ffsll((long long)word) - 1u;
	return true;
}
__device__ __forceinline__ void set_remove(Set &p, uint32_t v, uint32_t lane)
{
	const u64 bit = 1ull << (v & 63u);
	if ((v >> 6) == lane)
		p.a &= ~bit;
	if ((v >> 6) == lane + WAVE)
		p.b &= ~bit;
}
// what of the set lies above v
__device__ __forceinline__ void set_keep_above(Set &p, uint32_t v, uint32_t lane)
{
	const uint32_t w = v >> 6;
	const u64 upper = ~((2ull << (v & 63u)) - 1ull);
	p.a = lane < w ? 0ull : (lane == w ? p.a & upper : p.a);
	p.b = lane + WAVE < w ? 0ull : (lane + WAVE == w ? p.b & upper : p.b);
}
__device__ __forceinline__ uint32_t wave_scan(uint32_t c, uint32_t lane) // inclusive
{
#pragma unroll
	for (int off = 1; off < WAVE; off <<= 1)
	{
		const uint32_t t = __shfl_up(c, off, WAVE);
		if (lane >= (uint32_t)off)
			c += t;
	}
	return c;
}
// the k-th member in ascending order (k from 0); false: there are k or fewer
__device__ bool set_kth(const Set &p, uint32_t k, uint32_t lane, uint32_t *v)
{
	const uint32_t ca = (uint32_t)__popcll(p.a), cb = (uint32_t)__popcll(p.b);
	const uint32_t sa = wave_scan(ca, lane), total_a = __shfl(sa, WAVE - 1, WAVE);
	const uint32_t sb = wave_scan(cb, lane) + total_a;
	uint32_t mine = 0xffffffffu;
	if (k >= sa - ca && k < sa)
	{
		u64 w = p.a;
		for (uint32_t j = k - (sa - ca); j; j--) // (fewer than 64 steps)
			w &= w - 1ull;
		mine = lane * 64u + (uint32_t)__ffsll((long long)w) - 1u;
	}
	else if (k >= sb - cb && k < sb)
	{
		u64 w = p.b;
		for (uint32_t j = k - (sb - cb); j; j--)
			w &= w - 1ull;
		mine = (lane + WAVE) * 64u + (uint32_t)__ffsll((long long)w) - 1u;
	}
	const u64 who = __ballot(mine != 0xffffffffu);
	if (!who)
		return false;
	*v = __shfl(mine, __ffsll((long long)who) - 1, WAVE);
	return true;
}
// does a greedy colouring of p need more than `room` colours?  (TeaserSearch::colours_exceed: the classes are built one after the other, each takes the
// smallest vertex left that is adjacent to none of its members)  Every inner step removes a vertex from q: at most |p| steps in all.
__device__ bool colours_exceed(const uint64_t *__restrict__ rows, uint32_t W, const Set &p, uint32_t room, uint32_t lane)
{
	Set q = p;
	for (uint32_t colours = 0;;)
	{
		uint32_t v;
		if (!set_lowest(q, &v))
			return false;
		if (++colours > room)
			return true;
		Set u = q;
		while (set_lowest(u, &v))
		{
			set_remove(q, v, lane);
			set_remove(u, v, lane);
			const Set r = load_row(rows, W, v, lane);
			u.a &= ~r.a, u.b &= ~r.b;
		}
	}
}

__global__ void __launch_bounds__(256) k_teaser_later(const uint64_t *__restrict__ sub, uint32_t m, uint32_t W, uint32_t *__restrict__ later)
{
	const uint32_t v = blockIdx.x * 4u + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
	if (v >= m)
		return;
	Set p = load_row(sub, W, v, lane);
	set_keep_above(p, v, lane);
	const uint32_t c = set_count(p);
	if (lane == 0)
		later[v] = c;
}

__global__ void __launch_bounds__(256) k_teaser_clique(TeaserSearchArgs A)
{
	const uint32_t worker = blockIdx.x * 4u + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
	if (worker >= A.workers)
		return;
	const uint64_t *__restrict__ sub = A.sub;
	const uint32_t W = A.W, levels = A.levels;
	TeaserSearchCtl *ctl = A.ctl;
	TeaserWorkerState *ws = A.state + worker;
	uint64_t *slab = A.slab + (size_t)worker * levels * W;
	uint32_t *cur = A.cur + (size_t)worker * levels;
	uint32_t active = ws->active, rank = ws->rank, depth = ws->depth, base = ws->base, found = ws->found; // (the same words in every lane)
	uint32_t nodes = 0;
	bool saved = false, failed = false;
	Set p = {0ull, 0ull};
	if (active)
		p = load_row(slab, W, depth, lane); // (depth < levels: it was stored from here)
	for (;;)
	{
		if (!active)
		{
			// the next rank; in phase B ranks above the lowest one that succeeded are not started (draws ascend: none below it is left then)
			uint32_t id = MULLS_TEASER_NO_RANK;
			if (lane == 0)
			{
				uint32_t limit = A.n_tasks;
				if (A.phase)
					limit = min(limit, relaxed_load(&ctl->best_rank));
				if (relaxed_load(&ctl->next) < limit) // (the counter stops near the end of the queue: it cannot wrap)
				{
					id = atomicAdd(&ctl->next, 1u);
					if (id >= limit)
						id = MULLS_TEASER_NO_RANK;
				}
			}
			id = __shfl(id, 0, WAVE);
			if (id == MULLS_TEASER_NO_RANK)
				break;
			// root: the last v with first[v] <= id (roots without a task have first[v] == first[v + 1])
			uint32_t lo = 0, hi = A.m; // first[lo] <= id < first[hi]
			while (hi - lo > 1u)	   // (at most 13 steps)
			{
				const uint32_t mid = (lo + hi) / 2u;
				if (A.first[mid] <= id)
					lo = mid;
				else
					hi = mid;
			}
			const uint32_t v = lo, f0 = A.first[v], n_here = A.first[v + 1u] - f0;
			p = load_row(sub, W, v, lane);
			set_keep_above(p, v, lane);
			base = 1;
			if (lane == 0)
				cur[0] = v;
			if (n_here > 1u) // a split root: the child of its (id - f0)-th candidate
			{
				uint32_t c = 0;
				if (!set_kth(p, id - f0, lane, &c))
				{
					failed = true;
					break;
				}
				set_keep_above(p, c, lane);
				const Set r = load_row(sub, W, c, lane);
				p.a &= r.a, p.b &= r.b;
				base = 2;
				if (lane == 0)
					cur[1] = c;
			}
			active = 1, rank = id, depth = base;
		}
		if (nodes >= A.quota) // the task goes on in the next launch
		{
			store_set(slab + (size_t)depth * W, W, p, lane);
			saved = true;
			break;
		}
		nodes++;
		uint32_t goal;
		if (A.phase)
		{
			if (rank > shared_word(&ctl->best_rank, lane))
			{
				active = 0;
				continue;
			}
			goal = A.omega;
			if (depth >= goal) // cur[0 .. omega) is the smallest list with this task's prefix
			{
				if (lane == 0)
					atomicMin(&ctl->best_rank, rank);
				found = rank, active = 0;
				continue;
			}
		}
		else
		{
			goal = shared_word(&ctl->bound, lane) + 1u;
			if (depth >= goal)
			{
				if (lane == 0)
					atomicMax(&ctl->bound, depth);
				goal = depth + 1u;
			}
		}
		uint32_t need = goal - depth;
		bool cut = set_count(p) < need;
		if (!cut && depth + 1u >= levels) // (the plan excludes it: no clique has more than max_core + 1 vertices)
			cut = true, failed = true;
		if (!cut && need >= 2u)
			cut = !colours_exceed(sub, W, p, need - 1u, lane);
		if (cut)
		{
			for (;;) // back to the deepest level that still has enough candidates
			{
				if (depth == base)
				{
					active = 0;
					break;
				}
				depth--;
				p = load_row(slab, W, depth, lane);
				if (!A.phase)
					goal = shared_word(&ctl->bound, lane) + 1u;
				need = goal > depth ? goal - depth : 1u;
				if (set_count(p) >= need)
					break;
			}
			if (!active)
				continue;
		}
		uint32_t v = 0;
		(void)set_lowest(p, &v); // (p is not empty: it has need >= 1 members)
		set_remove(p, v, lane);
		store_set(slab + (size_t)depth * W, W, p, lane); // what is left at this depth are the candidates above v
		if (lane == 0)
			cur[depth] = v;
		const Set r = load_row(sub, W, v, lane);
		p.a &= r.a, p.b &= r.b;
		depth++;
	}
	if (lane == 0)
	{
		ws->active = active, ws->rank = rank, ws->depth = depth, ws->base = base, ws->found = found;
		if (nodes)
			atomicAdd(&ctl->nodes, (u64)nodes);
		if (saved)
			atomicAdd(&ctl->saves, 1u);
		if (failed)
			atomicOr(&ctl->error, 1u);
	}
}

// v, then again and again the smallest vertex adjacent to all members so far (teaser_greedy_clique); out[0] = the count, out[1 ..] = the vertices as taken
__global__ void __launch_bounds__(WAVE) k_teaser_witness(const uint64_t *__restrict__ sub, uint32_t m, uint32_t W, uint32_t v, uint32_t *__restrict__ out)
{
	const uint32_t lane = threadIdx.x;
	Set p = load_row(sub, W, v, lane);
	uint32_t size = 1;
	if (lane == 0)
		out[1] = v;
	for (uint32_t step = 0; step + 1u < m; step++) // (a clique has at most m vertices)
	{
		uint32_t u;
		if (!set_lowest(p, &u))
			break;
		const Set r = load_row(sub, W, u, lane);
		p.a &= r.a, p.b &= r.b;
		if (lane == 0)
			out[1u + size] = u;
		size++;
	}
	if (lane == 0)
		out[0] = size;
}
} // namespace

hipError_t launch_teaser_later(hipStream_t st, const uint64_t *sub, uint32_t m, uint32_t *later)
{
	if (!m || m > MULLS_TEASER_MAX_POINTS)
		return m ? hipErrorInvalidValue : hipSuccess;
	hipLaunchKernelGGL(k_teaser_later, dim3((m + 3u) / 4u), dim3(256), 0, st, sub, m, (m + 63u) / 64u, later);
	return hipGetLastError();
}

hipError_t launch_teaser_clique(hipStream_t st, const TeaserSearchArgs &A)
{
	// two words per lane: W <= 128; a set of the stack is W words, and the binary search needs a root
	if (!A.m || A.m > MULLS_TEASER_MAX_POINTS || A.W != (A.m + 63u) / 64u || !A.workers || A.levels < 2u || !A.quota)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_teaser_clique, dim3((A.workers + 3u) / 4u), dim3(256), 0, st, A);
	return hipGetLastError();
}

hipError_t launch_teaser_witness(hipStream_t st, const uint64_t *sub, uint32_t m, uint32_t v, uint32_t *out)
{
	if (!m || m > MULLS_TEASER_MAX_POINTS || v >= m)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_teaser_witness, dim3(1), dim3(WAVE), 0, st, sub, m, (m + 63u) / 64u, v, out);
	return hipGetLastError();
}
