// k_teaser.hip — the TEASER coarse-registration solver (CRegistration::coarse_reg_teaser, cregistration.hpp:664-759) for gfx950.  Every step is written
// once, as a __device__ function over resolved pointers and sizes (teaser_graph ... teaser_update below), and launched through two thin kernels:
//   k_teaser_*   one problem per call (mulls_coarse_reg_teaser, _indexed): pointers and sizes are launch arguments
//   k_tb_*       the problems of one sub-batch per launch (mulls_coarse_reg_teaser_batch): they come from the descriptor table of teaser_batch.h (a
//                problem's n, W, m, C and the offsets of its arrays in the arena), and the problem is a grid axis — blockIdx.y (blockIdx.z for the
//                graph, blockIdx.x for the single-workgroup steps); every loop is bounded by that problem's own sizes, so a block beyond them leaves at once
// (a single call run through the k_tb_* kernels as a batch of one measured 1 to 2 % slower — profiles/teaser_kernel_stats.txt, section 5; the descriptor
// read in front of every step is the supposed cause, not an isolated one — which is why the single call keeps launch arguments.)  The steps:
//   graph    the pair-consistency graph as a bit matrix: a wave tests 64 consecutive j against one i and stores the ballot word
//   degrees  a wave per row: popcounts
//   cores    one workgroup: core numbers by peeling in rounds (alive set and degrees in LDS, a wave per leaving vertex lowers its neighbours')
//   greedy   a wave per vertex: the clique grown by taking the smallest common neighbour — the lower bound of the exact search
//   compact  the sub-matrix of the vertices that can still belong to a maximum clique
//   pick     the clique's points
//   fit_part / fit, cost_part / cost, update   one GNC-TLS iteration over the clique's pairwise measurements
// Every double expression is written in the order include/mulls_hip.h and DESIGN.md section 7.4 define (built with -ffp-contract=off); the shared
// arithmetic is teaser_math.h, which the CPU harness compiles too: tests/teaser_restated.py reproduces the bits.  Each problem has its own partial sums
// and its own TeaserGnc record, so every sum has the order of the definition per problem.
//   GNC of a sub-batch, lock-step: iteration `iter` is one launch set for all problems.  A problem whose record carries stop != 0 from an EARLIER iteration
//   is skipped by every kernel (a test on the record, uniform per workgroup): k_tb_cost, the first kernel that may change the word, marks such a problem
//   in frozen[], which is what lets k_tb_update tell "stopped before" (skip) from "the cost settled in this iteration" (stop == 2: the update still runs,
//   as in the single call, which breaks after it).  A problem with C < 2 never enters.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "teaser_launch.h"

namespace
{
constexpr int WAVE = 64;
constexpr uint32_t P = MULLS_TEASER_PARTIALS;
constexpr int RT = 1024; // threads of the single-workgroup kernels
static_assert(P == 4u * RT, "the reductions fold four partials per thread before the LDS tree");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
	for (int off = WAVE / 2; off > 0; off >>= 1)
		v += __shfl_xor(v, off, WAVE);
	return v;
}

// measurement k: a = s[c_b] - s[c_a], b = t[c_b] - t[c_a], widened first
__device__ __forceinline__ void measurement(const float4 *cs, const float4 *ct, uint32_t C, uint64_t k, double *a, double *b)
{
	uint32_t ia, ib;
	teaser_decode(k, C, &ia, &ib);
	const float4 s0 = cs[ia], s1 = cs[ib], t0 = ct[ia], t1 = ct[ib];
	a[0] = (double)s1.x - (double)s0.x, a[1] = (double)s1.y - (double)s0.y, a[2] = (double)s1.z - (double)s0.z;
	b[0] = (double)t1.x - (double)t0.x, b[1] = (double)t1.y - (double)t0.y, b[2] = (double)t1.z - (double)t0.z;
}

// the pairwise tree over P partials: p[t] += p[t + s], s = P / 2, ..., 1 — the two widest levels in registers, the rest in LDS
__device__ double tree_sum(const double *part, double *red)
{
	const int t = threadIdx.x;
	const double v = (part[t] + part[t + 2 * RT]) + (part[t + RT] + part[t + 3 * RT]);
	__syncthreads(); // (red may still be read by the previous sum)
	red[t] = v;
	__syncthreads();
	for (int s = RT / 2; s > 0; s >>= 1)
	{
		if (t < s)
			red[t] = red[t] + red[t + s];
		__syncthreads();
	}
	return red[0];
}

// ---- the steps: one text for both kernel families
__device__ __forceinline__ void teaser_graph(const float4 *src, const float4 *tgt, uint32_t n, uint32_t W, double beta, uint64_t *adj)
{
	__shared__ float4 si[WAVE], ti[WAVE];
	const uint32_t i0 = blockIdx.y * WAVE, j = blockIdx.x * 256u + threadIdx.x;
	const uint32_t lane = threadIdx.x % WAVE, word = blockIdx.x * 4u + threadIdx.x / WAVE;
	if (threadIdx.x < WAVE)
	{
		const uint32_t i = i0 + threadIdx.x;
		si[threadIdx.x] = i < n ? src[i] : make_float4(0, 0, 0, 0);
		ti[threadIdx.x] = i < n ? tgt[i] : make_float4(0, 0, 0, 0);
	}
	__syncthreads();
	if (word >= W)
		return;
	float sj[3] = {0, 0, 0}, tj[3] = {0, 0, 0};
	if (j < n)
	{
		const float4 a = src[j], b = tgt[j];
		sj[0] = a.x, sj[1] = a.y, sj[2] = a.z;
		tj[0] = b.x, tj[1] = b.y, tj[2] = b.z;
	}
	const uint32_t rows = min((uint32_t)WAVE, n - i0); // (i0 < n: blockIdx.y < W)
	for (uint32_t r = 0; r < rows; r++)
	{
		const uint32_t i = i0 + r;
		const float a[3] = {si[r].x, si[r].y, si[r].z}, b[3] = {ti[r].x, ti[r].y, ti[r].z};
		const bool e = j < n && j != i && teaser_edge(a, b, sj, tj, beta);
		const unsigned long long bits = __ballot(e);
		if (lane == 0)
			adj[(size_t)i * W + word] = bits;
	}
}

__device__ __forceinline__ void teaser_degrees(const uint64_t *adj, uint32_t n, uint32_t W, uint32_t *deg, unsigned long long *deg_sum)
{
	const uint32_t i = blockIdx.x * 4u + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
	if (i >= n)
		return;
	uint32_t c = 0;
	for (uint32_t w = lane; w < W; w += WAVE)
		c += (uint32_t)__popcll(adj[(size_t)i * W + w]);
	c = wave_sum(c);
	if (lane == 0)
	{
		deg[i] = c;
		if (c)
			atomicAdd(deg_sum, (unsigned long long)c);
	}
}

// Peeling: at level k every alive vertex of degree <= k leaves with core number k, and the waves take the leavers' rows and lower the degrees of their
// alive neighbours (degrees in LDS); a round that removes nothing raises k to the smallest alive degree.  Every round removes a vertex or raises k, and k
// stays below n: at most 2 n + 2 rounds.  Every row is read once.  SWEEP: the words of the LDS sets that are swept — all 128 in the single call, the
// problem's own W (SWEEP = 0) in a sub-batch (integers: the core numbers do not depend on it).  50 KB of LDS and 1024 threads: two workgroups per CU, by the wave slots (2 x 16 of the 32 a
// CU holds) before the LDS (which has room for three: 3 x 50 of 160 KB), so sizing the arrays to a sub-batch's largest n would not raise the residency.
template <uint32_t SWEEP>
__device__ __forceinline__ void teaser_cores(const uint64_t *adj, uint32_t n, uint32_t W, const uint32_t *deg, uint32_t *core)
{
	__shared__ unsigned long long alive[MULLS_TEASER_MAX_POINTS / 64];
	__shared__ uint32_t gone[MULLS_TEASER_MAX_POINTS / 32];
	__shared__ uint32_t cur[MULLS_TEASER_MAX_POINTS];
	__shared__ uint16_t leavers[MULLS_TEASER_MAX_POINTS];
	__shared__ uint32_t sh_removed, sh_alive, sh_min;
	const uint32_t t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
	const uint32_t words = SWEEP ? SWEEP : W;
	for (uint32_t w = t; w < words; w += RT)
	{
		const uint32_t lo = w * 64u;
		alive[w] = lo + 64u <= n ? ~0ull : (!SWEEP || lo < n ? (1ull << (n - lo)) - 1ull : 0ull); // (SWEEP = 0: w < W, so lo < n)
	}
	for (uint32_t v = t; v < n; v += RT)
		cur[v] = deg[v];
	uint32_t k = 0;
	__syncthreads();
	for (uint32_t round = 0; round < 2u * n + 2u; round++)
	{
		for (uint32_t w = t; w < 2u * words; w += RT)
			gone[w] = 0;
		if (t == 0)
			sh_removed = 0, sh_alive = 0, sh_min = 0xffffffffu;
		__syncthreads();
		uint32_t left = 0, lowest = 0xffffffffu;
		for (uint32_t v = t; v < n; v += RT)
			if ((alive[v >> 6] >> (v & 63u)) & 1ull)
			{
				const uint32_t d = cur[v];
				if (d <= k)
				{
					core[v] = k;
					atomicOr(&gone[v >> 5], 1u << (v & 31u));
					leavers[atomicAdd(&sh_removed, 1u)] = (uint16_t)v; // (at most n <= 8192 entries: a vertex leaves once)
				}
				else
					left++, lowest = min(lowest, d);
			}
		if (left)
			atomicAdd(&sh_alive, left), atomicMin(&sh_min, lowest);
		__syncthreads();
		const uint32_t n_removed = sh_removed, n_alive = sh_alive, lowest_alive = sh_min;
		if (n_alive == 0)
			break; // (uniform: read after the barrier)
		if (n_removed == 0)
		{
			k = lowest_alive;
			__syncthreads(); // (the counters are reset at the top of the next round)
			continue;
		}
		if (t < words)
			alive[t] &= ~((unsigned long long)gone[2u * t] | ((unsigned long long)gone[2u * t + 1u] << 32));
		__syncthreads();
		for (uint32_t r = wave; r < n_removed; r += RT / WAVE)
		{
			const uint32_t v = leavers[r];
			for (uint32_t w = lane; w < W; w += WAVE)
			{
				unsigned long long bits = adj[(size_t)v * W + w] & alive[w];
				for (int b = 0; b < 64 && bits; b++) // (one step per set bit)
				{
					atomicSub(&cur[w * 64u + (uint32_t)__ffsll((long long)bits) - 1u], 1u);
					bits &= bits - 1ull;
				}
			}
		}
		__syncthreads();
	}
}

__device__ __forceinline__ void teaser_greedy(const uint64_t *adj, uint32_t n, uint32_t W, uint32_t *greedy)
{
	const uint32_t v = blockIdx.x * 4u + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
	if (v >= n)
		return;
	// the candidates: W <= 128 words, two per lane
	unsigned long long p0 = lane < W ? adj[(size_t)v * W + lane] : 0ull, p1 = lane + WAVE < W ? adj[(size_t)v * W + lane + WAVE] : 0ull;
	uint32_t size = 1;
	for (uint32_t step = 0; step < n; step++)
	{
		const unsigned long long b0 = __ballot(p0 != 0ull), b1 = __ballot(p1 != 0ull);
		if (!b0 && !b1)
			break;
		const int l = b0 ? __ffsll(b0) - 1 : __ffsll(b1) - 1;
		const uint32_t lo = __shfl((uint32_t)(b0 ? p0 : p1), l, WAVE), hi = __shfl((uint32_t)((b0 ? p0 : p1) >> 32), l, WAVE);
		const uint32_t bit = lo ? (uint32_t)__ffs(lo) - 1u : 32u + (uint32_t)__ffs(hi) - 1u;
		const uint32_t u = ((b0 ? 0u : (uint32_t)WAVE) + (uint32_t)l) * 64u + bit; // (< n: the graph kernel sets no bit at or above n)
		p0 &= lane < W ? adj[(size_t)u * W + lane] : 0ull; // (row u has no bit u: u leaves the candidates)
		p1 &= lane + WAVE < W ? adj[(size_t)u * W + lane + WAVE] : 0ull;
		size++;
	}
	if (lane == 0)
		greedy[v] = size;
}

// (m > 0)
__device__ __forceinline__ void teaser_compact(const uint64_t *adj, uint32_t W, const int32_t *keep, uint32_t m, uint32_t Wm, uint64_t *sub)
{
	const uint32_t id = blockIdx.x * 4u + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
	if (id / Wm >= m)
		return;
	const uint32_t r = id / Wm, w = id % Wm;
	const uint32_t c = w * 64u + lane;
	bool e = false;
	if (c < m)
	{
		const uint32_t j = (uint32_t)keep[c];
		e = (adj[(size_t)keep[r] * W + (j >> 6)] >> (j & 63u)) & 1ull;
	}
	const unsigned long long bits = __ballot(e);
	if (lane == 0)
		sub[(size_t)r * Wm + w] = bits;
}

__device__ __forceinline__ void teaser_pick(const float4 *src, const float4 *tgt, const int32_t *clique, uint32_t C, float4 *cs, float4 *ct)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= C)
		return;
	cs[k] = src[clique[k]]; // (the host made the list from vertex numbers below n)
	ct[k] = tgt[clique[k]];
}

// partial p adds the measurements p, p + P, ... in ascending order
__device__ __forceinline__ void teaser_fit_part(const float4 *cs, const float4 *ct, uint32_t C, uint64_t M, int first, const double *weights, double *part)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // the grid's x is exactly P threads
	double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	for (uint64_t k = p; k < M; k += P)
	{
		double a[3], b[3];
		measurement(cs, ct, C, k, a, b);
		const double w = first ? 1.0 : weights[k];
#pragma unroll
		for (int r = 0; r < 3; r++)
#pragma unroll
			for (int c = 0; c < 3; c++)
				h[r * 3 + c] = h[r * 3 + c] + (w * a[r]) * b[c];
	}
#pragma unroll
	for (int q = 0; q < 9; q++)
		part[(size_t)q * P + p] = h[q];
}

__device__ __forceinline__ void teaser_fit(const double *part, int iter, TeaserGnc *S)
{
	__shared__ double red[RT];
	double H[9];
	for (int q = 0; q < 9; q++)
		H[q] = tree_sum(part + (size_t)q * P, red);
	if (threadIdx.x == 0)
	{
		if (iter > 0)
			teaser_gnc_next(S);
		teaser_horn_rot(H, S->R);
	}
}

__device__ __forceinline__ void teaser_cost_part(const float4 *cs, const float4 *ct, uint32_t C, uint64_t M, int first, const double *weights, const TeaserGnc *S,
												 double *part)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	double R[9];
#pragma unroll
	for (int q = 0; q < 9; q++)
		R[q] = S->R[q];
	double cost = 0.0, mx = 0.0;
	for (uint64_t k = p; k < M; k += P)
	{
		double a[3], b[3];
		measurement(cs, ct, C, k, a, b);
		const double r = teaser_resid(R, a, b), w = first ? 1.0 : weights[k];
		cost = cost + w * r;
		if (r > mx)
			mx = r;
	}
	part[p] = cost;
	part[(size_t)P + p] = mx;
}

__device__ __forceinline__ void teaser_cost(const double *part, int iter, double nb2, TeaserGnc *S)
{
	__shared__ double red[RT];
	const int t = threadIdx.x;
	const double cost = tree_sum(part, red);
	const double *mxp = part + P;
	const double m4 = fmax(fmax(mxp[t], mxp[t + RT]), fmax(mxp[t + 2 * RT], mxp[t + 3 * RT])); // (a maximum of finite numbers: no order to define)
	__syncthreads();
	red[t] = m4;
	__syncthreads();
	for (int s = RT / 2; s > 0; s >>= 1)
	{
		if (t < s)
			red[t] = fmax(red[t], red[t + s]);
		__syncthreads();
	}
	if (t == 0)
	{
		teaser_gnc_decide(S, iter, cost, red[0], nb2);
		S->n_inlier = 0;
	}
}

// first, stride: the kernel's global thread number and thread count
__device__ __forceinline__ void teaser_update(const float4 *cs, const float4 *ct, uint32_t C, uint64_t M, double nb2, double *weights, TeaserGnc *S, uint64_t first,
											  uint64_t stride)
{
	if (S->stop == 1u) // mu <= 0 in iteration 0: the weights stay 1 (the host counts M inliers)
		return;
	double R[9];
#pragma unroll
	for (int q = 0; q < 9; q++)
		R[q] = S->R[q];
	const double mu = S->mu;
	uint32_t mine = 0;
	for (uint64_t k = first; k < M; k += stride)
	{
		double a[3], b[3];
		measurement(cs, ct, C, k, a, b);
		const double w = teaser_weight(teaser_resid(R, a, b), mu, nb2);
		weights[k] = w;
		mine += w >= 0.5 ? 1u : 0u;
	}
	mine = wave_sum(mine);
	if (threadIdx.x % WAVE == 0 && mine)
		atomicAdd(&S->n_inlier, mine);
}

// ---- one problem per call: pointers and sizes are launch arguments
__global__ void __launch_bounds__(256) k_teaser_graph(const float4 *__restrict__ src, const float4 *__restrict__ tgt, uint32_t n, uint32_t W, double beta,
													   uint64_t *__restrict__ adj)
{
	teaser_graph(src, tgt, n, W, beta, adj); // (the grid has ceil(n / 64) rows of blocks)
}

__global__ void __launch_bounds__(256) k_teaser_degrees(const uint64_t *__restrict__ adj, uint32_t n, uint32_t W, uint32_t *__restrict__ deg,
														 unsigned long long *deg_sum)
{
	teaser_degrees(adj, n, W, deg, deg_sum);
}

__global__ void __launch_bounds__(RT) k_teaser_cores(const uint64_t *__restrict__ adj, uint32_t n, uint32_t W, const uint32_t *__restrict__ deg,
													  uint32_t *__restrict__ core)
{
	teaser_cores<MULLS_TEASER_MAX_POINTS / 64>(adj, n, W, deg, core); // (n <= MULLS_TEASER_MAX_POINTS: the launcher refuses more)
}

__global__ void __launch_bounds__(256) k_teaser_greedy(const uint64_t *__restrict__ adj, uint32_t n, uint32_t W, uint32_t *__restrict__ greedy)
{
	teaser_greedy(adj, n, W, greedy);
}

__global__ void __launch_bounds__(256) k_teaser_compact(const uint64_t *__restrict__ adj, uint32_t W, const int32_t *__restrict__ keep, uint32_t m, uint32_t Wm,
														 uint64_t *__restrict__ sub)
{
	teaser_compact(adj, W, keep, m, Wm, sub);
}

__global__ void __launch_bounds__(256) k_teaser_pick(const float4 *src, const float4 *tgt, const int32_t *clique, uint32_t C, float4 *cs, float4 *ct)
{
	teaser_pick(src, tgt, clique, C, cs, ct);
}

__global__ void __launch_bounds__(256) k_teaser_fit_part(const float4 *__restrict__ cs, const float4 *__restrict__ ct, uint32_t C, uint64_t M, int first,
														  const double *__restrict__ weights, double *__restrict__ part)
{
	teaser_fit_part(cs, ct, C, M, first, weights, part);
}

__global__ void __launch_bounds__(RT) k_teaser_fit(const double *__restrict__ part, int iter, TeaserGnc *S)
{
	teaser_fit(part, iter, S);
}

__global__ void __launch_bounds__(256) k_teaser_cost_part(const float4 *__restrict__ cs, const float4 *__restrict__ ct, uint32_t C, uint64_t M, int first,
														   const double *__restrict__ weights, const TeaserGnc *__restrict__ S, double *__restrict__ part)
{
	teaser_cost_part(cs, ct, C, M, first, weights, S, part);
}

__global__ void __launch_bounds__(RT) k_teaser_cost(const double *__restrict__ part, int iter, double nb2, TeaserGnc *S)
{
	teaser_cost(part, iter, nb2, S);
}

__global__ void __launch_bounds__(256) k_teaser_update(const float4 *__restrict__ cs, const float4 *__restrict__ ct, uint32_t C, uint64_t M, double nb2,
														double *__restrict__ weights, TeaserGnc *S)
{
	teaser_update(cs, ct, C, M, nb2, weights, S, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
}

// ---- the problems of one sub-batch per launch: pointers and sizes come from the descriptor table
template <typename T>
__device__ __forceinline__ T *at(unsigned char *arena, uint64_t off)
{
	return reinterpret_cast<T *>(arena + off);
}

__global__ void __launch_bounds__(256) k_tb_graph(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, double beta)
{
	const TeaserBatchDesc &D = desc[blockIdx.z];
	if (blockIdx.y >= D.W || blockIdx.x * 4u >= D.W) // (uniform: the grid is sized for the largest problem)
		return;
	teaser_graph(at<const float4>(arena, D.src), at<const float4>(arena, D.tgt), D.n, D.W, beta, at<uint64_t>(arena, D.adj));
}

__global__ void __launch_bounds__(256) k_tb_degrees(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, unsigned long long *deg_sum)
{
	const TeaserBatchDesc &D = desc[blockIdx.y];
	teaser_degrees(at<const uint64_t>(arena, D.adj), D.n, D.W, at<uint32_t>(arena, D.deg), &deg_sum[blockIdx.y]);
}

__global__ void __launch_bounds__(RT) k_tb_cores(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena)
{
	const TeaserBatchDesc &D = desc[blockIdx.x]; // (n <= MULLS_TEASER_MAX_POINTS: the host refuses more)
	teaser_cores<0>(at<const uint64_t>(arena, D.adj), D.n, D.W, at<const uint32_t>(arena, D.deg), at<uint32_t>(arena, D.core));
}

__global__ void __launch_bounds__(256) k_tb_greedy(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena)
{
	const TeaserBatchDesc &D = desc[blockIdx.y];
	teaser_greedy(at<const uint64_t>(arena, D.adj), D.n, D.W, at<uint32_t>(arena, D.core) + D.n); // the greedy sizes lie behind the core numbers
}

__global__ void __launch_bounds__(256) k_tb_compact(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena)
{
	const TeaserBatchDesc &D = desc[blockIdx.y];
	if (D.m) // (m = 0: a graph without an edge, nothing to search)
		teaser_compact(at<const uint64_t>(arena, D.adj), D.W, at<const int32_t>(arena, D.keep), D.m, D.Wm, at<uint64_t>(arena, D.sub));
}

__global__ void __launch_bounds__(256) k_tb_pick(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena)
{
	const TeaserBatchDesc &D = desc[blockIdx.y];
	teaser_pick(at<const float4>(arena, D.src), at<const float4>(arena, D.tgt), at<const int32_t>(arena, D.keep), D.C, at<float4>(arena, D.cs), at<float4>(arena, D.ct));
}

// GNC: problem first + blockIdx.y (blockIdx.x in the single-workgroup kernels)
__device__ __forceinline__ bool enters(const TeaserBatchDesc &D, const TeaserGnc *S, int iter)
{
	return D.C >= 2u && (iter == 0 || S->stop == 0u); // (iteration 0 writes every field of the record: nothing of an earlier call is read)
}

__global__ void __launch_bounds__(256) k_tb_fit_part(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, unsigned char *warena, const TeaserGnc *gnc,
													  uint32_t first_problem, int iter)
{
	const uint32_t pb = first_problem + blockIdx.y;
	const TeaserBatchDesc &D = desc[pb];
	if (enters(D, &gnc[pb], iter))
		teaser_fit_part(at<const float4>(arena, D.cs), at<const float4>(arena, D.ct), D.C, D.M, iter == 0, at<const double>(warena, D.weights), at<double>(arena, D.part));
}

__global__ void __launch_bounds__(RT) k_tb_fit(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, TeaserGnc *gnc, uint32_t first_problem, int iter)
{
	const uint32_t pb = first_problem + blockIdx.x;
	const TeaserBatchDesc &D = desc[pb];
	if (enters(D, &gnc[pb], iter))
		teaser_fit(at<const double>(arena, D.part), iter, &gnc[pb]);
}

__global__ void __launch_bounds__(256) k_tb_cost_part(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, unsigned char *warena, const TeaserGnc *gnc,
													   uint32_t first_problem, int iter)
{
	const uint32_t pb = first_problem + blockIdx.y;
	const TeaserBatchDesc &D = desc[pb];
	if (enters(D, &gnc[pb], iter))
		teaser_cost_part(at<const float4>(arena, D.cs), at<const float4>(arena, D.ct), D.C, D.M, iter == 0, at<const double>(warena, D.weights), &gnc[pb],
						 at<double>(arena, D.part));
}

__global__ void __launch_bounds__(RT) k_tb_cost(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, TeaserGnc *gnc, uint32_t *frozen,
												 uint32_t first_problem, int iter, double nb2)
{
	const uint32_t pb = first_problem + blockIdx.x;
	const TeaserBatchDesc &D = desc[pb];
	if (!enters(D, &gnc[pb], iter)) // (every thread reads the word here; thread 0 writes it behind the barriers of the sums)
	{
		if (threadIdx.x == 0)
			frozen[pb] = 1u; // stopped in an earlier iteration (or never entered): k_tb_update leaves the weights and the count alone
		return;
	}
	teaser_cost(at<const double>(arena, D.part), iter, nb2, &gnc[pb]);
}

__global__ void __launch_bounds__(256) k_tb_update(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, unsigned char *warena, TeaserGnc *gnc,
													const uint32_t *__restrict__ frozen, uint32_t first_problem, double nb2)
{
	const uint32_t pb = first_problem + blockIdx.y;
	const TeaserBatchDesc &D = desc[pb];
	if (!frozen[pb])
		teaser_update(at<const float4>(arena, D.cs), at<const float4>(arena, D.ct), D.C, D.M, nb2, at<double>(warena, D.weights), &gnc[pb],
					  (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
}
} // namespace

hipError_t launch_teaser_graph(hipStream_t st, const float4 *src, const float4 *tgt, uint32_t n, double beta, uint64_t *adj)
{
	if (!n)
		return hipSuccess;
	const uint32_t W = (n + 63u) / 64u;
	hipLaunchKernelGGL(k_teaser_graph, dim3((n + 255u) / 256u, W), dim3(256), 0, st, src, tgt, n, W, beta, adj);
	return hipGetLastError();
}

hipError_t launch_teaser_degrees(hipStream_t st, const uint64_t *adj, uint32_t n, uint32_t *deg, unsigned long long *deg_sum)
{
	if (!n)
		return hipSuccess;
	hipLaunchKernelGGL(k_teaser_degrees, dim3((n + 3u) / 4u), dim3(256), 0, st, adj, n, (n + 63u) / 64u, deg, deg_sum);
	return hipGetLastError();
}

hipError_t launch_teaser_cores(hipStream_t st, const uint64_t *adj, uint32_t n, const uint32_t *deg, uint32_t *core)
{
	if (!n || n > MULLS_TEASER_MAX_POINTS)
		return n ? hipErrorInvalidValue : hipSuccess;
	hipLaunchKernelGGL(k_teaser_cores, dim3(1), dim3(RT), 0, st, adj, n, (n + 63u) / 64u, deg, core);
	return hipGetLastError();
}

hipError_t launch_teaser_greedy(hipStream_t st, const uint64_t *adj, uint32_t n, uint32_t *greedy)
{
	if (!n || n > MULLS_TEASER_MAX_POINTS) // (two words per lane: W <= 128)
		return n ? hipErrorInvalidValue : hipSuccess;
	hipLaunchKernelGGL(k_teaser_greedy, dim3((n + 3u) / 4u), dim3(256), 0, st, adj, n, (n + 63u) / 64u, greedy);
	return hipGetLastError();
}

hipError_t launch_teaser_compact(hipStream_t st, const uint64_t *adj, uint32_t n, const int32_t *keep, uint32_t m, uint64_t *sub)
{
	if (!m)
		return hipSuccess;
	const uint32_t Wm = (m + 63u) / 64u;
	hipLaunchKernelGGL(k_teaser_compact, dim3((m * Wm + 3u) / 4u), dim3(256), 0, st, adj, (n + 63u) / 64u, keep, m, Wm, sub);
	return hipGetLastError();
}

hipError_t launch_teaser_pick(hipStream_t st, const float4 *src, const float4 *tgt, const int32_t *clique, uint32_t C, float4 *cs, float4 *ct)
{
	if (!C)
		return hipSuccess;
	hipLaunchKernelGGL(k_teaser_pick, dim3((C + 255u) / 256u), dim3(256), 0, st, src, tgt, clique, C, cs, ct);
	return hipGetLastError();
}

hipError_t launch_teaser_gnc_iteration(hipStream_t st, const float4 *cs, const float4 *ct, uint32_t C, int iter, double nb2, double *weights, double *part,
									   TeaserGnc *S)
{
	if (C < 2u || C > MULLS_TEASER_MAX_POINTS)
		return hipErrorInvalidValue;
	const uint64_t M = (uint64_t)C * (C - 1u) / 2u;
	const int first = iter == 0;
	hipLaunchKernelGGL(k_teaser_fit_part, dim3(P / 256u), dim3(256), 0, st, cs, ct, C, M, first, weights, part);
	hipLaunchKernelGGL(k_teaser_fit, dim3(1), dim3(RT), 0, st, part, iter, S);
	hipLaunchKernelGGL(k_teaser_cost_part, dim3(P / 256u), dim3(256), 0, st, cs, ct, C, M, first, weights, S, part);
	hipLaunchKernelGGL(k_teaser_cost, dim3(1), dim3(RT), 0, st, part, iter, nb2, S);
	const uint32_t blocks = (uint32_t)std::min<uint64_t>((M + 255u) / 256u, 4096u);
	hipLaunchKernelGGL(k_teaser_update, dim3(blocks), dim3(256), 0, st, cs, ct, C, M, nb2, weights, S);
	return hipGetLastError();
}

hipError_t launch_teaser_batch_graph(hipStream_t st, const TeaserBatchDesc *desc, uint32_t B, uint32_t n_max, unsigned char *arena, double beta,
									 unsigned long long *deg_sum)
{
	if (!B || !n_max || n_max > MULLS_TEASER_MAX_POINTS)
		return B && n_max ? hipErrorInvalidValue : hipSuccess;
	const uint32_t W = (n_max + 63u) / 64u;
	hipLaunchKernelGGL(k_tb_graph, dim3((n_max + 255u) / 256u, W, B), dim3(256), 0, st, desc, arena, beta);
	hipLaunchKernelGGL(k_tb_degrees, dim3((n_max + 3u) / 4u, B), dim3(256), 0, st, desc, arena, deg_sum);
	hipLaunchKernelGGL(k_tb_cores, dim3(B), dim3(RT), 0, st, desc, arena);
	hipLaunchKernelGGL(k_tb_greedy, dim3((n_max + 3u) / 4u, B), dim3(256), 0, st, desc, arena);
	return hipGetLastError();
}

hipError_t launch_teaser_batch_compact(hipStream_t st, const TeaserBatchDesc *desc, uint32_t B, uint64_t words_max, unsigned char *arena)
{
	if (!B || !words_max)
		return hipSuccess;
	hipLaunchKernelGGL(k_tb_compact, dim3((uint32_t)((words_max + 3u) / 4u), B), dim3(256), 0, st, desc, arena);
	return hipGetLastError();
}

hipError_t launch_teaser_batch_pick(hipStream_t st, const TeaserBatchDesc *desc, uint32_t B, uint32_t C_max, unsigned char *arena)
{
	if (!B || !C_max)
		return hipSuccess;
	hipLaunchKernelGGL(k_tb_pick, dim3((C_max + 255u) / 256u, B), dim3(256), 0, st, desc, arena);
	return hipGetLastError();
}

hipError_t launch_teaser_batch_gnc_iteration(hipStream_t st, const TeaserBatchDesc *desc, uint32_t first, uint32_t count, uint64_t M_max, int iter, double nb2,
											 unsigned char *arena, unsigned char *weights, TeaserGnc *gnc, uint32_t *frozen)
{
	if (!count || !M_max)
		return hipSuccess;
	hipLaunchKernelGGL(k_tb_fit_part, dim3(P / 256u, count), dim3(256), 0, st, desc, arena, weights, gnc, first, iter);
	hipLaunchKernelGGL(k_tb_fit, dim3(count), dim3(RT), 0, st, desc, arena, gnc, first, iter);
	hipLaunchKernelGGL(k_tb_cost_part, dim3(P / 256u, count), dim3(256), 0, st, desc, arena, weights, gnc, first, iter);
	hipLaunchKernelGGL(k_tb_cost, dim3(count), dim3(RT), 0, st, desc, arena, gnc, frozen, first, iter, nb2);
	const uint32_t blocks = (uint32_t)std::min<uint64_t>((M_max + 255u) / 256u, 4096u);
	hipLaunchKernelGGL(k_tb_update, dim3(blocks, count), dim3(256), 0, st, desc, arena, weights, gnc, frozen, first, nb2);
	return hipGetLastError();
}
