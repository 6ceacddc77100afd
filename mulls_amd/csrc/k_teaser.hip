// k_teaser.hip — the TEASER coarse-registration solver (CRegistration::coarse_reg_teaser, cregistration.hpp:664-759) for gfx950.
//   k_teaser_graph    the pair-consistency graph as a bit matrix: a wave tests 64 consecutive j against one i and stores the ballot word
//   k_teaser_degrees  a wave per row: popcounts
//   k_teaser_cores    one workgroup: core numbers by peeling in rounds (alive set and degrees in LDS, a wave per leaving vertex lowers its neighbours')
//   k_teaser_greedy   a wave per vertex: the clique grown by taking the smallest common neighbour — the lower bound of the exact search
//   k_teaser_compact  the sub-matrix of the vertices that can still belong to a maximum clique
//   k_teaser_pick     the clique's points
//   k_teaser_fit_part / _fit, _cost_part / _cost, _update   one GNC-TLS iteration over the clique's pairwise measurements
// Every double expression is written in the order include/mulls_hip.h and DESIGN.md section 7.4 define (built with -ffp-contract=off); the shared
// arithmetic is teaser_math.h, which the CPU harness compiles too: tests/teaser_restated.py reproduces the bits.
#include <hip/hip_runtime.h>

#include "teaser_device.h"
#include "teaser_launch.h"

namespace
{
__global__ void __launch_bounds__(256) k_teaser_graph(const float4 *__restrict__ src, const float4 *__restrict__ tgt, uint32_t n, uint32_t W, double beta,
													   uint64_t *__restrict__ adj)
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
	const uint32_t rows = min((uint32_t)WAVE, n - i0); // (i0 < n: the grid has ceil(n / 64) rows of blocks)
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

__global__ void __launch_bounds__(256) k_teaser_degrees(const uint64_t *__restrict__ adj, uint32_t n, uint32_t W, uint32_t *__restrict__ deg,
														 unsigned long long *deg_sum)
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
// stays below n: at most 2 n + 2 rounds.  Every row is read once.
__global__ void __launch_bounds__(RT) k_teaser_cores(const uint64_t *__restrict__ adj, uint32_t n, uint32_t W, const uint32_t *__restrict__ deg,
													  uint32_t *__restrict__ core)
{
	__shared__ unsigned long long alive[MULLS_TEASER_MAX_POINTS / 64];
	__shared__ uint32_t gone[MULLS_TEASER_MAX_POINTS / 32];
	__shared__ uint32_t cur[MULLS_TEASER_MAX_POINTS];
	__shared__ uint16_t leavers[MULLS_TEASER_MAX_POINTS];
	__shared__ uint32_t sh_removed, sh_alive, sh_min;
	const uint32_t t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
	for (uint32_t w = t; w < MULLS_TEASER_MAX_POINTS / 64; w += RT)
	{
		const uint32_t lo = w * 64u;
		alive[w] = lo + 64u <= n ? ~0ull : (lo < n ? (1ull << (n - lo)) - 1ull : 0ull);
	}
	for (uint32_t v = t; v < n; v += RT)
		cur[v] = deg[v];
	uint32_t k = 0;
	__syncthreads();
	for (uint32_t round = 0; round < 2u * n + 2u; round++)
	{
		for (uint32_t w = t; w < MULLS_TEASER_MAX_POINTS / 32; w += RT)
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
		if (t < MULLS_TEASER_MAX_POINTS / 64)
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

__global__ void __launch_bounds__(256) k_teaser_greedy(const uint64_t *__restrict__ adj, uint32_t n, uint32_t W, uint32_t *__restrict__ greedy)
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

__global__ void __launch_bounds__(256) k_teaser_compact(const uint64_t *__restrict__ adj, uint32_t W, const int32_t *__restrict__ keep, uint32_t m, uint32_t Wm,
														 uint64_t *__restrict__ sub)
{
	const uint32_t id = blockIdx.x * 4u + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
	const uint32_t r = id / Wm, w = id % Wm;
	if (r >= m)
		return;
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

__global__ void __launch_bounds__(256) k_teaser_pick(const float4 *src, const float4 *tgt, const int32_t *clique, uint32_t C, float4 *cs, float4 *ct)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= C)
		return;
	cs[k] = src[clique[k]]; // (the host made the list from vertex numbers below n)
	ct[k] = tgt[clique[k]];
}

// partial p adds the measurements p, p + P, ... in ascending order
__global__ void __launch_bounds__(256) k_teaser_fit_part(const float4 *__restrict__ cs, const float4 *__restrict__ ct, uint32_t C, uint64_t M, int first,
														  const double *__restrict__ weights, double *__restrict__ part)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // the grid is exactly P threads
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

__global__ void __launch_bounds__(RT) k_teaser_fit(const double *__restrict__ part, int iter, TeaserGnc *S)
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

__global__ void __launch_bounds__(256) k_teaser_cost_part(const float4 *__restrict__ cs, const float4 *__restrict__ ct, uint32_t C, uint64_t M, int first,
														   const double *__restrict__ weights, const TeaserGnc *__restrict__ S, double *__restrict__ part)
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

__global__ void __launch_bounds__(RT) k_teaser_cost(const double *__restrict__ part, int iter, double nb2, TeaserGnc *S)
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

__global__ void __launch_bounds__(256) k_teaser_update(const float4 *__restrict__ cs, const float4 *__restrict__ ct, uint32_t C, uint64_t M, double nb2,
														double *__restrict__ weights, TeaserGnc *S)
{
	if (S->stop == 1u) // mu <= 0 in iteration 0: the weights stay 1 (the host counts M inliers)
		return;
	double R[9];
#pragma unroll
	for (int q = 0; q < 9; q++)
		R[q] = S->R[q];
	const double mu = S->mu;
	uint32_t mine = 0;
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < M; k += stride)
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
