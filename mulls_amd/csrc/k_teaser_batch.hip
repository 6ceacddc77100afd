// k_teaser_batch.hip — the kernels of mulls_coarse_reg_teaser_batch: the steps of k_teaser.hip over the problems of one sub-batch per launch, driven by
// the descriptor table of teaser_batch.h (a problem's n, W, m, C and the offsets of its arrays in the arena).  The problem is a grid axis: blockIdx.y
// (blockIdx.z for the graph, blockIdx.x for the single-workgroup steps), and every loop is bounded by that problem's own sizes, so a block beyond them
// leaves at once.  The arithmetic is the text the single call compiles: teaser_math.h, and measurement / tree_sum of teaser_device.h; each problem has its
// own partial sums and its own TeaserGnc record, so every sum has the order of the definition (include/mulls_hip.h) per problem.
//   GNC, lock-step: iteration `iter` is one launch set for all problems.  A problem whose record carries stop != 0 from an EARLIER iteration is skipped
//   by every kernel (a test on the record, uniform per workgroup): k_tb_cost, the first kernel that may change the word, marks such a problem in
//   frozen[], which is what lets k_tb_update tell "stopped before" (skip) from "the cost settled in this iteration" (stop == 2: the update still runs, as
//   in the single call, which breaks after it).  A problem with C < 2 never enters.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "teaser_batch_launch.h"
#include "teaser_device.h"

namespace
{
template <typename T>
__device__ __forceinline__ T *at(unsigned char *arena, uint64_t off)
{
	return reinterpret_cast<T *>(arena + off);
}

// out[i] = the first four floats of record idx[i] (idx == NULL: i) of a device cloud of 48-byte records: launch_ransac_gather over a list of jobs
__global__ void __launch_bounds__(256) k_tb_gather(const TeaserBatchGather *__restrict__ jobs, unsigned char *arena)
{
	const TeaserBatchGather J = jobs[blockIdx.y];
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= J.n)
		return;
	const int32_t *idx = J.indexed ? at<const int32_t>(arena, J.idx) : nullptr;
	const uint32_t r = idx ? (uint32_t)idx[i] : i; // (the host checked every index against its cloud)
	at<float4>(arena, J.out)[i] = *reinterpret_cast<const float4 *>(J.recs + (size_t)r * 48u);
}

__global__ void __launch_bounds__(256) k_tb_graph(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, double beta)
{
	__shared__ float4 si[WAVE], ti[WAVE];
	const TeaserBatchDesc &D = desc[blockIdx.z];
	const uint32_t n = D.n, W = D.W;
	if (blockIdx.y >= W || blockIdx.x * 4u >= W) // (uniform: the grid is sized for the largest problem)
		return;
	const float4 *src = at<const float4>(arena, D.src), *tgt = at<const float4>(arena, D.tgt);
	uint64_t *adj = at<uint64_t>(arena, D.adj);
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

__global__ void __launch_bounds__(256) k_tb_degrees(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, unsigned long long *deg_sum)
{
	const TeaserBatchDesc &D = desc[blockIdx.y];
	const uint32_t n = D.n, W = D.W;
	const uint32_t i = blockIdx.x * 4u + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
	if (i >= n)
		return;
	const uint64_t *adj = at<const uint64_t>(arena, D.adj);
	uint32_t c = 0;
	for (uint32_t w = lane; w < W; w += WAVE)
		c += (uint32_t)__popcll(adj[(size_t)i * W + w]);
	c = wave_sum(c);
	if (lane == 0)
	{
		at<uint32_t>(arena, D.deg)[i] = c;
		if (c)
			atomicAdd(&deg_sum[blockIdx.y], (unsigned long long)c);
	}
}

// k_teaser_cores, one workgroup per problem: the peeling in rounds, with the LDS sets swept up to the problem's own W words and not to the 128 of the
// largest problem (integers: the core numbers do not depend on it).  50 KB of LDS and 1024 threads: two workgroups per CU, by the wave slots (2 x 16 of
// the 32 a CU holds) before the LDS (which has room for three: 3 x 50 of 160 KB), so sizing the arrays to the sub-batch's largest n would not raise the
// residency.
__global__ void __launch_bounds__(RT) k_tb_cores(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena)
{
	__shared__ unsigned long long alive[MULLS_TEASER_MAX_POINTS / 64];
	__shared__ uint32_t gone[MULLS_TEASER_MAX_POINTS / 32];
	__shared__ uint32_t cur[MULLS_TEASER_MAX_POINTS];
	__shared__ uint16_t leavers[MULLS_TEASER_MAX_POINTS];
	__shared__ uint32_t sh_removed, sh_alive, sh_min;
	const TeaserBatchDesc &D = desc[blockIdx.x];
	const uint32_t n = D.n, W = D.W; // (n <= MULLS_TEASER_MAX_POINTS: the host refuses more)
	const uint64_t *adj = at<const uint64_t>(arena, D.adj);
	const uint32_t *deg = at<const uint32_t>(arena, D.deg);
	uint32_t *core = at<uint32_t>(arena, D.core);
	const uint32_t t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
	for (uint32_t w = t; w < W; w += RT)
	{
		const uint32_t lo = w * 64u;
		alive[w] = lo + 64u <= n ? ~0ull : (1ull << (n - lo)) - 1ull; // (lo < n: w < W)
	}
	for (uint32_t v = t; v < n; v += RT)
		cur[v] = deg[v];
	uint32_t k = 0;
	__syncthreads();
	for (uint32_t round = 0; round < 2u * n + 2u; round++)
	{
		for (uint32_t w = t; w < 2u * W; w += RT)
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
		if (t < W)
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

__global__ void __launch_bounds__(256) k_tb_greedy(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena)
{
	const TeaserBatchDesc &D = desc[blockIdx.y];
	const uint32_t n = D.n, W = D.W;
	const uint32_t v = blockIdx.x * 4u + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
	if (v >= n)
		return;
	const uint64_t *adj = at<const uint64_t>(arena, D.adj);
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
		at<uint32_t>(arena, D.core)[n + v] = size; // the greedy sizes lie behind the core numbers
}

__global__ void __launch_bounds__(256) k_tb_compact(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena)
{
	const TeaserBatchDesc &D = desc[blockIdx.y];
	const uint32_t W = D.W, m = D.m, Wm = D.Wm;
	const uint32_t id = blockIdx.x * 4u + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
	if (!m || id / Wm >= m) // (m = 0: a graph without an edge, nothing to search)
		return;
	const uint32_t r = id / Wm, w = id % Wm;
	const uint64_t *adj = at<const uint64_t>(arena, D.adj);
	const int32_t *keep = at<const int32_t>(arena, D.keep);
	const uint32_t c = w * 64u + lane;
	bool e = false;
	if (c < m)
	{
		const uint32_t j = (uint32_t)keep[c];
		e = (adj[(size_t)keep[r] * W + (j >> 6)] >> (j & 63u)) & 1ull;
	}
	const unsigned long long bits = __ballot(e);
	if (lane == 0)
		at<uint64_t>(arena, D.sub)[(size_t)r * Wm + w] = bits;
}

__global__ void __launch_bounds__(256) k_tb_pick(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena)
{
	const TeaserBatchDesc &D = desc[blockIdx.y];
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= D.C)
		return;
	const int32_t *clique = at<const int32_t>(arena, D.keep); // (the host made the list from vertex numbers below n)
	at<float4>(arena, D.cs)[k] = at<const float4>(arena, D.src)[clique[k]];
	at<float4>(arena, D.ct)[k] = at<const float4>(arena, D.tgt)[clique[k]];
}

// ---- GNC: problem first + blockIdx.y (blockIdx.x in the single-workgroup kernels)
__device__ __forceinline__ bool enters(const TeaserBatchDesc &D, const TeaserGnc *S, int iter)
{
	return D.C >= 2u && (iter == 0 || S->stop == 0u); // (iteration 0 writes every field of the record: nothing of an earlier call is read)
}

// partial p adds the measurements p, p + P, ... in ascending order
__global__ void __launch_bounds__(256) k_tb_fit_part(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, unsigned char *warena, const TeaserGnc *gnc,
													  uint32_t first_problem, int iter)
{
	const uint32_t pb = first_problem + blockIdx.y;
	const TeaserBatchDesc &D = desc[pb];
	if (!enters(D, &gnc[pb], iter))
		return;
	const float4 *cs = at<const float4>(arena, D.cs), *ct = at<const float4>(arena, D.ct);
	const double *weights = at<const double>(warena, D.weights);
	double *part = at<double>(arena, D.part);
	const uint32_t C = D.C;
	const uint64_t M = D.M;
	const int first = iter == 0;
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

__global__ void __launch_bounds__(RT) k_tb_fit(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, TeaserGnc *gnc, uint32_t first_problem, int iter)
{
	__shared__ double red[RT];
	const uint32_t pb = first_problem + blockIdx.x;
	const TeaserBatchDesc &D = desc[pb];
	TeaserGnc *S = &gnc[pb];
	if (!enters(D, S, iter))
		return;
	const double *part = at<const double>(arena, D.part);
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

__global__ void __launch_bounds__(256) k_tb_cost_part(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, unsigned char *warena, const TeaserGnc *gnc,
													   uint32_t first_problem, int iter)
{
	const uint32_t pb = first_problem + blockIdx.y;
	const TeaserBatchDesc &D = desc[pb];
	const TeaserGnc *S = &gnc[pb];
	if (!enters(D, S, iter))
		return;
	const float4 *cs = at<const float4>(arena, D.cs), *ct = at<const float4>(arena, D.ct);
	const double *weights = at<const double>(warena, D.weights);
	double *part = at<double>(arena, D.part);
	const uint32_t C = D.C;
	const uint64_t M = D.M;
	const int first = iter == 0;
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

__global__ void __launch_bounds__(RT) k_tb_cost(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, TeaserGnc *gnc, uint32_t *frozen,
												 uint32_t first_problem, int iter, double nb2)
{
	__shared__ double red[RT];
	const uint32_t pb = first_problem + blockIdx.x;
	const TeaserBatchDesc &D = desc[pb];
	TeaserGnc *S = &gnc[pb];
	if (!enters(D, S, iter)) // (every thread reads the word here; thread 0 writes it behind the barriers of the sums below)
	{
		if (threadIdx.x == 0)
			frozen[pb] = 1u; // stopped in an earlier iteration (or never entered): k_tb_update leaves the weights and the count alone
		return;
	}
	const double *part = at<const double>(arena, D.part);
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

__global__ void __launch_bounds__(256) k_tb_update(const TeaserBatchDesc *__restrict__ desc, unsigned char *arena, unsigned char *warena, TeaserGnc *gnc,
													const uint32_t *__restrict__ frozen, uint32_t first_problem, double nb2)
{
	const uint32_t pb = first_problem + blockIdx.y;
	const TeaserBatchDesc &D = desc[pb];
	TeaserGnc *S = &gnc[pb];
	if (frozen[pb] || S->stop == 1u) // stop == 1: mu <= 0 in iteration 0, the weights stay 1 (the host counts M inliers)
		return;
	const float4 *cs = at<const float4>(arena, D.cs), *ct = at<const float4>(arena, D.ct);
	double *weights = at<double>(warena, D.weights);
	const uint32_t C = D.C;
	const uint64_t M = D.M;
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

hipError_t launch_teaser_batch_gather(hipStream_t st, const TeaserBatchGather *jobs, uint32_t n_jobs, uint32_t n_max, unsigned char *arena)
{
	if (!n_jobs || !n_max)
		return hipSuccess;
	hipLaunchKernelGGL(k_tb_gather, dim3((n_max + 255u) / 256u, n_jobs), dim3(256), 0, st, jobs, arena);
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
