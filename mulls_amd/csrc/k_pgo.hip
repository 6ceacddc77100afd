// k_pgo.hip — the device side of mulls_pgo_optimize / mulls_pgo_optimize_batch (gfx950, all double).  One launch of each kernel serves every problem
// of a sub-batch: blockIdx.y is the problem for the per-edge, per-entry and per-node kernels, blockIdx.x for the two that give a problem one workgroup
// (factor and solve; decide).  A problem that has stopped is skipped with its record frozen.  No kernel waits for another workgroup, none loops over
// iterations: the host launches them once per Levenberg-Marquardt iteration (pgo.cpp).  The order of every sum is the one include/mulls_hip.h states.
#include <hip/hip_runtime.h>

#include "../../include/mulls_hip.h"
#include "pgo_launch.h"
#include "pgo_math.h"

namespace
{
template <typename T>
__device__ inline T *at(unsigned char *arena, uint64_t off)
{
	return reinterpret_cast<T *>(arena + off);
}
__device__ inline bool finite(double x) { return __builtin_isfinite(x); }

__global__ void __launch_bounds__(64) k_pgo_reset(PgoRec *rec, uint32_t P)
{
	const uint32_t p = blockIdx.x * 64u + threadIdx.x;
	if (p >= P)
		return;
	PgoRec r;
	r.cost = r.initial_cost = 0.0;
	r.radius = 1e4, r.nu = 2.0, r.md = 0.0, r.gmax = 0.0, r.dmax = 0.0;
	r.status = 1, r.termination = 0, r.iterations = 0, r.successful = 0;
	r.running = 1, r.relin = 1, r.solve_failed = 0, r.pad = 0;
	rec[p] = r;
}

// full = 1: the edge's slot at the state; full = 0: only rho(s), at the candidate
template <int FULL>
__global__ void __launch_bounds__(64) k_pgo_edges(const PgoDesc *__restrict__ desc, unsigned char *arena, PgoOpts opt, const PgoRec *__restrict__ rec)
{
	const uint32_t p = blockIdx.y;
	const PgoRec &R = rec[p];
	if (!R.running || (FULL ? !R.relin : R.solve_failed))
		return;
	const PgoDesc D = desc[p];
	const uint32_t e = blockIdx.x * 64u + threadIdx.x;
	if (e >= D.n_edges)
		return;
	const PgoEdge &E = at<const PgoEdge>(arena, D.o_edges)[e];
	const double *X = at<const double>(arena, FULL ? D.o_state : D.o_cand);
	double xa[7], xb[7], th[3], qh[4];
#pragma unroll
	for (int i = 0; i < 7; i++)
		xa[i] = X[7u * (uint32_t)E.a + i], xb[i] = X[7u * (uint32_t)E.b + i];
#pragma unroll
	for (int i = 0; i < 3; i++)
		th[i] = E.th[i];
#pragma unroll
	for (int i = 0; i < 4; i++)
		qh[i] = E.qh[i];
	double r[6], Rm[9], v[3], Pq[4], Qq[4], u[6], w;
	pgo::residual(xa, xb, th, qh, r, Rm, v, Pq, Qq);
	const double s = pgo::weighted_square(E.W, r, u);
	at<double>(arena, D.o_term)[e] = pgo::robust(s, opt.robustify, opt.delta, &w);
	if (!FULL)
		return;
	double Ja[36], Jb[36], WJ[36];
	pgo::jacobians(Rm, v, Pq, Qq, qh, Ja, Jb);
	double *S = at<double>(arena, D.o_slot) + (size_t)MULLS_PGO_SLOT_DOUBLES * e;
	// WJa, then Haa
#pragma unroll
	for (int k = 0; k < 6; k++)
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			double a = 0.0;
#pragma unroll
			for (int l = 0; l < 6; l++)
				a += E.W[6 * k + l] * Ja[6 * l + c];
			WJ[6 * k + c] = w * a;
		}
#pragma unroll
	for (int rr = 0; rr < 6; rr++)
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			double a = 0.0;
#pragma unroll
			for (int k = 0; k < 6; k++)
				a += Ja[6 * k + rr] * WJ[6 * k + c];
			S[6 * rr + c] = a;
		}
	// WJb, then Hab and Hbb
#pragma unroll
	for (int k = 0; k < 6; k++)
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			double a = 0.0;
#pragma unroll
			for (int l = 0; l < 6; l++)
				a += E.W[6 * k + l] * Jb[6 * l + c];
			WJ[6 * k + c] = w * a;
		}
#pragma unroll
	for (int rr = 0; rr < 6; rr++)
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			double a = 0.0, b = 0.0;
#pragma unroll
			for (int k = 0; k < 6; k++)
			{
				a += Ja[6 * k + rr] * WJ[6 * k + c];
				b += Jb[6 * k + rr] * WJ[6 * k + c];
			}
			S[36 + 6 * rr + c] = a;
			S[72 + 6 * rr + c] = b;
		}
#pragma unroll
	for (int k = 0; k < 6; k++)
		u[k] = w * u[k];
#pragma unroll
	for (int rr = 0; rr < 6; rr++)
	{
		double a = 0.0, b = 0.0;
#pragma unroll
		for (int k = 0; k < 6; k++)
		{
			a += Ja[6 * k + rr] * u[k];
			b += Jb[6 * k + rr] * u[k];
		}
		S[108 + rr] = a;
		S[114 + rr] = b;
	}
}

// 0.5 times the defined sum of term[0 .. n): strided partials, pairwise tree; every thread of the workgroup of MULLS_PGO_TREE calls it, s_p is its LDS
__device__ inline double tree_sum(const double *term, uint32_t n, double *s_p)
{
	const uint32_t l = threadIdx.x;
	double a = 0.0;
	for (uint32_t i = l; i < n; i += MULLS_PGO_TREE)
		a += term[i];
	s_p[l] = a;
	__syncthreads();
	for (uint32_t w = MULLS_PGO_TREE / 2; w >= 1; w >>= 1)
	{
		if (l < w)
			s_p[l] += s_p[l + w];
		__syncthreads();
	}
	const double r = s_p[0];
	__syncthreads();
	return r;
}
// the largest |x[i]| (NaN entries do not count)
__device__ inline double tree_absmax(const double *x, uint32_t n, double *s_p)
{
	const uint32_t l = threadIdx.x;
	double m = 0.0;
	for (uint32_t i = l; i < n; i += MULLS_PGO_TREE)
	{
		const double a = fabs(x[i]);
		m = a > m ? a : m;
	}
	s_p[l] = m;
	__syncthreads();
	for (uint32_t w = MULLS_PGO_TREE / 2; w >= 1; w >>= 1)
	{
		if (l < w)
			s_p[l] = s_p[l + w] > s_p[l] ? s_p[l + w] : s_p[l];
		__syncthreads();
	}
	const double r = s_p[0];
	__syncthreads();
	return r;
}

__global__ void __launch_bounds__(MULLS_PGO_TREE) k_pgo_begin(const PgoDesc *__restrict__ desc, unsigned char *arena, PgoOpts opt, PgoRec *rec)
{
	__shared__ double s_p[MULLS_PGO_TREE];
	const uint32_t p = blockIdx.x;
	const PgoDesc D = desc[p];
	const double cost = 0.5 * tree_sum(at<const double>(arena, D.o_term), D.n_edges, s_p);
	if (threadIdx.x)
		return;
	PgoRec &R = rec[p];
	R.cost = R.initial_cost = cost;
	R.relin = 0; // the slots hold the linearisation at the start: the first iteration does not repeat it
	if (!finite(cost))
		R.status = -2, R.running = 0;
	else if (D.n_unk == 0)
		R.termination = MULLS_PGO_TERM_NO_FREE, R.running = 0;
	else if (opt.num_iterations <= 0)
		R.termination = MULLS_PGO_TERM_MAX_ITERATIONS, R.running = 0;
}

__global__ void __launch_bounds__(256) k_pgo_assemble(const PgoDesc *__restrict__ desc, unsigned char *arena, const PgoRec *__restrict__ rec)
{
	const uint32_t p = blockIdx.y;
	if (!rec[p].running)
		return;
	const PgoDesc D = desc[p];
	const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	const uint64_t n_h = 36ull * D.n_blocks;
	if (idx >= n_h + 6ull * D.n_unk)
		return;
	const PgoEdge *E = at<const PgoEdge>(arena, D.o_edges);
	const uint32_t *adj0 = at<const uint32_t>(arena, D.o_adj0), *adj = at<const uint32_t>(arena, D.o_adj);
	const uint32_t *node = at<const uint32_t>(arena, D.o_node);
	const double *slot = at<const double>(arena, D.o_slot);
	if (idx >= n_h)
	{
		const uint32_t k = (uint32_t)(idx - n_h), ui = k / 6u, r = k % 6u;
		const int32_t i = (int32_t)node[ui];
		double a = 0.0;
		for (uint32_t t = adj0[i]; t < adj0[i + 1]; t++)
		{
			const uint32_t e = adj[t];
			a += slot[(size_t)MULLS_PGO_SLOT_DOUBLES * e + (E[e].a == i ? 108u : 114u) + r];
		}
		at<double>(arena, D.o_g)[k] = a;
		at<double>(arena, D.o_delta)[k] = -a;
		return;
	}
	const uint32_t blk = (uint32_t)(idx / 36u), rc = (uint32_t)(idx % 36u), r = rc / 6u, c = rc % 6u;
	const uint32_t ui = at<const uint32_t>(arena, D.o_blkrow)[blk];
	const uint32_t uj = at<const uint32_t>(arena, D.o_first)[ui] + (blk - at<const uint32_t>(arena, D.o_rowoff)[ui]);
	const int32_t i = (int32_t)node[ui], j = (int32_t)node[uj];
	double a = 0.0;
	for (uint32_t t = adj0[i]; t < adj0[i + 1]; t++)
	{
		const uint32_t e = adj[t];
		const double *S = slot + (size_t)MULLS_PGO_SLOT_DOUBLES * e;
		const bool i_is_a = E[e].a == i;
		if (ui == uj)
			a += S[(i_is_a ? 0u : 72u) + rc];
		else if ((i_is_a ? E[e].b : E[e].a) == j)
			a += S[36u + (i_is_a ? rc : 6u * c + r)];
	}
	if (ui == uj && r == c)
	{
		const double lo = a > 1e-6 ? a : 1e-6;
		const double d = (lo < 1e32 ? lo : 1e32) / rec[p].radius;
		at<double>(arena, D.o_diag)[6u * ui + r] = d;
		a = a + d;
	}
	at<double>(arena, D.o_H)[idx] = a;
}

__global__ void __launch_bounds__(MULLS_PGO_TREE) k_pgo_factor_solve(const PgoDesc *__restrict__ desc, unsigned char *arena, PgoRec *rec)
{
	__shared__ double s_p[MULLS_PGO_TREE];
	__shared__ double s_L[36], s_y[6];
	__shared__ int s_flag;
	const uint32_t p = blockIdx.x, tid = threadIdx.x;
	if (tid == 0)
		s_flag = rec[p].running;
	__syncthreads();
	if (!s_flag)
		return;
	__syncthreads();
	const PgoDesc D = desc[p];
	const uint32_t U = D.n_unk;
	const double *g = at<const double>(arena, D.o_g), *diag = at<const double>(arena, D.o_diag);
	double *H = at<double>(arena, D.o_H), *y = at<double>(arena, D.o_delta);
	const uint32_t *first = at<const uint32_t>(arena, D.o_first), *rowoff = at<const uint32_t>(arena, D.o_rowoff), *colmax = at<const uint32_t>(arena, D.o_colmax);
	PgoRec &R = rec[p];

	const double gmax = tree_absmax(g, 6u * U, s_p);
	if (gmax <= 1e-10)
	{
		if (tid == 0)
			R.gmax = gmax, R.termination = MULLS_PGO_TERM_GRADIENT, R.running = 0;
		return;
	}
	if (tid == 0)
		R.gmax = gmax, R.iterations += 1, R.solve_failed = 0, s_flag = 0;
	__syncthreads();

	// Cholesky, column by column (left-looking): every entry takes its updates in ascending block column
	for (uint32_t j = 0; j < U; j++)
	{
		const uint32_t rows = colmax[j] - j + 1u, fj = first[j];
		const double *Lj = H + 36ull * rowoff[j]; // block row j from column fj
		for (uint32_t t = tid; t < rows * 36u; t += MULLS_PGO_TREE)
		{
			const uint32_t i = j + t / 36u, rc = t % 36u, r = rc / 6u, c = rc % 6u;
			const uint32_t fi = first[i];
			if (fi > j || (i == j && c > r))
				continue;
			double *Li = H + 36ull * rowoff[i];
			double s = Li[36ull * (j - fi) + rc];
			for (uint32_t k = fi > fj ? fi : fj; k < j; k++)
			{
				const double *A = Li + 36ull * (k - fi) + 6u * r, *B = Lj + 36ull * (k - fj) + 6u * c;
				double a = 0.0;
#pragma unroll
				for (int m = 0; m < 6; m++)
					a += A[m] * B[m];
				s -= a;
			}
			Li[36ull * (j - fi) + rc] = s;
		}
		__syncthreads();
		double *Ljj = H + 36ull * (rowoff[j] + (j - fj));
		if (tid < 36u)
			s_L[tid] = Ljj[tid];
		__syncthreads();
		if (tid == 0)
		{
			for (int c = 0; c < 6; c++)
				for (int r = c; r < 6; r++)
				{
					double x = s_L[6 * r + c];
					for (int m = 0; m < c; m++)
						x -= s_L[6 * r + m] * s_L[6 * c + m];
					if (r == c)
					{
						if (!(x > 0.0) || !finite(x))
							s_flag = 1;
						s_L[6 * c + c] = sqrt(x);
					}
					else
						s_L[6 * r + c] = x / s_L[6 * c + c];
				}
			for (int r = 0; r < 6; r++)
				for (int c = r + 1; c < 6; c++)
					s_L[6 * r + c] = 0.0;
		}
		__syncthreads();
		if (s_flag)
		{
			if (tid == 0)
				R.solve_failed = 1;
			return;
		}
		if (tid < 36u)
			Ljj[tid] = s_L[tid];
		for (uint32_t t = tid; t < (rows - 1u) * 6u; t += MULLS_PGO_TREE)
		{
			const uint32_t i = j + 1u + t / 6u, r = t % 6u, fi = first[i];
			if (fi > j)
				continue;
			double *row = H + 36ull * (rowoff[i] + (j - fi)) + 6u * r;
			double l[6];
#pragma unroll
			for (int c = 0; c < 6; c++)
			{
				double x = row[c];
#pragma unroll
				for (int m = 0; m < c; m++)
					x -= l[m] * s_L[6 * c + m];
				l[c] = x / s_L[6 * c + c];
			}
#pragma unroll
			for (int c = 0; c < 6; c++)
				row[c] = l[c];
		}
		__syncthreads();
	}
	// forward: L y = -g
	for (uint32_t j = 0; j < U; j++)
	{
		const uint32_t fj = first[j];
		if (tid < 36u)
			s_L[tid] = H[36ull * (rowoff[j] + (j - fj)) + tid];
		if (tid < 6u)
			s_y[tid] = y[6u * j + tid];
		__syncthreads();
		if (tid == 0)
			for (int r = 0; r < 6; r++)
			{
				double x = s_y[r];
				for (int m = 0; m < r; m++)
					x -= s_L[6 * r + m] * s_y[m];
				s_y[r] = x / s_L[6 * r + r];
			}
		__syncthreads();
		if (tid < 6u)
			y[6u * j + tid] = s_y[tid];
		const uint32_t rows = colmax[j] - j;
		for (uint32_t t = tid; t < rows * 6u; t += MULLS_PGO_TREE)
		{
			const uint32_t i = j + 1u + t / 6u, r = t % 6u, fi = first[i];
			if (fi > j)
				continue;
			const double *A = H + 36ull * (rowoff[i] + (j - fi)) + 6u * r;
			double a = 0.0;
#pragma unroll
			for (int m = 0; m < 6; m++)
				a += A[m] * s_y[m];
			y[6u * i + r] -= a;
		}
		__syncthreads();
	}
	// backward: L^T delta = y
	for (uint32_t k = U; k-- > 0;)
	{
		const uint32_t fk = first[k];
		if (tid < 36u)
			s_L[tid] = H[36ull * (rowoff[k] + (k - fk)) + tid];
		if (tid < 6u)
			s_y[tid] = y[6u * k + tid];
		__syncthreads();
		if (tid == 0)
			for (int r = 5; r >= 0; r--)
			{
				double x = s_y[r];
				for (int m = r + 1; m < 6; m++)
					x -= s_L[6 * m + r] * s_y[m];
				s_y[r] = x / s_L[6 * r + r];
			}
		__syncthreads();
		if (tid < 6u)
			y[6u * k + tid] = s_y[tid];
		for (uint32_t t = tid; t < (k - fk) * 6u; t += MULLS_PGO_TREE)
		{
			const uint32_t j = fk + t / 6u, c = t % 6u;
			const double *A = H + 36ull * (rowoff[k] + (j - fk));
			double a = 0.0;
#pragma unroll
			for (int m = 0; m < 6; m++)
				a += A[6 * m + c] * s_y[m];
			y[6u * j + c] -= a;
		}
		__syncthreads();
	}
	const double dmax = tree_absmax(y, 6u * U, s_p);
	// the model decrease: -0.5 sum_j delta_j (g_j - D_jj delta_j), the defined sum
	double a = 0.0;
	for (uint32_t i = tid; i < 6u * U; i += MULLS_PGO_TREE)
		a += y[i] * (g[i] - diag[i] * y[i]);
	s_p[tid] = a;
	__syncthreads();
	for (uint32_t w = MULLS_PGO_TREE / 2; w >= 1; w >>= 1)
	{
		if (tid < w)
			s_p[tid] += s_p[tid + w];
		__syncthreads();
	}
	if (tid == 0)
	{
		R.dmax = dmax;
		R.md = -0.5 * s_p[0];
		if (dmax <= 1e-8)
			R.termination = MULLS_PGO_TERM_STEP, R.running = 0;
	}
}

__global__ void __launch_bounds__(64) k_pgo_candidate(const PgoDesc *__restrict__ desc, unsigned char *arena, PgoOpts opt, const PgoRec *__restrict__ rec)
{
	const uint32_t p = blockIdx.y;
	if (!rec[p].running || rec[p].solve_failed)
		return;
	const PgoDesc D = desc[p];
	const uint32_t i = blockIdx.x * 64u + threadIdx.x;
	if (i >= D.n_nodes)
		return;
	const double *X = at<const double>(arena, D.o_state) + 7u * i, *X0 = at<const double>(arena, D.o_init) + 7u * i;
	double *O = at<double>(arena, D.o_cand) + 7u * i;
	const int32_t u = at<const int32_t>(arena, D.o_unk)[i];
	double x[7], x0[7], d[6], o[7];
#pragma unroll
	for (int c = 0; c < 7; c++)
		x[c] = X[c], x0[c] = X0[c];
	if (u < 0)
	{
#pragma unroll
		for (int c = 0; c < 7; c++)
			O[c] = x[c];
		return;
	}
	const double *dl = at<const double>(arena, D.o_delta) + 6u * (uint32_t)u, *lim = at<const double>(arena, D.o_limit) + 2u * i;
#pragma unroll
	for (int c = 0; c < 6; c++)
		d[c] = dl[c];
	pgo::step_node(x, d, x0, at<const int32_t>(arena, D.o_boxed)[i], lim[0], lim[1], opt.only_translation, o);
#pragma unroll
	for (int c = 0; c < 7; c++)
		O[c] = o[c];
}

__global__ void __launch_bounds__(MULLS_PGO_TREE) k_pgo_decide(const PgoDesc *__restrict__ desc, unsigned char *arena, PgoOpts opt, PgoRec *rec, uint32_t *running)
{
	__shared__ double s_p[MULLS_PGO_TREE];
	__shared__ int s_run, s_failed, s_accept;
	const uint32_t p = blockIdx.x, tid = threadIdx.x;
	if (tid == 0)
		s_run = rec[p].running, s_failed = rec[p].solve_failed;
	__syncthreads();
	if (!s_run)
		return;
	const PgoDesc D = desc[p];
	PgoRec &R = rec[p];
	double cp = 0.0;
	if (!s_failed)
		cp = 0.5 * tree_sum(at<const double>(arena, D.o_term), D.n_edges, s_p);
	if (tid == 0)
	{
		bool ok = false;
		double rr = 0.0;
		if (!s_failed && finite(cp) && R.md > 0.0)
		{
			rr = (R.cost - cp) / R.md;
			ok = rr > 1e-3;
		}
		int run = 1;
		if (ok)
		{
			const double old = R.cost, u = 2.0 * rr - 1.0, f = 1.0 - (u * u) * u, third = 1.0 / 3.0;
			const double rad = R.radius / (third > f ? third : f);
			R.radius = rad < 1e16 ? rad : 1e16;
			R.nu = 2.0;
			R.cost = cp;
			R.successful += 1;
			R.relin = 1;
			if (fabs(old - cp) <= opt.function_tolerance * old)
				R.termination = MULLS_PGO_TERM_FUNCTION_TOLERANCE, run = 0;
		}
		else
		{
			R.radius = R.radius / R.nu;
			R.nu = 2.0 * R.nu;
			R.relin = 0;
			if (R.radius < 1e-32)
				R.termination = MULLS_PGO_TERM_RADIUS, run = 0;
		}
		if (run && R.iterations >= opt.num_iterations)
			R.termination = MULLS_PGO_TERM_MAX_ITERATIONS, run = 0;
		R.running = run;
		if (run)
			atomicAdd(running, 1u);
		s_accept = ok;
	}
	__syncthreads();
	if (!s_accept)
		return;
	const double *C = at<const double>(arena, D.o_cand);
	double *X = at<double>(arena, D.o_state);
	for (uint32_t i = tid; i < 7u * D.n_nodes; i += MULLS_PGO_TREE)
		X[i] = C[i];
}
inline uint32_t blocks_of(uint64_t n, uint32_t b) { return (uint32_t)((n + b - 1) / b); }
} // namespace

hipError_t launch_pgo_reset(hipStream_t st, PgoRec *rec, uint32_t P)
{
	hipLaunchKernelGGL(k_pgo_reset, dim3(blocks_of(P, 64)), dim3(64), 0, st, rec, P);
	return hipGetLastError();
}
hipError_t launch_pgo_linearize(hipStream_t st, const PgoDesc *desc, uint32_t P, uint32_t e_max, unsigned char *arena, PgoOpts opt, const PgoRec *rec)
{
	if (!e_max)
		return hipSuccess;
	hipLaunchKernelGGL(k_pgo_edges<1>, dim3(blocks_of(e_max, 64), P), dim3(64), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_pgo_begin(hipStream_t st, const PgoDesc *desc, uint32_t P, unsigned char *arena, PgoOpts opt, PgoRec *rec)
{
	hipLaunchKernelGGL(k_pgo_begin, dim3(P), dim3(MULLS_PGO_TREE), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_pgo_assemble(hipStream_t st, const PgoDesc *desc, uint32_t P, uint64_t w_max, unsigned char *arena, const PgoRec *rec)
{
	if (!w_max)
		return hipSuccess;
	hipLaunchKernelGGL(k_pgo_assemble, dim3(blocks_of(w_max, 256), P), dim3(256), 0, st, desc, arena, rec);
	return hipGetLastError();
}
hipError_t launch_pgo_factor_solve(hipStream_t st, const PgoDesc *desc, uint32_t P, unsigned char *arena, PgoRec *rec)
{
	hipLaunchKernelGGL(k_pgo_factor_solve, dim3(P), dim3(MULLS_PGO_TREE), 0, st, desc, arena, rec);
	return hipGetLastError();
}
hipError_t launch_pgo_candidate(hipStream_t st, const PgoDesc *desc, uint32_t P, uint32_t n_max, unsigned char *arena, PgoOpts opt, const PgoRec *rec)
{
	if (!n_max)
		return hipSuccess;
	hipLaunchKernelGGL(k_pgo_candidate, dim3(blocks_of(n_max, 64), P), dim3(64), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_pgo_cost(hipStream_t st, const PgoDesc *desc, uint32_t P, uint32_t e_max, unsigned char *arena, PgoOpts opt, const PgoRec *rec)
{
	if (!e_max)
		return hipSuccess;
	hipLaunchKernelGGL(k_pgo_edges<0>, dim3(blocks_of(e_max, 64), P), dim3(64), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_pgo_decide(hipStream_t st, const PgoDesc *desc, uint32_t P, unsigned char *arena, PgoOpts opt, PgoRec *rec, uint32_t *running)
{
	hipLaunchKernelGGL(k_pgo_decide, dim3(P), dim3(MULLS_PGO_TREE), 0, st, desc, arena, opt, rec, running);
	return hipGetLastError();
}
