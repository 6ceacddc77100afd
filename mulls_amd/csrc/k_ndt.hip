// k_ndt.hip — the device side of mulls_ndt / mulls_ndt_batch (gfx950).  One launch of each kernel serves every problem of a sub-batch: blockIdx.y is the
// problem for the per-point and per-slot kernels, blockIdx.x for those that give a problem one workgroup.  Setup: the guess, the box and the stable crop
// (k_ndt_crop), the target's cells into a hash table keyed by the cell index (k_ndt_clear, k_ndt_cells, k_ndt_offsets, k_ndt_scatter) and one lane per leaf that sorts
// its points' indices and adds the points in input order (k_ndt_leaves) — atomics place entries, they never decide an order of additions.  Iteration: the
// host launches k_ndt_eval (the hot path: 28 double sums per source point, strided partials) and k_ndt_decide (the tree, then the Newton / More-Thuente
// state of ndt_math.h on one lane) once per tick; a problem that has stopped returns at once.  No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "ndt_launch.h"
#include "reg_device.h"

namespace
{
static_assert(MULLS_NDT_SEG == MULLS_REG_SEG, "k_ndt_offsets runs reg_device.h's scan");
__device__ inline bool finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

// rows 0 .. 6: DIRECT7 (row 0 alone: DIRECT1); rows 7 .. 32: DIRECT26
__constant__ int8_t c_offsets[33][3] = {
	{0, 0, 0}, {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1},
	{-1, -1, -1}, {-1, 0, -1}, {-1, 1, -1}, {0, -1, -1}, {0, 0, -1}, {0, 1, -1}, {1, -1, -1}, {1, 0, -1}, {1, 1, -1}, {-1, -1, 0}, {0, -1, 0}, {1, -1, 0}, {-1, 0, 0},
	{1, 1, 1}, {1, 0, 1}, {1, -1, 1}, {0, 1, 1}, {0, 0, 1}, {0, -1, 1}, {-1, 1, 1}, {-1, 0, 1}, {-1, -1, 1}, {1, 1, 0}, {0, 1, 0}, {-1, 1, 0}, {1, 0, 0}};

__device__ inline uint32_t hash_slot(int32_t key, uint32_t shift) { return ((uint32_t)key * 2654435761u) >> shift; }

// block-wide minimum / maximum of six floats per thread (lo[3], hi[3]); the result in s_red[0 .. 6) after the call; MULLS_NDT_SEG threads
__device__ inline void block_minmax(float *lo, float *hi, float (*s_red)[MULLS_NDT_SEG])
{
	const uint32_t t = threadIdx.x;
	__syncthreads();
	for (int c = 0; c < 3; c++)
		s_red[c][t] = lo[c], s_red[3 + c][t] = hi[c];
	__syncthreads();
	for (uint32_t w = MULLS_NDT_SEG / 2; w >= 1; w >>= 1)
	{
		if (t < w)
			for (int c = 0; c < 3; c++)
			{
				s_red[c][t] = fminf(s_red[c][t], s_red[c][t + w]);
				s_red[3 + c][t] = fmaxf(s_red[3 + c][t], s_red[3 + c][t + w]);
			}
		__syncthreads();
	}
}

__global__ void __launch_bounds__(MULLS_NDT_SEG) k_ndt_crop(const NdtDesc *__restrict__ desc, unsigned char *arena, NdtOpts opt, NdtRec *rec)
{
	__shared__ float s_red[6][MULLS_NDT_SEG];
	__shared__ uint32_t s_cnt[MULLS_NDT_SEG];
	__shared__ double s_box[6];
	__shared__ int s_bad;
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	const NdtDesc D = desc[p];
	NdtRec &R = rec[p];
	if (t == 0)
		s_bad = 0;
	__syncthreads();
	const float inf = __builtin_huge_valf();
	// the source: finite? the guess, in place; the box of the moved cloud
	float *S = at<float>(arena, D.o_src_in);
	const float *Tg = at<const float>(arena, D.o_tgt_in);
	{
		const uint32_t seg = (D.n_src_in + MULLS_NDT_SEG - 1) / MULLS_NDT_SEG;
		const uint32_t b = t * seg < D.n_src_in ? t * seg : D.n_src_in, e = b + seg < D.n_src_in ? b + seg : D.n_src_in;
		float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
		int bad = 0;
		for (uint32_t i = b; i < e; i++)
		{
			float x = S[3 * i], y = S[3 * i + 1], z = S[3 * i + 2];
			if (!finite3(x, y, z))
				bad = 1;
			if (D.apply_guess)
			{
				const double dx = (double)x, dy = (double)y, dz = (double)z;
				x = (float)(((D.G[0] * dx + D.G[1] * dy) + D.G[2] * dz) + D.G[9]);
				y = (float)(((D.G[3] * dx + D.G[4] * dy) + D.G[5] * dz) + D.G[10]);
				z = (float)(((D.G[6] * dx + D.G[7] * dy) + D.G[8] * dz) + D.G[11]);
				S[3 * i] = x, S[3 * i + 1] = y, S[3 * i + 2] = z;
				if (!finite3(x, y, z))
					bad = 1;
			}
			lo[0] = fminf(lo[0], x), lo[1] = fminf(lo[1], y), lo[2] = fminf(lo[2], z);
			hi[0] = fmaxf(hi[0], x), hi[1] = fmaxf(hi[1], y), hi[2] = fmaxf(hi[2], z);
		}
		if (bad)
			s_bad = 1;
		block_minmax(lo, hi, s_red);
		if (t == 0)
			for (int c = 0; c < 3; c++)
			{
				const double smin = D.apply_guess ? (double)s_red[c][0] : D.src_bound[c], smax = D.apply_guess ? (double)s_red[3 + c][0] : D.src_bound[3 + c];
				s_box[c] = (D.tgt_bound[c] > smin ? D.tgt_bound[c] : smin) - 2.0;
				s_box[3 + c] = (D.tgt_bound[3 + c] < smax ? D.tgt_bound[3 + c] : smax) + 2.0;
			}
		__syncthreads();
	}
	// the stable crop of both clouds: every thread counts its segment, one thread adds the counts up, every thread writes its segment
	float glo[3] = {inf, inf, inf}, ghi[3] = {-inf, -inf, -inf};
	uint32_t kept[2] = {0, 0};
	for (int c = 0; c < 2; c++)
	{
		const float *in = c == 0 ? S : Tg;
		float *out = at<float>(arena, c == 0 ? D.o_src : D.o_tgt);
		const uint32_t n = c == 0 ? D.n_src_in : D.n_tgt_in;
		const uint32_t seg = (n + MULLS_NDT_SEG - 1) / MULLS_NDT_SEG;
		const uint32_t b = t * seg < n ? t * seg : n, e = b + seg < n ? b + seg : n;
		uint32_t cnt = 0;
		int bad = 0;
		for (uint32_t i = b; i < e; i++)
		{
			const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
			if (!finite3(x, y, z))
				bad = 1;
			const bool in_box = (double)x > s_box[0] && (double)x < s_box[3] && (double)y > s_box[1] && (double)y < s_box[4] && (double)z > s_box[2] && (double)z < s_box[5];
			cnt += (!D.crop || in_box) ? 1u : 0u;
		}
		if (bad)
			s_bad = 1;
		s_cnt[t] = cnt;
		__syncthreads();
		if (t == 0)
		{
			uint32_t run = 0;
			for (uint32_t k = 0; k < MULLS_NDT_SEG; k++)
			{
				const uint32_t v = s_cnt[k];
				s_cnt[k] = run;
				run += v;
			}
			kept[c] = run; // (thread 0 only)
			if (c == 0)
				R.n_src = run;
			else
				R.n_tgt = run;
		}
		__syncthreads();
		uint32_t o = s_cnt[t];
		for (uint32_t i = b; i < e; i++)
		{
			const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
			const bool in_box = (double)x > s_box[0] && (double)x < s_box[3] && (double)y > s_box[1] && (double)y < s_box[4] && (double)z > s_box[2] && (double)z < s_box[5];
			if (!D.crop || in_box)
			{
				out[3 * o] = x, out[3 * o + 1] = y, out[3 * o + 2] = z;
				o++;
				if (c == 1)
				{
					glo[0] = fminf(glo[0], x), glo[1] = fminf(glo[1], y), glo[2] = fminf(glo[2], z);
					ghi[0] = fmaxf(ghi[0], x), ghi[1] = fmaxf(ghi[1], y), ghi[2] = fmaxf(ghi[2], z);
				}
			}
		}
		__syncthreads();
	}
	block_minmax(glo, ghi, s_red);
	if (t != 0)
		return;
	// the grid's extent (applyFilter :76-104)
	int status = NDT_ST_OK;
	R.n_leaves = 0, R.n_leaves_used = 0, R.fitness = 0.0;
	if (s_bad)
		status = NDT_ST_NONFINITE;
	else if (kept[0] == 0 || kept[1] == 0)
		status = NDT_ST_EMPTY;
	else
	{
		const float inv = opt.inv_resolution;
		int64_t d[3], prod = 1, prod_b = 1;
		for (int c = 0; c < 3; c++)
		{
			d[c] = (int64_t)((s_red[3 + c][0] - s_red[c][0]) * inv) + 1;
			const float fl = floorf(s_red[c][0] * inv), fh = floorf(s_red[3 + c][0] * inv);
			if (!(fabsf(fl) < 0x1p30f) || !(fabsf(fh) < 0x1p30f))
				status = NDT_ST_GRID;
			else
			{
				R.min_b[c] = (int32_t)fl, R.max_b[c] = (int32_t)fh;
				R.div_b[c] = R.max_b[c] - R.min_b[c] + 1;
			}
		}
		if (status == NDT_ST_OK)
		{
			for (int c = 0; c < 3; c++)
			{
				prod = prod > (int64_t)INT32_MAX ? prod : prod * d[c];
				prod_b = prod_b > (int64_t)INT32_MAX ? prod_b : prod_b * (int64_t)R.div_b[c];
			}
			if (prod > (int64_t)INT32_MAX || prod_b > (int64_t)INT32_MAX)
				status = NDT_ST_GRID;
		}
	}
	R.status = status;
}

// the empty hash table: every key free, every count, start and fill 0
__global__ void __launch_bounds__(256) k_ndt_clear(const NdtDesc *__restrict__ desc, unsigned char *arena)
{
	const NdtDesc D = desc[blockIdx.y];
	const uint32_t s = blockIdx.x * 256u + threadIdx.x;
	if (s >= D.table_size)
		return;
	at<int32_t>(arena, D.o_keys)[s] = -1;
	at<uint32_t>(arena, D.o_count)[s] = 0u, at<uint32_t>(arena, D.o_start)[s] = 0u, at<uint32_t>(arena, D.o_fill)[s] = 0u;
}

// every cropped target point: its cell, the cell's slot in the hash table (claimed by compare-and-swap), the slot's count
__global__ void __launch_bounds__(256) k_ndt_cells(const NdtDesc *__restrict__ desc, unsigned char *arena, NdtOpts opt, const NdtRec *__restrict__ rec)
{
	const uint32_t p = blockIdx.y;
	const NdtRec &R = rec[p];
	if (R.status != NDT_ST_OK)
		return;
	const NdtDesc D = desc[p];
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= R.n_tgt || i >= D.n_tgt_in)
		return;
	const float *Tg = at<const float>(arena, D.o_tgt);
	const float inv = opt.inv_resolution;
	const int32_t c0 = (int32_t)(floorf(Tg[3 * i] * inv) - (float)R.min_b[0]);
	const int32_t c1 = (int32_t)(floorf(Tg[3 * i + 1] * inv) - (float)R.min_b[1]);
	const int32_t c2 = (int32_t)(floorf(Tg[3 * i + 2] * inv) - (float)R.min_b[2]);
	const int32_t key = c0 + c1 * R.div_b[0] + c2 * (R.div_b[0] * R.div_b[1]);
	int32_t *keys = at<int32_t>(arena, D.o_keys);
	uint32_t slot = hash_slot(key, D.table_shift);
	uint32_t found = 0xffffffffu;
	for (uint32_t probe = 0; probe < D.table_size; probe++)
	{
		const int32_t was = atomicCAS(&keys[slot], -1, key);
		if (was == -1 || was == key)
		{
			found = slot;
			break;
		}
		slot = (slot + 1u) & (D.table_size - 1u);
	}
	at<uint32_t>(arena, D.o_cell)[i] = found; // (always found: the table has at least twice as many slots as there are points)
	if (found != 0xffffffffu)
		atomicAdd(&at<uint32_t>(arena, D.o_count)[found], 1u);
}

// start[slot]: the exclusive sum of the counts; the number of occupied slots
__global__ void __launch_bounds__(MULLS_NDT_SEG) k_ndt_offsets(const NdtDesc *__restrict__ desc, unsigned char *arena, NdtRec *rec)
{
	__shared__ uint32_t s_cnt[MULLS_NDT_SEG], s_occ[MULLS_NDT_SEG];
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	if (rec[p].status != NDT_ST_OK)
		return;
	const NdtDesc D = desc[p];
	const uint32_t leaves = scan_counts(at<const uint32_t>(arena, D.o_count), at<uint32_t>(arena, D.o_start), D.table_size, s_cnt, s_occ);
	if (t == 0)
		rec[p].n_leaves = leaves;
}

__global__ void __launch_bounds__(256) k_ndt_scatter(const NdtDesc *__restrict__ desc, unsigned char *arena, const NdtRec *__restrict__ rec)
{
	const uint32_t p = blockIdx.y;
	const NdtRec &R = rec[p];
	if (R.status != NDT_ST_OK)
		return;
	const NdtDesc D = desc[p];
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= R.n_tgt || i >= D.n_tgt_in)
		return;
	(void)list_point(at<const uint32_t>(arena, D.o_cell), at<const uint32_t>(arena, D.o_start), at<uint32_t>(arena, D.o_fill), at<uint32_t>(arena, D.o_list), D.table_size,
					 D.n_tgt_in, i);
}

// one lane per occupied slot: its points' indices ascending, the sums in input order, the leaf
__global__ void __launch_bounds__(256) k_ndt_leaves(const NdtDesc *__restrict__ desc, unsigned char *arena, NdtOpts opt, NdtRec *rec)
{
	const uint32_t p = blockIdx.y;
	if (rec[p].status != NDT_ST_OK)
		return;
	const NdtDesc D = desc[p];
	const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
	if (slot >= D.table_size)
		return;
	const uint32_t n = at<const uint32_t>(arena, D.o_count)[slot];
	if (!n)
		return;
	const uint32_t first = at<const uint32_t>(arena, D.o_start)[slot];
	if (first >= D.n_tgt_in || n > D.n_tgt_in - first)
		return;
	uint32_t *L = at<uint32_t>(arena, D.o_list) + first;
	sort_list(L, n);
	const float *Tg = at<const float>(arena, D.o_tgt);
	double s[3] = {0.0, 0.0, 0.0}, q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	for (uint32_t k = 0; k < n; k++)
	{
		const uint32_t i = L[k] < D.n_tgt_in ? L[k] : 0u;
		const double x = (double)Tg[3 * i], y = (double)Tg[3 * i + 1], z = (double)Tg[3 * i + 2];
		s[0] += x, s[1] += y, s[2] += z;
		q[0] += x * x, q[1] += x * y, q[2] += x * z, q[3] += y * y, q[4] += y * z, q[5] += z * z;
	}
	ndt::Leaf leaf;
	ndt::finalize_leaf((int32_t)n, s, q, opt.min_points, opt.eig_mult, &leaf);
	at<ndt::Leaf>(arena, D.o_leaves)[first] = leaf;
	if (leaf.n >= opt.min_points)
		atomicAdd(&rec[p].n_leaves_used, 1u);
}

__global__ void __launch_bounds__(64) k_ndt_begin(NdtRec *rec, uint32_t P)
{
	const uint32_t p = blockIdx.x * 64u + threadIdx.x;
	if (p >= P)
		return;
	NdtRec &R = rec[p];
	ndt::State S;
	ndt::begin(S);
	if (R.status != NDT_ST_OK)
		S.running = 0;
	R.S = S;
	if (S.running)
		ndt::make_frame(S.xt, &R.F);
}

// The hot path.  Lane l of the problem's MULLS_NDT_TREE lanes takes the source points l, l + MULLS_NDT_TREE, ..: the point under T(xt) rounded to float, its
// 1, 7 or 26 cells, the leaves' terms in offset order into the point's 28 sums, those into the lane's.  The frame's 81 doubles are read from LDS.
__global__ void __launch_bounds__(256) k_ndt_eval(const NdtDesc *__restrict__ desc, unsigned char *arena, NdtOpts opt, const NdtRec *__restrict__ rec)
{
	__shared__ ndt::Frame s_F;
	const uint32_t p = blockIdx.y;
	const NdtRec &R = rec[p];
	if (!R.S.running)
		return;
	{
		const double *src = reinterpret_cast<const double *>(&R.F);
		double *dst = reinterpret_cast<double *>(&s_F);
		if (threadIdx.x < sizeof(ndt::Frame) / 8)
			dst[threadIdx.x] = src[threadIdx.x];
	}
	__syncthreads();
	const NdtDesc D = desc[p];
	const int with_h = R.S.with_hessian;
	const uint32_t n = R.n_src < D.n_src_in ? R.n_src : D.n_src_in;
	const float *S = at<const float>(arena, D.o_src);
	const int32_t *keys = at<const int32_t>(arena, D.o_keys);
	const uint32_t *start = at<const uint32_t>(arena, D.o_start);
	const ndt::Leaf *leaves = at<const ndt::Leaf>(arena, D.o_leaves);
	const int32_t mb0 = R.min_b[0], mb1 = R.min_b[1], mb2 = R.min_b[2], xb0 = R.max_b[0], xb1 = R.max_b[1], xb2 = R.max_b[2];
	const int32_t dv0 = R.div_b[0], dv01 = R.div_b[0] * R.div_b[1];
	const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
	double acc[28];
#pragma unroll
	for (int k = 0; k < 28; k++)
		acc[k] = 0.0;
	for (uint32_t i = lane; i < n; i += MULLS_NDT_TREE)
	{
		const float fx = S[3 * i], fy = S[3 * i + 1], fz = S[3 * i + 2];
		float xp[3];
		ndt::transform_point(s_F.R, s_F.t, fx, fy, fz, xp);
		const float q0 = floorf(xp[0] / opt.resolution), q1 = floorf(xp[1] / opt.resolution), q2 = floorf(xp[2] / opt.resolution);
		if (!(fabsf(q0) < 0x1p30f) || !(fabsf(q1) < 0x1p30f) || !(fabsf(q2) < 0x1p30f))
			continue;
		const int32_t i0 = (int32_t)q0, i1 = (int32_t)q1, i2 = (int32_t)q2;
		const double x[3] = {(double)fx, (double)fy, (double)fz};
		double a[28];
#pragma unroll
		for (int k = 0; k < 28; k++)
			a[k] = 0.0;
		for (int32_t o = 0; o < D.n_offsets; o++)
		{
			const int32_t c0 = i0 + c_offsets[D.offset_first + o][0], c1 = i1 + c_offsets[D.offset_first + o][1], c2 = i2 + c_offsets[D.offset_first + o][2];
			if (c0 < mb0 || c0 > xb0 || c1 < mb1 || c1 > xb1 || c2 < mb2 || c2 > xb2)
				continue;
			const int32_t key = (c0 - mb0) + (c1 - mb1) * dv0 + (c2 - mb2) * dv01;
			uint32_t slot = hash_slot(key, D.table_shift);
			uint32_t found = 0xffffffffu;
			for (uint32_t probe = 0; probe < D.table_size; probe++)
			{
				const int32_t k = keys[slot];
				if (k == key)
					found = slot;
				if (k == key || k == -1)
					break;
				slot = (slot + 1u) & (D.table_size - 1u);
			}
			if (found == 0xffffffffu)
				continue;
			const uint32_t li = start[found];
			if (li >= D.n_tgt_in)
				continue;
			const ndt::Leaf &L = leaves[li];
			if (L.n < opt.min_points)
				continue;
			const double xt[3] = {(double)xp[0] - L.mean[0], (double)xp[1] - L.mean[1], (double)xp[2] - L.mean[2]};
			const double C[6] = {L.icov[0], L.icov[1], L.icov[2], L.icov[3], L.icov[4], L.icov[5]};
			ndt::contribution(x, xt, C, s_F.j, s_F.h, opt.d1, opt.d2, with_h, a);
		}
#pragma unroll
		for (int k = 0; k < 28; k++)
			acc[k] += a[k];
	}
	double *partial = at<double>(arena, D.o_partial);
#pragma unroll
	for (int k = 0; k < 28; k++)
		partial[(uint32_t)k * MULLS_NDT_TREE + lane] = acc[k];
}

__global__ void __launch_bounds__(256) k_ndt_decide(const NdtDesc *__restrict__ desc, unsigned char *arena, NdtOpts opt, NdtRec *rec, uint32_t *running,
													uint32_t *next)
{
	__shared__ double s_p[256];
	__shared__ double s_sum[28];
	__shared__ int s_run, s_with_h;
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	if (p == 0 && t == 0)
		*next = 0u; // (the next tick's count starts from 0)
	if (t == 0)
		s_run = rec[p].S.running, s_with_h = rec[p].S.with_hessian;
	__syncthreads();
	if (!s_run)
		return;
	const NdtDesc D = desc[p];
	const int n_sums = s_with_h ? 28 : 7;
	tree_of_sums(at<const double>(arena, D.o_partial), 28, [&](int k) { return k < n_sums; }, s_p, s_sum);
	if (t != 0)
		return;
	NdtRec &R = rec[p];
	ndt::State S = R.S;
	ndt::Opts o = opt.o;
	o.n_src = (double)R.n_src;
	ndt::advance(S, s_sum, o);
	R.S = S;
	if (S.running)
	{
		ndt::make_frame(S.xt, &R.F);
		atomicAdd(running, 1u);
	}
}

// the float squared distance from every cropped source point under T(p) to its nearest cropped target point: tiles of the target through LDS
__global__ void __launch_bounds__(256) k_ndt_nearest(const NdtDesc *__restrict__ desc, unsigned char *arena, NdtRec *rec, const double *__restrict__ frames)
{
	__shared__ ndt::Frame s_F;
	__shared__ float s_t[256][3];
	const uint32_t p = blockIdx.y;
	NdtRec &R = rec[p];
	if (R.status != NDT_ST_OK)
		return;
	const NdtDesc D = desc[p];
	const uint32_t ns = R.n_src < D.n_src_in ? R.n_src : D.n_src_in, nt = R.n_tgt < D.n_tgt_in ? R.n_tgt : D.n_tgt_in;
	if (blockIdx.x * 256u >= ns)
		return;
	if (frames) // (mulls_gicp: the rotation and translation as given, 12 doubles a problem)
	{
		if (threadIdx.x < 12)
			reinterpret_cast<double *>(&s_F)[threadIdx.x] = frames[12u * p + threadIdx.x];
	}
	else if (threadIdx.x == 0)
		ndt::make_frame(R.S.p, &s_F);
	__syncthreads();
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	const float *S = at<const float>(arena, D.o_src), *Tg = at<const float>(arena, D.o_tgt);
	float xp[3] = {0.f, 0.f, 0.f};
	if (i < ns)
		ndt::transform_point(s_F.R, s_F.t, S[3 * i], S[3 * i + 1], S[3 * i + 2], xp);
	float best = __builtin_huge_valf();
	for (uint32_t base = 0; base < nt; base += 256u)
	{
		const uint32_t k = base + threadIdx.x;
		__syncthreads();
		if (k < nt)
			s_t[threadIdx.x][0] = Tg[3 * k], s_t[threadIdx.x][1] = Tg[3 * k + 1], s_t[threadIdx.x][2] = Tg[3 * k + 2];
		__syncthreads();
		const uint32_t m = nt - base < 256u ? nt - base : 256u;
		for (uint32_t j = 0; j < m; j++)
		{
			const float dx = xp[0] - s_t[j][0], dy = xp[1] - s_t[j][1], dz = xp[2] - s_t[j][2];
			const float d2 = (dx * dx + dy * dy) + dz * dz;
			best = d2 < best ? d2 : best;
		}
	}
	if (i < ns)
		at<float>(arena, D.o_dist)[i] = best;
}
__global__ void __launch_bounds__(256) k_ndt_fitness(const NdtDesc *__restrict__ desc, unsigned char *arena, NdtRec *rec)
{
	__shared__ double s_p[256];
	const uint32_t p = blockIdx.x, t = threadIdx.x;
	NdtRec &R = rec[p];
	if (R.status != NDT_ST_OK)
		return;
	const NdtDesc D = desc[p];
	const uint32_t ns = R.n_src < D.n_src_in ? R.n_src : D.n_src_in;
	const float *dist = at<const float>(arena, D.o_dist);
	double r[16];
#pragma unroll
	for (int m = 0; m < 16; m++)
	{
		double a = 0.0;
		for (uint32_t i = t + 256u * m; i < ns; i += MULLS_NDT_TREE)
			a += (double)dist[i];
		r[m] = a;
	}
	const double sum = tree_of_partials(r, s_p);
	if (t == 0)
		R.fitness = sum / (double)ns;
}
} // namespace

hipError_t launch_ndt_crop(hipStream_t st, const NdtDesc *desc, uint32_t P, unsigned char *arena, NdtOpts opt, NdtRec *rec)
{
	hipLaunchKernelGGL(k_ndt_crop, dim3(P), dim3(MULLS_NDT_SEG), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_ndt_cells(hipStream_t st, const NdtDesc *desc, uint32_t P, uint32_t n_tgt_max, uint32_t table_max, unsigned char *arena, NdtOpts opt, NdtRec *rec)
{
	hipLaunchKernelGGL(k_ndt_clear, dim3(blocks_of(table_max, 256), P), dim3(256), 0, st, desc, arena);
	hipLaunchKernelGGL(k_ndt_cells, dim3(blocks_of(n_tgt_max, 256), P), dim3(256), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_ndt_offsets(hipStream_t st, const NdtDesc *desc, uint32_t P, unsigned char *arena, NdtRec *rec)
{
	hipLaunchKernelGGL(k_ndt_offsets, dim3(P), dim3(MULLS_NDT_SEG), 0, st, desc, arena, rec);
	return hipGetLastError();
}
hipError_t launch_ndt_scatter(hipStream_t st, const NdtDesc *desc, uint32_t P, uint32_t n_tgt_max, unsigned char *arena, const NdtRec *rec)
{
	hipLaunchKernelGGL(k_ndt_scatter, dim3(blocks_of(n_tgt_max, 256), P), dim3(256), 0, st, desc, arena, rec);
	return hipGetLastError();
}
hipError_t launch_ndt_leaves(hipStream_t st, const NdtDesc *desc, uint32_t P, uint32_t table_max, unsigned char *arena, NdtOpts opt, NdtRec *rec)
{
	hipLaunchKernelGGL(k_ndt_leaves, dim3(blocks_of(table_max, 256), P), dim3(256), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_ndt_begin(hipStream_t st, uint32_t P, NdtRec *rec)
{
	hipLaunchKernelGGL(k_ndt_begin, dim3(blocks_of(P, 64)), dim3(64), 0, st, rec, P);
	return hipGetLastError();
}
hipError_t launch_ndt_eval(hipStream_t st, const NdtDesc *desc, uint32_t P, unsigned char *arena, NdtOpts opt, const NdtRec *rec)
{
	hipLaunchKernelGGL(k_ndt_eval, dim3(MULLS_NDT_TREE / 256u, P), dim3(256), 0, st, desc, arena, opt, rec);
	return hipGetLastError();
}
hipError_t launch_ndt_decide(hipStream_t st, const NdtDesc *desc, uint32_t P, unsigned char *arena, NdtOpts opt, NdtRec *rec, uint32_t *running, uint32_t *next)
{
	hipLaunchKernelGGL(k_ndt_decide, dim3(P), dim3(256), 0, st, desc, arena, opt, rec, running, next);
	return hipGetLastError();
}
hipError_t launch_ndt_fitness(hipStream_t st, const NdtDesc *desc, uint32_t P, uint32_t n_src_max, unsigned char *arena, NdtRec *rec, const double *frames)
{
	hipLaunchKernelGGL(k_ndt_nearest, dim3(blocks_of(n_src_max, 256), P), dim3(256), 0, st, desc, arena, rec, frames);
	hipLaunchKernelGGL(k_ndt_fitness, dim3(P), dim3(256), 0, st, desc, arena, rec);
	return hipGetLastError();
}
