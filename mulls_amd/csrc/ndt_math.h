// ndt_math.h — the arithmetic of mulls_ndt (include/mulls_hip.h has the definition, operation by operation), shared by the host (ndt.cpp: the output pose;
// tests/ndt_math_harness.cpp) and the device (k_ndt.hip: a leaf's finalisation, the evaluation of a source point, the Newton and More-Thuente state).
// Every expression is written in the order the header states; the library is built without FMA contraction, and sin, cos and exp come from detmath.h,
// so host and device give the same bits.  Nothing here calls the C library except sqrt, fabs and floor, which are exact operations.
#pragma once
#include <cmath>
#include <stdint.h>

#include "detmath.h"
#include "jacobi_rot.h"

namespace ndt
{
// a leaf as the evaluation reads it: 13 doubles
struct Leaf
{
	double mean[3];
	double icov[6]; // xx xy xz yy yz zz
	double evals[3]; // ascending, after the inflation
	int32_t n;		 // points; -1: disabled (VoxelGridCovariance sets nr_points = -1)
	int32_t inflated; // eigenvalues raised to min_covar_eigvalue_mult times the largest: 0, 1 or 2
};

// voxel_grid_covariance_omp_impl.hpp:283-367 of one leaf: n points, their sum s[3] and the sum q[6] of their outer products (xx xy xz yy yz zz),
// both added in input order in double
MULLS_HD inline void finalize_leaf(int32_t n, const double *s, const double *q, int32_t min_points, double eig_mult, Leaf *L)
{
	const double dn = (double)n;
	const double m0 = s[0] / dn, m1 = s[1] / dn, m2 = s[2] / dn;
	L->mean[0] = m0, L->mean[1] = m1, L->mean[2] = m2;
	L->n = n, L->inflated = 0;
	for (int k = 0; k < 6; k++)
		L->icov[k] = 0.0;
	L->evals[0] = L->evals[1] = L->evals[2] = 0.0;
	if (n < min_points)
		return;
	// the lower triangle, which is what the eigen-solver reads: element (b, a), b >= a, is ((q_ab - 2 (s_b m_a)) / n + m_b m_a) (n - 1) / n
	const double f = (dn - 1.0) / dn;
	double a00 = ((q[0] - 2.0 * (s[0] * m0)) / dn + m0 * m0) * f;
	double a01 = ((q[1] - 2.0 * (s[1] * m0)) / dn + m1 * m0) * f;
	double a02 = ((q[2] - 2.0 * (s[2] * m0)) / dn + m2 * m0) * f;
	double a11 = ((q[3] - 2.0 * (s[1] * m1)) / dn + m1 * m1) * f;
	double a12 = ((q[4] - 2.0 * (s[2] * m1)) / dn + m2 * m1) * f;
	double a22 = ((q[5] - 2.0 * (s[2] * m2)) / dn + m2 * m2) * f;
	double c00 = a00, c01 = a01, c02 = a02, c11 = a11, c12 = a12, c22 = a22;
	double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
	for (int sweep = 0; sweep < 60; sweep++)
	{
		const double off = a01 * a01 + a02 * a02 + a12 * a12;
		if (!(off >= 1e-300))
			break;
		MULLS_PCA_ROT(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21) // (0,1)
		MULLS_PCA_ROT(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22) // (0,2)
		MULLS_PCA_ROT(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22) // (1,2)
	}
	// ascending, the lower index first among equals
	double e0 = a00, e1 = a11, e2 = a22;
	double x0 = v00, y0 = v10, z0 = v20, x1 = v01, y1 = v11, z1 = v21, x2 = v02, y2 = v12, z2 = v22;
#define MULLS_NDT_SWAP(ea, eb, xa, ya, za, xb, yb, zb) \
	if (eb < ea)                                       \
	{                                                  \
		double w = ea;                                 \
		ea = eb, eb = w;                               \
		w = xa, xa = xb, xb = w;                       \
		w = ya, ya = yb, yb = w;                       \
		w = za, za = zb, zb = w;                       \
	}
	MULLS_NDT_SWAP(e0, e1, x0, y0, z0, x1, y1, z1)
	MULLS_NDT_SWAP(e0, e2, x0, y0, z0, x2, y2, z2)
	MULLS_NDT_SWAP(e1, e2, x1, y1, z1, x2, y2, z2)
#undef MULLS_NDT_SWAP
	if (e0 < 0.0 || e1 < 0.0 || !(e2 > 0.0))
	{
		L->n = -1;
		return;
	}
	const double lo = eig_mult * e2;
	if (e0 < lo)
	{
		e0 = lo, L->inflated = 1;
		if (e1 < lo)
			e1 = lo, L->inflated = 2;
		// V diag(e) V^T
		c00 = ((x0 * e0) * x0 + (x1 * e1) * x1) + (x2 * e2) * x2;
		c01 = ((x0 * e0) * y0 + (x1 * e1) * y1) + (x2 * e2) * y2;
		c02 = ((x0 * e0) * z0 + (x1 * e1) * z1) + (x2 * e2) * z2;
		c11 = ((y0 * e0) * y0 + (y1 * e1) * y1) + (y2 * e2) * y2;
		c12 = ((y0 * e0) * z0 + (y1 * e1) * z1) + (y2 * e2) * z2;
		c22 = ((z0 * e0) * z0 + (z1 * e1) * z1) + (z2 * e2) * z2;
	}
	L->evals[0] = e0, L->evals[1] = e1, L->evals[2] = e2;
	// the inverse by cofactors
	const double k00 = c11 * c22 - c12 * c12, k01 = c02 * c12 - c01 * c22, k02 = c01 * c12 - c02 * c11;
	const double k11 = c00 * c22 - c02 * c02, k12 = c01 * c02 - c00 * c12, k22 = c00 * c11 - c01 * c01;
	const double det = (c00 * k00 + c01 * k01) + c02 * k02;
	L->icov[0] = k00 / det, L->icov[1] = k01 / det, L->icov[2] = k02 / det;
	L->icov[3] = k11 / det, L->icov[4] = k12 / det, L->icov[5] = k22 / det;
	const double inf = 1.0 / 0.0;
	for (int k = 0; k < 6; k++)
		if (L->icov[k] == inf || L->icov[k] == -inf)
			L->n = -1;
}

// what an evaluation at p needs of p: the rotation and translation of T(p), and the vectors of equations 6.19 and 6.21
struct Frame
{
	double R[9], t[3];
	double j[8][3];	 // a .. h
	double h[15][3]; // a2 a3 b2 b3 c2 c3 d1 d2 d3 e1 e2 e3 f1 f2 f3
};
MULLS_HD inline void make_frame(const double *p, Frame *F)
{
	using mulls::det::cos_cr;
	using mulls::det::sin_cr;
	{
		// T(p) = Translation(p0, p1, p2) Rx(p3) Ry(p4) Rz(p5), with the angle functions themselves
		const double cx = cos_cr(p[3]), sx = sin_cr(p[3]), cy = cos_cr(p[4]), sy = sin_cr(p[4]), cz = cos_cr(p[5]), sz = sin_cr(p[5]);
		F->R[0] = cy * cz, F->R[1] = -cy * sz, F->R[2] = sy;
		F->R[3] = cx * sz + sx * sy * cz, F->R[4] = cx * cz - sx * sy * sz, F->R[5] = -sx * cy;
		F->R[6] = sx * sz - cx * sy * cz, F->R[7] = cx * sy * sz + sx * cz, F->R[8] = cx * cy;
		F->t[0] = p[0], F->t[1] = p[1], F->t[2] = p[2];
	}
	// computeAngleDerivatives (ndt_omp_impl.hpp:288-393): angles below 10e-5 count as zero there
	double cx, cy, cz, sx, sy, sz;
	if (fabs(p[3]) < 10e-5)
		cx = 1.0, sx = 0.0;
	else
		cx = cos_cr(p[3]), sx = sin_cr(p[3]);
	if (fabs(p[4]) < 10e-5)
		cy = 1.0, sy = 0.0;
	else
		cy = cos_cr(p[4]), sy = sin_cr(p[4]);
	if (fabs(p[5]) < 10e-5)
		cz = 1.0, sz = 0.0;
	else
		cz = cos_cr(p[5]), sz = sin_cr(p[5]);
#define MULLS_NDT_V3(dst, a, b, c) dst[0] = (a), dst[1] = (b), dst[2] = (c)
	MULLS_NDT_V3(F->j[0], (-sx * sz + cx * sy * cz), (-sx * cz - cx * sy * sz), (-cx * cy));
	MULLS_NDT_V3(F->j[1], (cx * sz + sx * sy * cz), (cx * cz - sx * sy * sz), (-sx * cy));
	MULLS_NDT_V3(F->j[2], (-sy * cz), sy * sz, cy);
	MULLS_NDT_V3(F->j[3], sx * cy * cz, (-sx * cy * sz), sx * sy);
	MULLS_NDT_V3(F->j[4], (-cx * cy * cz), cx * cy * sz, (-cx * sy));
	MULLS_NDT_V3(F->j[5], (-cy * sz), (-cy * cz), 0.0);
	MULLS_NDT_V3(F->j[6], (cx * cz - sx * sy * sz), (-cx * sz - sx * sy * cz), 0.0);
	MULLS_NDT_V3(F->j[7], (sx * cz + cx * sy * sz), (cx * sy * cz - sx * sz), 0.0);
	MULLS_NDT_V3(F->h[0], (-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), sx * cy);
	MULLS_NDT_V3(F->h[1], (-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), (-cx * cy));
	MULLS_NDT_V3(F->h[2], (cx * cy * cz), (-cx * cy * sz), (cx * sy));
	MULLS_NDT_V3(F->h[3], (sx * cy * cz), (-sx * cy * sz), (sx * sy));
	MULLS_NDT_V3(F->h[4], (-sx * cz - cx * sy * sz), (sx * sz - cx * sy * cz), 0.0);
	MULLS_NDT_V3(F->h[5], (cx * cz - sx * sy * sz), (-sx * sy * cz - cx * sz), 0.0);
	MULLS_NDT_V3(F->h[6], (-cy * cz), (cy * sz), (sy));
	MULLS_NDT_V3(F->h[7], (-sx * sy * cz), (sx * sy * sz), (sx * cy));
	MULLS_NDT_V3(F->h[8], (cx * sy * cz), (-cx * sy * sz), (-cx * cy));
	MULLS_NDT_V3(F->h[9], (sy * sz), (sy * cz), 0.0);
	MULLS_NDT_V3(F->h[10], (-sx * cy * sz), (-sx * cy * cz), 0.0);
	MULLS_NDT_V3(F->h[11], (cx * cy * sz), (cx * cy * cz), 0.0);
	MULLS_NDT_V3(F->h[12], (-cy * cz), (cy * sz), 0.0);
	MULLS_NDT_V3(F->h[13], (-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), 0.0);
	MULLS_NDT_V3(F->h[14], (-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), 0.0);
#undef MULLS_NDT_V3
}
// T(p) x in double, rounded to float: the point whose cell is looked up
MULLS_HD inline void transform_point(const double *R, const double *t, float x, float y, float z, float *o)
{
	const double dx = (double)x, dy = (double)y, dz = (double)z;
	o[0] = (float)(((R[0] * dx + R[1] * dy) + R[2] * dz) + t[0]);
	o[1] = (float)(((R[3] * dx + R[4] * dy) + R[5] * dz) + t[1]);
	o[2] = (float)(((R[6] * dx + R[7] * dy) + R[8] * dz) + t[2]);
}

MULLS_HD inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// One (point, leaf) contribution, equations 6.9, 6.12 and 6.13, added to a[28] = score, gradient[6], Hessian upper triangle[21] (row by row).
// x: the source point; xt: the transformed point (rounded to float) minus the leaf's mean; j, h: Frame's vectors (h is read only with_hessian).
// Everything is indexed by constants after unrolling: on the device it stays in registers.
template <typename J3, typename H3>
MULLS_HD inline void contribution(const double *x, const double *xt, const double *C, const J3 &j, const H3 &h, double d1, double d2,
								  int with_hessian, double *a)
{
	// C as a full symmetric matrix
	const double c[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
	double cx[3];
#pragma unroll
	for (int r = 0; r < 3; r++)
		cx[r] = dot3(c[r][0], c[r][1], c[r][2], xt[0], xt[1], xt[2]);
	const double q = dot3(xt[0], xt[1], xt[2], cx[0], cx[1], cx[2]);
	const double e = mulls::det::exp_cr((-d2 * q) / 2.0);
	const double score_inc = -d1 * e;
	double e2 = d2 * e;
	if (e2 > 1.0 || e2 < 0.0 || e2 != e2)
		return;
	e2 = e2 * d1;
	// the columns of the point's Jacobian: unit vectors, then (0, x.a, x.b), (x.c, x.d, x.e), (x.f, x.g, x.h)
	double J[3][6];
#pragma unroll
	for (int r = 0; r < 3; r++)
#pragma unroll
		for (int k = 0; k < 3; k++)
			J[r][k] = r == k ? 1.0 : 0.0;
	J[0][3] = 0.0, J[1][3] = dot3(x[0], x[1], x[2], j[0][0], j[0][1], j[0][2]), J[2][3] = dot3(x[0], x[1], x[2], j[1][0], j[1][1], j[1][2]);
	J[0][4] = dot3(x[0], x[1], x[2], j[2][0], j[2][1], j[2][2]), J[1][4] = dot3(x[0], x[1], x[2], j[3][0], j[3][1], j[3][2]);
	J[2][4] = dot3(x[0], x[1], x[2], j[4][0], j[4][1], j[4][2]);
	J[0][5] = dot3(x[0], x[1], x[2], j[5][0], j[5][1], j[5][2]), J[1][5] = dot3(x[0], x[1], x[2], j[6][0], j[6][1], j[6][2]);
	J[2][5] = dot3(x[0], x[1], x[2], j[7][0], j[7][1], j[7][2]);
	// cJ[k] = C J_k (a column of C for k < 3), g[k] = xt . cJ[k]
	double cJ[6][3], g[6];
#pragma unroll
	for (int k = 0; k < 6; k++)
	{
#pragma unroll
		for (int r = 0; r < 3; r++)
			cJ[k][r] = k < 3 ? c[r][k] : dot3(c[r][0], c[r][1], c[r][2], J[0][k], J[1][k], J[2][k]);
		g[k] = dot3(xt[0], xt[1], xt[2], cJ[k][0], cJ[k][1], cJ[k][2]);
	}
	a[0] += score_inc;
#pragma unroll
	for (int k = 0; k < 6; k++)
		a[1 + k] += e2 * g[k];
	if (!with_hessian)
		return;
	// the second derivatives of T(p) x: block (i, k), 3 <= i <= k; (3,3) a, (3,4) b, (3,5) c, (4,4) d, (4,5) e, (5,5) f
	double hv[6][3];
#pragma unroll
	for (int m = 0; m < 3; m++) // a, b, c: (0, x.h[2m], x.h[2m+1])
	{
		hv[m][0] = 0.0;
		hv[m][1] = dot3(x[0], x[1], x[2], h[2 * m][0], h[2 * m][1], h[2 * m][2]);
		hv[m][2] = dot3(x[0], x[1], x[2], h[2 * m + 1][0], h[2 * m + 1][1], h[2 * m + 1][2]);
	}
#pragma unroll
	for (int m = 0; m < 3; m++) // d, e, f
#pragma unroll
		for (int r = 0; r < 3; r++)
			hv[3 + m][r] = dot3(x[0], x[1], x[2], h[6 + 3 * m + r][0], h[6 + 3 * m + r][1], h[6 + 3 * m + r][2]);
	int at = 7;
#pragma unroll
	for (int i = 0; i < 6; i++)
#pragma unroll
		for (int k = i; k < 6; k++, at++)
		{
			double inner = (-d2 * g[i]) * g[k];
			if (i >= 3)
			{
				// (3,3) 0  (3,4) 1  (3,5) 2  (4,4) 3  (4,5) 4  (5,5) 5
				const int b = i == 3 ? k - 3 : (i == 4 ? k - 1 : 5);
				inner = inner + dot3(cx[0], cx[1], cx[2], hv[b][0], hv[b][1], hv[b][2]);
			}
			inner = inner + (k < 3 ? cJ[i][k] : dot3(J[0][k], J[1][k], J[2][k], cJ[i][0], cJ[i][1], cJ[i][2]));
			a[at] += e2 * inner;
		}
}

// delta = -H^+ g: cyclic Jacobi eigen-decomposition (SWEEPS sweeps, pairs (0,1) (0,2) .. (4,5)) of the symmetric matrix whose upper triangle is Hu,
// then the sum over the eigenvalues with |lambda| > 6 * 2^-52 * max |lambda|
constexpr int SOLVE_SWEEPS = 12;
MULLS_HD inline void solve6(const double *Hu, const double *g, double *delta)
{
	double A[6][6], V[6][6];
	int at = 0;
	for (int i = 0; i < 6; i++)
		for (int k = i; k < 6; k++, at++)
			A[i][k] = A[k][i] = Hu[at];
	for (int i = 0; i < 6; i++)
		for (int k = 0; k < 6; k++)
			V[i][k] = i == k ? 1.0 : 0.0;
	for (int sweep = 0; sweep < SOLVE_SWEEPS; sweep++)
		for (int p = 0; p < 5; p++)
			for (int q = p + 1; q < 6; q++)
			{
				const double apq = A[p][q];
				if (apq == 0.0)
					continue;
				const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
				const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
				for (int k = 0; k < 6; k++) // A <- A J
				{
					const double u = A[k][p], w = A[k][q];
					A[k][p] = cs * u - sn * w, A[k][q] = sn * u + cs * w;
				}
				for (int k = 0; k < 6; k++) // A <- J^T A
				{
					const double u = A[p][k], w = A[q][k];
					A[p][k] = cs * u - sn * w, A[q][k] = sn * u + cs * w;
				}
				A[p][q] = A[q][p] = 0.0;
				for (int k = 0; k < 6; k++)
				{
					const double u = V[k][p], w = V[k][q];
					V[k][p] = cs * u - sn * w, V[k][q] = sn * u + cs * w;
				}
			}
	double big = 0.0;
	for (int k = 0; k < 6; k++)
	{
		const double m = fabs(A[k][k]);
		big = m > big ? m : big;
	}
	const double thr = (6.0 * 0x1p-52) * big;
	double c[6];
	for (int k = 0; k < 6; k++)
	{
		double t = 0.0;
		for (int i = 0; i < 6; i++)
			t += V[i][k] * g[i];
		c[k] = fabs(A[k][k]) > thr ? t / A[k][k] : (A[k][k] != A[k][k] ? A[k][k] : 0.0); // (a NaN eigenvalue makes the step NaN: the run ends unconverged)
	}
	for (int i = 0; i < 6; i++)
	{
		double s = 0.0;
		for (int k = 0; k < 6; k++)
			s += V[i][k] * c[k];
		delta[i] = -s;
	}
}

// ---- the Newton loop (computeTransformation, ndt_omp_impl.hpp:119-171) and computeStepLengthMT (:757-916) as a state that advances by one evaluation
enum Phase
{
	PH_INIT = 0,	 // waits for the derivatives at p = 0
	PH_MT_FIRST = 1, // ... at the first trial of a line search (with the Hessian)
	PH_MT_LOOP = 2,	 // ... at a trial of the inner loop (score and gradient)
	PH_HESS = 3		 // ... for the Hessian at the accepted trial (the inner loop ran)
};
struct Opts
{
	double step_size, transformation_epsilon, mu, nu, n_src;
	int32_t max_iterations, max_step_iterations;
};
struct State
{
	double p[6], xt[6]; // the pose; the trial at which the next evaluation is taken
	double x0[6], dir[6];
	double score, g[6], H[21];
	double phi_0, d_phi_0, a_l, f_l, g_l, a_u, f_u, g_u, a_t, phi_t, d_phi_t, psi_t, d_psi_t;
	double trans_probability;
	int32_t phase, step_iterations, interval_converged, open_interval;
	int32_t nr_iterations, evaluations, converged, running;
	int32_t with_hessian, reversals, inner_steps, reserved;
};

MULLS_HD inline bool update_interval(State &S, double a_t, double f_t, double g_t)
{
	if (f_t > S.f_l)
	{
		S.a_u = a_t, S.f_u = f_t, S.g_u = g_t;
		return false;
	}
	else if (g_t * (S.a_l - a_t) > 0)
	{
		S.a_l = a_t, S.f_l = f_t, S.g_l = g_t;
		return false;
	}
	else if (g_t * (S.a_l - a_t) < 0)
	{
		S.a_u = S.a_l, S.f_u = S.f_l, S.g_u = S.g_l;
		S.a_l = a_t, S.f_l = f_t, S.g_l = g_t;
		return false;
	}
	return true;
}
MULLS_HD inline double trial_value(double a_l, double f_l, double g_l, double a_u, double f_u, double g_u, double a_t, double f_t, double g_t)
{
	if (f_t > f_l)
	{
		const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
		const double w = sqrt(z * z - g_t * g_l);
		const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
		const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
		if (fabs(a_c - a_l) < fabs(a_q - a_l))
			return a_c;
		return 0.5 * (a_q + a_c);
	}
	else if (g_t * g_l < 0)
	{
		const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
		const double w = sqrt(z * z - g_t * g_l);
		const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
		const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
		if (fabs(a_c - a_t) >= fabs(a_s - a_t))
			return a_c;
		return a_s;
	}
	else if (fabs(g_t) <= fabs(g_l))
	{
		const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
		const double w = sqrt(z * z - g_t * g_l);
		const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
		const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
		const double a_n = fabs(a_c - a_t) < fabs(a_s - a_t) ? a_c : a_s;
		const double lim = a_t + 0.66 * (a_u - a_t);
		if (a_t > a_l)
			return a_n < lim ? a_n : lim; // std::min(lim, a_n)
		return lim < a_n ? a_n : lim;	  // std::max(lim, a_n)
	}
	const double z = 3 * (f_t - f_u) / (a_t - a_u) - g_t - g_u;
	const double w = sqrt(z * z - g_t * g_u);
	return a_u + (a_t - a_u) * (w - g_u - z) / (g_t - g_u + 2 * w);
}
MULLS_HD inline double clamp_step(double a, double lo, double hi)
{
	a = hi < a ? hi : a; // std::min(a, hi)
	return a < lo ? lo : a; // std::max(a, lo)
}
MULLS_HD inline void set_trial(State &S)
{
	for (int k = 0; k < 6; k++)
		S.xt[k] = S.x0[k] + S.dir[k] * S.a_t;
}

// the state before the first evaluation (at p = 0, with the Hessian)
MULLS_HD inline void begin(State &S)
{
	State z{};
	S = z;
	S.phase = PH_INIT, S.running = 1, S.with_hessian = 1, S.evaluations = 1;
}

// the 28 sums of the evaluation the state asked for have arrived: advance to the next evaluation (running stays 1; xt and with_hessian say which) or to the end
MULLS_HD inline void advance(State &S, const double *sums, const Opts &o)
{
	const double step_max = o.step_size, step_min = o.transformation_epsilon / 2;
	enum
	{
		MT_CHECK,
		NEWTON_END,
		NEWTON_START
	} next;
	if (S.phase == PH_HESS)
	{
		for (int k = 0; k < 21; k++)
			S.H[k] = sums[7 + k];
		next = NEWTON_END;
	}
	else
	{
		S.score = sums[0];
		for (int k = 0; k < 6; k++)
			S.g[k] = sums[1 + k];
		if (S.phase != PH_MT_LOOP)
			for (int k = 0; k < 21; k++)
				S.H[k] = sums[7 + k];
		if (S.phase == PH_INIT)
			next = NEWTON_START;
		else
		{
			S.phi_t = -S.score;
			double d = 0.0;
			for (int k = 0; k < 6; k++)
				d += S.g[k] * S.dir[k];
			S.d_phi_t = -d;
			S.psi_t = S.phi_t - S.phi_0 - o.mu * S.d_phi_0 * S.a_t;
			S.d_psi_t = S.d_phi_t - o.mu * S.d_phi_0;
			if (S.phase == PH_MT_LOOP)
			{
				if (S.open_interval && (S.psi_t <= 0 && S.d_psi_t >= 0))
				{
					S.open_interval = 0;
					S.f_l = S.f_l + S.phi_0 - o.mu * S.d_phi_0 * S.a_l;
					S.g_l = S.g_l + o.mu * S.d_phi_0;
					S.f_u = S.f_u + S.phi_0 - o.mu * S.d_phi_0 * S.a_u;
					S.g_u = S.g_u + o.mu * S.d_phi_0;
				}
				if (S.open_interval)
					S.interval_converged = update_interval(S, S.a_t, S.psi_t, S.d_psi_t) ? 1 : 0;
				else
					S.interval_converged = update_interval(S, S.a_t, S.phi_t, S.d_phi_t) ? 1 : 0;
				S.step_iterations++, S.inner_steps++;
			}
			next = MT_CHECK;
		}
	}
	for (int hop = 0; hop < 8; hop++)
	{
		if (next == MT_CHECK)
		{
			if (!S.interval_converged && S.step_iterations < o.max_step_iterations && !(S.psi_t <= 0 && S.d_phi_t <= -o.nu * S.d_phi_0))
			{
				if (S.open_interval)
					S.a_t = trial_value(S.a_l, S.f_l, S.g_l, S.a_u, S.f_u, S.g_u, S.a_t, S.psi_t, S.d_psi_t);
				else
					S.a_t = trial_value(S.a_l, S.f_l, S.g_l, S.a_u, S.f_u, S.g_u, S.a_t, S.phi_t, S.d_phi_t);
				S.a_t = clamp_step(S.a_t, step_min, step_max);
				set_trial(S);
				S.phase = PH_MT_LOOP, S.with_hessian = 0, S.evaluations++;
				return;
			}
			if (S.step_iterations)
			{
				S.phase = PH_HESS, S.with_hessian = 1, S.evaluations++;
				return;
			}
			next = NEWTON_END;
		}
		else if (next == NEWTON_END)
		{
			for (int k = 0; k < 6; k++)
				S.p[k] = S.x0[k] + S.dir[k] * S.a_t;
			if (S.nr_iterations > o.max_iterations || (S.nr_iterations && fabs(S.a_t) < o.transformation_epsilon))
				S.converged = 1;
			S.nr_iterations++;
			if (S.converged)
			{
				S.trans_probability = S.score / o.n_src;
				S.running = 0;
				return;
			}
			next = NEWTON_START;
		}
		else
		{
			double delta[6];
			solve6(S.H, S.g, delta);
			double n2 = 0.0;
			for (int k = 0; k < 6; k++)
				n2 += delta[k] * delta[k];
			const double norm = sqrt(n2);
			if (norm == 0 || norm != norm)
			{
				S.trans_probability = S.score / o.n_src;
				S.converged = norm == norm ? 1 : 0;
				S.running = 0;
				return;
			}
			double d = 0.0;
			for (int k = 0; k < 6; k++)
			{
				S.dir[k] = delta[k] / norm;
				S.x0[k] = S.p[k];
				d += S.g[k] * S.dir[k];
			}
			S.phi_0 = -S.score;
			S.d_phi_0 = -d;
			S.step_iterations = 0;
			if (S.d_phi_0 >= 0)
			{
				if (S.d_phi_0 == 0)
				{
					S.a_t = 0.0;
					next = NEWTON_END;
					continue;
				}
				S.d_phi_0 = -S.d_phi_0;
				for (int k = 0; k < 6; k++)
					S.dir[k] = -S.dir[k];
				S.reversals++;
			}
			S.a_l = 0, S.a_u = 0;
			S.f_l = S.phi_0 - S.phi_0 - o.mu * S.d_phi_0 * S.a_l;
			S.g_l = S.d_phi_0 - o.mu * S.d_phi_0;
			S.f_u = S.phi_0 - S.phi_0 - o.mu * S.d_phi_0 * S.a_u;
			S.g_u = S.d_phi_0 - o.mu * S.d_phi_0;
			S.interval_converged = (step_max - step_min) > 0 ? 1 : 0; // (as upstream writes it: with step_min < step_max the inner loop never runs)
			S.open_interval = 1;
			S.a_t = clamp_step(norm, step_min, step_max);
			set_trial(S);
			S.phase = PH_MT_FIRST, S.with_hessian = 1, S.evaluations++;
			return;
		}
	}
	S.running = 0; // (not reached: every path above returns within four hops)
}
} // namespace ndt
