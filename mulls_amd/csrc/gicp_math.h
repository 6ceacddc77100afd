// gicp_math.h — the arithmetic of mulls_gicp (include/mulls_hip.h has the definition, operation by operation), shared by the host
// (tests/gicp_math_harness.cpp) and the device (k_gicp.hip: a point's covariance, the evaluation of a source point, the Gauss-Newton step).
// Every expression is written in the order the header states; the library is built without FMA contraction, and sin and atan2 come from detmath.h,
// so host and device give the same bits.  Nothing here calls the C library except sqrt and fabs, which are exact operations.
#pragma once
#include <cmath>
#include <stdint.h>

#include "detmath.h"
#include "jacobi_rot.h"

#if defined(__HIPCC__)
#define GICP_UNROLL _Pragma("unroll")
#else
#define GICP_UNROLL
#endif

namespace gicp
{
enum Stop
{
	STOP_NONE = 0,
	STOP_CONVERGED = 1,
	STOP_MAX_ITERATIONS = 2,
	STOP_SINGULAR = 3
};

MULLS_HD inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
MULLS_HD inline bool finite_d(double v) { return v - v == 0.0; }

// PLANE regularisation of a scatter matrix S (xx xy xz yy yz zz): the cyclic Jacobi rotations of jacobi_rot.h with the sweeps and the stopping rule of
// the NDT leaf, the eigenvalues descending (ties by column index ascending), C = (v0 v0^T + v1 v1^T) + 0.01 v2 v2^T
MULLS_HD inline void plane_covariance(const double *S, double *C)
{
	double a00 = S[0], a01 = S[1], a02 = S[2], a11 = S[3], a12 = S[4], a22 = S[5];
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
	double e0 = a00, e1 = a11, e2 = a22;
	int i0 = 0, i1 = 1, i2 = 2;
	double x0 = v00, y0 = v10, z0 = v20, x1 = v01, y1 = v11, z1 = v21, x2 = v02, y2 = v12, z2 = v22;
#define MULLS_GICP_SWAP(ea, eb, ia, ib, xa, ya, za, xb, yb, zb) \
	if (eb > ea || (eb == ea && ib < ia))                        \
	{                                                            \
		double w = ea;                                           \
		ea = eb, eb = w;                                         \
		const int iw = ia;                                       \
		ia = ib, ib = iw;                                        \
		w = xa, xa = xb, xb = w;                                 \
		w = ya, ya = yb, yb = w;                                 \
		w = za, za = zb, zb = w;                                 \
	}
	MULLS_GICP_SWAP(e0, e1, i0, i1, x0, y0, z0, x1, y1, z1)
	MULLS_GICP_SWAP(e0, e2, i0, i2, x0, y0, z0, x2, y2, z2)
	MULLS_GICP_SWAP(e1, e2, i1, i2, x1, y1, z1, x2, y2, z2)
#undef MULLS_GICP_SWAP
	C[0] = (x0 * x0 + x1 * x1) + 0.01 * (x2 * x2);
	C[1] = (x0 * y0 + x1 * y1) + 0.01 * (x2 * y2);
	C[2] = (x0 * z0 + x1 * z1) + 0.01 * (x2 * z2);
	C[3] = (y0 * y0 + y1 * y1) + 0.01 * (y2 * y2);
	C[4] = (y0 * z0 + y1 * z1) + 0.01 * (y2 * z2);
	C[5] = (z0 * z0 + z1 * z1) + 0.01 * (z2 * z2);
}

// the two passes over a point's neighbours, one neighbour at a time in the neighbours' order: the sum s[3], then, with m = s / k, the scatter S[6].
// The host's point_covariance and the two device tails (k_gicp.hip: the register list, the brute-force list) expand this text.
MULLS_HD inline void sum_add(double *s, double x, double y, double z) { s[0] += x, s[1] += y, s[2] += z; }
MULLS_HD inline void mean_of(const double *s, int k, double *m) { m[0] = s[0] / (double)k, m[1] = s[1] / (double)k, m[2] = s[2] / (double)k; }
MULLS_HD inline void scatter_add(double *S, const double *m, double x, double y, double z)
{
	const double d0 = x - m[0], d1 = y - m[1], d2 = z - m[2];
	S[0] += d0 * d0, S[1] += d0 * d1, S[2] += d0 * d2, S[3] += d1 * d1, S[4] += d1 * d2, S[5] += d2 * d2;
}
// the covariance of a point from its k neighbours in their order.  xyz: k x 3 doubles
MULLS_HD inline void point_covariance(const double *xyz, int k, double *C)
{
	double s[3] = {0.0, 0.0, 0.0}, m[3], S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	for (int j = 0; j < k; j++)
		sum_add(s, xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]);
	mean_of(s, k, m);
	for (int j = 0; j < k; j++)
		scatter_add(S, m, xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]);
	plane_covariance(S, C);
}

// R = exp(w), row-major
MULLS_HD inline void so3_exp(const double *w, double *R)
{
	const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
	if (th == 0.0)
	{
		R[0] = 1.0, R[1] = 0.0, R[2] = 0.0, R[3] = 0.0, R[4] = 1.0, R[5] = 0.0, R[6] = 0.0, R[7] = 0.0, R[8] = 1.0;
		return;
	}
	const double a = mulls::det::sin_cr(th) / th;
	const double s = mulls::det::sin_cr(th / 2.0);
	const double b = ((2.0 * s) * s) / (th * th);
	const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
	const double K2[9] = {-(w[1] * w[1] + w[2] * w[2]), w[0] * w[1], w[0] * w[2], w[0] * w[1], -(w[0] * w[0] + w[2] * w[2]), w[1] * w[2],
						  w[0] * w[2], w[1] * w[2], -(w[0] * w[0] + w[1] * w[1])};
	GICP_UNROLL
	for (int k = 0; k < 9; k++)
		R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + a * K[k]) + b * K2[k];
}
// w = log(R); rotations near pi are outside the definition
MULLS_HD inline void so3_log(const double *R, double *w)
{
	const double w0 = (R[7] - R[5]) / 2.0, w1 = (R[2] - R[6]) / 2.0, w2 = (R[3] - R[1]) / 2.0;
	const double c = (((R[0] + R[4]) + R[8]) - 1.0) / 2.0;
	const double n = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
	if (n == 0.0)
	{
		w[0] = w[1] = w[2] = 0.0;
		return;
	}
	const double f = mulls::det::atan2_cr(n, c) / n;
	w[0] = w0 * f, w[1] = w1 * f, w[2] = w2 * f;
}
MULLS_HD inline void mat3_mul(const double *A, const double *B, double *O)
{
	GICP_UNROLL
	for (int i = 0; i < 3; i++)
		GICP_UNROLL
	for (int j = 0; j < 3; j++)
		O[3 * i + j] = dot3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]);
}

// a' = R a + t in double
MULLS_HD inline void move_point(const double *R, const double *t, float x, float y, float z, double *a)
{
	const double dx = (double)x, dy = (double)y, dz = (double)z;
	a[0] = dot3(R[0], R[1], R[2], dx, dy, dz) + t[0];
	a[1] = dot3(R[3], R[4], R[5], dx, dy, dz) + t[1];
	a[2] = dot3(R[6], R[7], R[8], dx, dy, dz) + t[2];
}

// the voxel coordinate of a float: floor(x / resolution - 0.5), in float; *ok = 0 when it is not finite or outside [-2^20, 2^20)
MULLS_HD inline int32_t voxel_coord(float x, float resolution, int *ok)
{
	const float q = floorf(x / resolution - 0.5f);
	if (!(q >= -1048576.0f && q < 1048576.0f))
	{
		*ok = 0;
		return 0;
	}
	return (int32_t)q;
}
// three 21-bit fields
MULLS_HD inline uint64_t pack_coords(int32_t cx, int32_t cy, int32_t cz)
{
	return (uint64_t)(uint32_t)(cx + 1048576) | ((uint64_t)(uint32_t)(cy + 1048576) << 21) | ((uint64_t)(uint32_t)(cz + 1048576) << 42);
}
// the home slot of a key: the top bits of a 64-bit mix (k_sor.hip's); shift = 64 - log2(slots)
MULLS_HD inline uint32_t home_slot(uint64_t key, uint32_t shift)
{
	uint64_t z = key;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	z = z ^ (z >> 31);
	return (uint32_t)(z >> shift);
}

// One source point that has a voxel: a[28] += the upper triangle of J^T J (21, row by row), J^T e (6), e . e (1).
// ap: the moved point; CA: the point's covariance (xx xy xz yy yz zz); mean, CB: the voxel's; R: the rotation, row-major
MULLS_HD inline void point_term(const double *ap, const double *CA, const double *mean, const double *CB, const double *R, double *a)
{
	const double c[3][3] = {{CA[0], CA[1], CA[2]}, {CA[1], CA[3], CA[4]}, {CA[2], CA[4], CA[5]}};
	double RC[3][3];
	GICP_UNROLL
	for (int i = 0; i < 3; i++)
		GICP_UNROLL
	for (int j = 0; j < 3; j++)
		RC[i][j] = dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], c[0][j], c[1][j], c[2][j]);
	// the upper triangle of M = CB + R CA R^T, mirrored
#define MULLS_GICP_M(i, j, b) (CB[b] + dot3(RC[i][0], RC[i][1], RC[i][2], R[3 * j], R[3 * j + 1], R[3 * j + 2]))
	const double c00 = MULLS_GICP_M(0, 0, 0), c01 = MULLS_GICP_M(0, 1, 1), c02 = MULLS_GICP_M(0, 2, 2);
	const double c11 = MULLS_GICP_M(1, 1, 3), c12 = MULLS_GICP_M(1, 2, 4), c22 = MULLS_GICP_M(2, 2, 5);
#undef MULLS_GICP_M
	const double k00 = c11 * c22 - c12 * c12, k01 = c02 * c12 - c01 * c22, k02 = c01 * c12 - c02 * c11;
	const double k11 = c00 * c22 - c02 * c02, k12 = c01 * c02 - c00 * c12, k22 = c00 * c11 - c01 * c01;
	const double det = (c00 * k00 + c01 * k01) + c02 * k02;
	const double W[3][3] = {{k00 / det, k01 / det, k02 / det}, {k01 / det, k11 / det, k12 / det}, {k02 / det, k12 / det, k22 / det}};
	const double d0 = mean[0] - ap[0], d1 = mean[1] - ap[1], d2 = mean[2] - ap[2];
	double e[3], J[3][6];
	GICP_UNROLL
	for (int i = 0; i < 3; i++)
	{
		e[i] = dot3(W[i][0], W[i][1], W[i][2], d0, d1, d2);
		J[i][0] = W[i][1] * ap[2] - W[i][2] * ap[1];
		J[i][1] = W[i][2] * ap[0] - W[i][0] * ap[2];
		J[i][2] = W[i][0] * ap[1] - W[i][1] * ap[0];
		J[i][3] = -W[i][0], J[i][4] = -W[i][1], J[i][5] = -W[i][2];
	}
	int at = 0;
	GICP_UNROLL
	for (int i = 0; i < 6; i++)
		GICP_UNROLL
	for (int k = i; k < 6; k++, at++)
		a[at] += dot3(J[0][i], J[1][i], J[2][i], J[0][k], J[1][k], J[2][k]);
	GICP_UNROLL
	for (int i = 0; i < 6; i++)
		a[21 + i] += dot3(J[0][i], J[1][i], J[2][i], e[0], e[1], e[2]);
	a[27] += dot3(e[0], e[1], e[2], e[0], e[1], e[2]);
}

// delta = (J^T J)^-1 J^T e by Cholesky: L by columns, every sum subtracted term by term in ascending index; -> 0 when a pivot is not positive and
// finite or delta is not finite
MULLS_HD inline int solve_step(const double *Hu, const double *b, double *delta)
{
	double L[6][6];
	{
		int at = 0;
		GICP_UNROLL
		for (int i = 0; i < 6; i++)
			GICP_UNROLL
		for (int k = i; k < 6; k++, at++)
		{
			L[i][k] = 0.0;
			L[k][i] = Hu[at];
		}
	}
	int ok = 1;
	GICP_UNROLL
	for (int j = 0; j < 6; j++)
	{
		double s = L[j][j];
		GICP_UNROLL
		for (int k = 0; k < j; k++)
			s -= L[j][k] * L[j][k];
		if (!(s > 0.0) || !finite_d(s))
			ok = 0;
		const double piv = sqrt(s);
		L[j][j] = piv;
		GICP_UNROLL
		for (int i = j + 1; i < 6; i++)
		{
			double v = L[i][j];
			GICP_UNROLL
			for (int k = 0; k < j; k++)
				v -= L[i][k] * L[j][k];
			L[i][j] = v / piv;
		}
	}
	double y[6];
	GICP_UNROLL
	for (int i = 0; i < 6; i++)
	{
		double v = b[i];
		GICP_UNROLL
		for (int k = 0; k < i; k++)
			v -= L[i][k] * y[k];
		y[i] = v / L[i][i];
	}
	GICP_UNROLL
	for (int i = 5; i >= 0; i--)
	{
		double v = y[i];
		GICP_UNROLL
		for (int k = i + 1; k < 6; k++)
			v -= L[k][i] * delta[k];
		delta[i] = v / L[i][i];
	}
	GICP_UNROLL
	for (int i = 0; i < 6; i++)
		if (!finite_d(delta[i]))
			ok = 0;
	return ok;
}

// the loop's state of one problem
struct State
{
	double r[3], t[3]; // x
	double R[9];	   // exp(r), row-major
	double loss;
	uint32_t n_corr;
	int32_t iterations, converged, stop, running;
	int32_t pad;
};
MULLS_HD inline void begin(State &S, const float *start_rotvec)
{
	for (int k = 0; k < 3; k++)
		S.r[k] = (double)start_rotvec[k], S.t[k] = 0.0;
	so3_exp(S.r, S.R);
	S.loss = 0.0, S.n_corr = 0, S.iterations = 0, S.converged = 0, S.stop = STOP_NONE, S.running = 1, S.pad = 0;
}
// one iteration's end: the 28 sums and the count of the evaluation at S's x
MULLS_HD inline void advance(State &S, const double *sums, uint32_t n_corr, int max_iterations, double rotation_epsilon, double transformation_epsilon)
{
	S.loss = sums[27], S.n_corr = n_corr;
	double delta[6];
	if (!n_corr || !solve_step(sums, sums + 21, delta))
	{
		S.stop = STOP_SINGULAR, S.running = 0;
		return;
	}
	const double md[3] = {-delta[0], -delta[1], -delta[2]};
	double E[9], Rn[9];
	so3_exp(md, E);
	mat3_mul(E, S.R, Rn);
	so3_log(Rn, S.r);
	so3_exp(S.r, S.R);
	for (int k = 0; k < 3; k++)
		S.t[k] -= delta[3 + k];
	so3_exp(delta, E);
	double mr = 0.0, mt = 0.0;
	for (int k = 0; k < 9; k++)
	{
		const double v = fabs(E[k] - (k % 4 == 0 ? 1.0 : 0.0));
		mr = v > mr ? v : mr;
	}
	for (int k = 0; k < 3; k++)
	{
		const double v = fabs(delta[3 + k]);
		mt = v > mt ? v : mt;
	}
	const double qr = mr / rotation_epsilon, qt = mt / transformation_epsilon;
	if ((qr > qt ? qr : qt) < 1.0)
	{
		S.converged = 1, S.stop = STOP_CONVERGED, S.running = 0;
		return;
	}
	if (S.iterations + 1 >= max_iterations)
	{
		S.stop = STOP_MAX_ITERATIONS, S.running = 0;
		return;
	}
	S.iterations++;
}
} // namespace gicp
