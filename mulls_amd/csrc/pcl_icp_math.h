// pcl_icp_math.h — the arithmetic of mulls_pcl_icp (include/mulls_hip.h has the definition, operation by operation), shared by the host
// (tests/pcl_icp_math_harness.cpp) and the device (k_pcl_icp.hip: a target point's normal, a pair's terms, the step and the stop rules).
// Every expression is written in the order the header states; the library is built without FMA contraction, and sin and cos come from detmath.h,
// so host and device give the same bits.  Nothing here calls the C library except sqrt and fabs, which are exact operations.
#pragma once
#include <cfloat>
#include <cmath>
#include <stdint.h>

#include "detmath.h"
#include "gicp_math.h"
#include "jacobi_rot.h"

namespace pcl_icp
{
enum Stop
{
	STOP_NONE = 0,
	STOP_ITERATIONS = 1,
	STOP_TRANSFORM = 2,
	STOP_ABS_MSE = 3,
	STOP_REL_MSE = 4,
	STOP_NO_CORRESPONDENCES = 5,
	STOP_SINGULAR = 6
};
enum Metric
{
	POINT2POINT = 0,
	POINT2PLANE = 1
};
// the 28 sums of an iteration.  Point-to-plane: the upper triangle of A^T A row by row (0 .. 20), A^T b (21 .. 26).  Point-to-point: the sum of the
// paired source points (0 .. 2), of their target points (3 .. 5), the cross-covariance of the demeaned pairs row-major (6 .. 14).  Both: the pairs' d2 (27).
enum
{
	SUM_S = 0,
	SUM_T = 3,
	SUM_H = 6,
	SUM_D2 = 27,
	N_SUMS = 28
};

using gicp::dot3;
using gicp::finite_d;

// the float squared distance of the correspondence search, the reciprocity test, the neighbourhoods and the fitness
MULLS_HD inline float dist2(float ax, float ay, float az, float bx, float by, float bz)
{
	const float dx = ax - bx, dy = ay - by, dz = az - bz;
	return (dx * dx + dy * dy) + dz * dz;
}
// (d2, index) order
MULLS_HD inline bool before(float da, uint32_t ia, float db, uint32_t ib) { return da < db || (da == db && ia < ib); }

// the cell of a coordinate: floor(x inv_edge) in double; *ok = 0 outside [-2^20, 2^20) (or not finite)
MULLS_HD inline int32_t cell_coord(float x, double inv_edge, int *ok)
{
	const double q = floor((double)x * inv_edge);
	if (!(q >= -1048576.0 && q < 1048576.0))
	{
		*ok = 0;
		return 0;
	}
	return (int32_t)q;
}

// The normal of a target point p from the scatter matrix S (xx xy xz yy yz zz) of its k >= 3 neighbours: the cyclic Jacobi rotations of jacobi_rot.h
// with the sweeps and the stopping rule of the NDT leaf, the column of the smallest eigenvalue (ties: the lower column index), made a unit vector,
// negated when n . (-p) < 0, stored as float; check_normal's (0.577, 0.577, 0.577) when it is not finite.
MULLS_HD inline void normal_of_scatter(const double *S, double px, double py, double pz, float *n)
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
	double e = a00, x = v00, y = v10, z = v20;
	if (a11 < e)
		e = a11, x = v01, y = v11, z = v21;
	if (a22 < e)
		e = a22, x = v02, y = v12, z = v22;
	const double nrm = sqrt((x * x + y * y) + z * z);
	x = x / nrm, y = y / nrm, z = z / nrm;
	if (dot3(x, y, z, -px, -py, -pz) < 0.0)
		x = -x, y = -y, z = -z;
	if (!finite_d(x) || !finite_d(y) || !finite_d(z))
	{
		n[0] = n[1] = n[2] = 0.577f;
		return;
	}
	n[0] = (float)x, n[1] = (float)y, n[2] = (float)z;
}
// the normal of a point from its neighbours in their order (xyz: k x 3 doubles); fewer than 3: (0.577, 0.577, 0.577).  The device's normals kernel
// expands the same two passes (gicp_math.h's sum_add, mean_of, scatter_add) over its tiles.
MULLS_HD inline void point_normal(const double *xyz, int k, double px, double py, double pz, float *n)
{
	if (k < 3)
	{
		n[0] = n[1] = n[2] = 0.577f;
		return;
	}
	double s[3] = {0.0, 0.0, 0.0}, m[3], S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	for (int j = 0; j < k; j++)
		gicp::sum_add(s, xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]);
	gicp::mean_of(s, k, m);
	for (int j = 0; j < k; j++)
		gicp::scatter_add(S, m, xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]);
	normal_of_scatter(S, px, py, pz, n);
}

// one pair of the point-to-plane step: a[28] += the upper triangle of row^T row (21), row^T b (6), with row = (s x n, n) and b = n . (t - s)
MULLS_HD inline void plane_term(const double *s, const double *t, const double *n, double *a)
{
	const double row[6] = {s[1] * n[2] - s[2] * n[1], s[2] * n[0] - s[0] * n[2], s[0] * n[1] - s[1] * n[0], n[0], n[1], n[2]};
	const double b = dot3(n[0], n[1], n[2], t[0] - s[0], t[1] - s[1], t[2] - s[2]);
	int at = 0;
	GICP_UNROLL
	for (int i = 0; i < 6; i++)
		GICP_UNROLL
	for (int k = i; k < 6; k++, at++)
		a[at] += row[i] * row[k];
	GICP_UNROLL
	for (int i = 0; i < 6; i++)
		a[21 + i] += row[i] * b;
}
// x = (alpha, beta, gamma, tx, ty, tz) by gicp_math.h's Cholesky; R = Rz(gamma) Ry(beta) Rx(alpha) row-major; -> 0 on a bad pivot or a non-finite x
MULLS_HD inline int plane_step(const double *sums, double *R, double *t)
{
	double x[6];
	if (!gicp::solve_step(sums, sums + 21, x))
		return 0;
	using mulls::det::cos_cr;
	using mulls::det::sin_cr;
	const double ca = cos_cr(x[0]), sa = sin_cr(x[0]), cb = cos_cr(x[1]), sb = sin_cr(x[1]), cg = cos_cr(x[2]), sg = sin_cr(x[2]);
	R[0] = cg * cb, R[1] = (-sg) * ca + (cg * sb) * sa, R[2] = sg * sa + (cg * sb) * ca;
	R[3] = sg * cb, R[4] = cg * ca + (sg * sb) * sa, R[5] = (-cg) * sa + (sg * sb) * ca;
	R[6] = -sb, R[7] = cb * sa, R[8] = cb * ca;
	t[0] = x[3], t[1] = x[4], t[2] = x[5];
	return 1;
}

// The rigid step from the cross-covariance H[a * 3 + b] = sum of s_a t_b over the demeaned pairs and the centroids: ransac_math.h's decomposition
// (Horn's symmetric 4 x 4, ten sweeps of cyclic Jacobi, the eigenvector of the largest diagonal entry as a unit quaternion), kept in double.
MULLS_HD inline void rigid_step(const double *H, const double *cs, const double *ct, double *Ro, double *to)
{
	const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
	double A[4][4], V[4][4];
	A[0][0] = (Sxx + Syy) + Szz;
	A[1][1] = (Sxx - Syy) - Szz;
	A[2][2] = (Syy - Sxx) - Szz;
	A[3][3] = (Szz - Sxx) - Syy;
	A[0][1] = A[1][0] = Syz - Szy;
	A[0][2] = A[2][0] = Szx - Sxz;
	A[0][3] = A[3][0] = Sxy - Syx;
	A[1][2] = A[2][1] = Sxy + Syx;
	A[1][3] = A[3][1] = Szx + Sxz;
	A[2][3] = A[3][2] = Syz + Szy;
	GICP_UNROLL
	for (int r = 0; r < 4; r++)
		GICP_UNROLL
	for (int c = 0; c < 4; c++)
		V[r][c] = r == c ? 1.0 : 0.0;
	for (int sweep = 0; sweep < 10; sweep++)
	{
		GICP_UNROLL
		for (int p = 0; p < 3; p++)
			GICP_UNROLL
		for (int q = p + 1; q < 4; q++)
		{
			const double apq = A[p][q];
			if (apq == 0.0)
				continue;
			const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
			double tn = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
			if (theta < 0.0)
				tn = -tn;
			const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
			GICP_UNROLL
			for (int k = 0; k < 4; k++) // A <- A J
			{
				const double akp = A[k][p], akq = A[k][q];
				A[k][p] = c * akp - s * akq;
				A[k][q] = s * akp + c * akq;
			}
			GICP_UNROLL
			for (int k = 0; k < 4; k++) // A <- J^T A
			{
				const double apk = A[p][k], aqk = A[q][k];
				A[p][k] = c * apk - s * aqk;
				A[q][k] = s * apk + c * aqk;
			}
			GICP_UNROLL
			for (int k = 0; k < 4; k++) // V <- V J
			{
				const double vkp = V[k][p], vkq = V[k][q];
				V[k][p] = c * vkp - s * vkq;
				V[k][q] = s * vkp + c * vkq;
			}
		}
	}
	double best = A[0][0], q0 = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
	GICP_UNROLL
	for (int k = 1; k < 4; k++)
		if (A[k][k] > best)
			best = A[k][k], q0 = V[0][k], qx = V[1][k], qy = V[2][k], qz = V[3][k];
	const double nrm = sqrt(((q0 * q0 + qx * qx) + qy * qy) + qz * qz);
	q0 = q0 / nrm, qx = qx / nrm, qy = qy / nrm, qz = qz / nrm;
	const double q00 = q0 * q0, qxx = qx * qx, qyy = qy * qy, qzz = qz * qz;
	const double qxy = qx * qy, qxz = qx * qz, qyz = qy * qz, q0x = q0 * qx, q0y = q0 * qy, q0z = q0 * qz;
	Ro[0] = ((q00 + qxx) - qyy) - qzz;
	Ro[1] = 2.0 * (qxy - q0z);
	Ro[2] = 2.0 * (qxz + q0y);
	Ro[3] = 2.0 * (qxy + q0z);
	Ro[4] = ((q00 - qxx) + qyy) - qzz;
	Ro[5] = 2.0 * (qyz - q0x);
	Ro[6] = 2.0 * (qxz - q0y);
	Ro[7] = 2.0 * (qyz + q0x);
	Ro[8] = ((q00 - qxx) - qyy) + qzz;
	GICP_UNROLL
	for (int r = 0; r < 3; r++)
		to[r] = ct[r] - dot3(Ro[3 * r], Ro[3 * r + 1], Ro[3 * r + 2], cs[0], cs[1], cs[2]);
}

// a stored point under a step: float(((R_r0 x + R_r1 y) + R_r2 z) + t_r)
MULLS_HD inline void move_stored(const double *R, const double *t, float *p)
{
	double a[3];
	gicp::move_point(R, t, p[0], p[1], p[2], a);
	p[0] = (float)a[0], p[1] = (float)a[1], p[2] = (float)a[2];
}

// the loop's state of one problem
struct State
{
	double R[9], t[3];	 // the pose reached so far, row-major
	double Rs[9], ts[3]; // the last step (the source is moved by it when `moved`)
	double mse, prev_mse;
	uint32_t n_corr;
	int32_t iterations, converged, stop, running, moved;
};
MULLS_HD inline void begin(State &S)
{
	for (int k = 0; k < 9; k++)
		S.R[k] = S.Rs[k] = k % 4 == 0 ? 1.0 : 0.0;
	for (int k = 0; k < 3; k++)
		S.t[k] = S.ts[k] = 0.0;
	S.mse = 0.0, S.prev_mse = DBL_MAX;
	S.n_corr = 0, S.iterations = 0, S.converged = 0, S.stop = STOP_NONE, S.running = 1, S.moved = 0;
}
MULLS_HD inline void end_with(State &S, int stop, int converged) { S.stop = stop, S.converged = converged, S.running = 0; }
// one iteration's end: the 28 sums and the number of pairs of this iteration.  S.moved = 1: the caller moves the stored source by (S.Rs, S.ts).
MULLS_HD inline void advance(State &S, int metric, const double *sums, uint32_t n_corr, int max_iter_num, double transformation_epsilon,
							 double euclidean_fitness_epsilon)
{
	S.n_corr = n_corr, S.moved = 0;
	S.mse = n_corr ? sums[SUM_D2] / (double)n_corr : 0.0;
	if (n_corr < 3u)
	{
		end_with(S, STOP_NO_CORRESPONDENCES, 0);
		return;
	}
	double Rs[9], ts[3];
	int ok = 1;
	if (metric == POINT2PLANE)
		ok = plane_step(sums, Rs, ts);
	else
	{
		const double dn = (double)n_corr;
		const double cs[3] = {sums[SUM_S] / dn, sums[SUM_S + 1] / dn, sums[SUM_S + 2] / dn};
		const double ct[3] = {sums[SUM_T] / dn, sums[SUM_T + 1] / dn, sums[SUM_T + 2] / dn};
		rigid_step(sums + SUM_H, cs, ct, Rs, ts);
	}
	if (ok)
	{
		for (int k = 0; k < 9; k++)
			if (!finite_d(Rs[k]))
				ok = 0;
		for (int k = 0; k < 3; k++)
			if (!finite_d(ts[k]))
				ok = 0;
	}
	if (!ok)
	{
		end_with(S, STOP_SINGULAR, 0);
		return;
	}
	// final = step * final
	double Rn[9], tn[3];
	gicp::mat3_mul(Rs, S.R, Rn);
	for (int r = 0; r < 3; r++)
		tn[r] = dot3(Rs[3 * r], Rs[3 * r + 1], Rs[3 * r + 2], S.t[0], S.t[1], S.t[2]) + ts[r];
	for (int k = 0; k < 9; k++)
		S.R[k] = Rn[k], S.Rs[k] = Rs[k];
	for (int k = 0; k < 3; k++)
		S.t[k] = tn[k], S.ts[k] = ts[k];
	S.moved = 1;
	S.iterations++;
	if (S.iterations >= max_iter_num)
	{
		end_with(S, STOP_ITERATIONS, 1);
		return;
	}
	const double cos_angle = 0.5 * (((Rs[0] + Rs[4]) + Rs[8]) - 1.0);
	const double t2 = (ts[0] * ts[0] + ts[1] * ts[1]) + ts[2] * ts[2];
	if (cos_angle >= 1.0 - transformation_epsilon && t2 <= transformation_epsilon)
	{
		end_with(S, STOP_TRANSFORM, 1);
		return;
	}
	const double d = fabs(S.mse - S.prev_mse);
	if (d < 1e-12)
	{
		end_with(S, STOP_ABS_MSE, 1);
		return;
	}
	if (d / S.prev_mse < euclidean_fitness_epsilon)
	{
		end_with(S, STOP_REL_MSE, 1);
		return;
	}
	S.prev_mse = S.mse;
}
} // namespace pcl_icp
