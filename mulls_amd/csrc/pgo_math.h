// pgo_math.h — the arithmetic of the pose graph optimisation (include/mulls_hip.h has the definition, line by line), shared by the host (pgo.cpp: the
// state of a node, the output poses, the edge check) and the device (k_pgo.hip: residual, Jacobians, the edge's blocks, update and projection).  Every
// expression is written in the order the header states; the library is built without FMA contraction, so host and device give the same bits.
#pragma once
#include <cmath>
#include <stdint.h>

#include "detmath.h"

namespace pgo
{
// Eigen's quaternion product, (x, y, z, w)
MULLS_HD inline void qmul(const double *p, const double *q, double *o)
{
	o[0] = ((p[3] * q[0] + p[0] * q[3]) + p[1] * q[2]) - p[2] * q[1];
	o[1] = ((p[3] * q[1] + p[1] * q[3]) + p[2] * q[0]) - p[0] * q[2];
	o[2] = ((p[3] * q[2] + p[2] * q[3]) + p[0] * q[1]) - p[1] * q[0];
	o[3] = ((p[3] * q[3] - p[0] * q[0]) - p[1] * q[1]) - p[2] * q[2];
}
MULLS_HD inline void qnormalise(double *q)
{
	const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
	q[0] = q[0] / n, q[1] = q[1] / n, q[2] = q[2] / n, q[3] = q[3] / n;
}
// Eigen's toRotationMatrix, row-major R[3 r + c]
MULLS_HD inline void qrot(const double *q, double *R)
{
	const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
	const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
	const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
	const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
	R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
	R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
	R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}
// Eigen's matrix -> quaternion of a row-major 3 x 3, then the normalisation
inline void rot2quat(const double *m, double *q)
{
	double t = (m[0] + m[4]) + m[8];
	if (t > 0.0)
	{
		t = sqrt(t + 1.0);
		q[3] = 0.5 * t;
		t = 0.5 / t;
		q[0] = (m[7] - m[5]) * t, q[1] = (m[2] - m[6]) * t, q[2] = (m[3] - m[1]) * t;
	}
	else
	{
		int i = 0;
		if (m[4] > m[0])
			i = 1;
		if (m[8] > m[4 * i])
			i = 2;
		const int j = (i + 1) % 3, k = (j + 1) % 3;
		t = sqrt(((m[4 * i] - m[4 * j]) - m[4 * k]) + 1.0);
		q[i] = 0.5 * t;
		t = 0.5 / t;
		q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
		q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
		q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
	}
	qnormalise(q);
}
// x[7] = t, q of a column-major 4 x 4
inline void pose2state(const double *T, double *x)
{
	double m[9];
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 3; c++)
			m[3 * r + c] = T[r + 4 * c];
	x[0] = T[12], x[1] = T[13], x[2] = T[14];
	rot2quat(m, x + 3);
}
inline void state2pose(const double *x, double *T)
{
	double q[4] = {x[3], x[4], x[5], x[6]}, R[9];
	qnormalise(q);
	qrot(q, R);
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 3; c++)
			T[r + 4 * c] = R[3 * r + c];
	T[12] = x[0], T[13] = x[1], T[14] = x[2];
	T[3] = T[7] = T[11] = 0.0, T[15] = 1.0;
}

// residual e[6] of an edge (th, qh) between states xa, xb; R = R(q_a), v = R^T (t_b - t_a), P and Q as the header names them
MULLS_HD inline void residual(const double *xa, const double *xb, const double *th, const double *qh, double *e, double *R, double *v, double *P, double *Q)
{
	qrot(xa + 3, R);
	const double d0 = xb[0] - xa[0], d1 = xb[1] - xa[1], d2 = xb[2] - xa[2];
#pragma unroll
	for (int r = 0; r < 3; r++)
	{
		v[r] = (R[r] * d0 + R[3 + r] * d1) + R[6 + r] * d2;
		e[r] = v[r] - th[r];
	}
	const double qac[4] = {-xa[3], -xa[4], -xa[5], xa[6]};
	double qab[4];
	qmul(qac, xb + 3, qab);
	Q[0] = -qab[0], Q[1] = -qab[1], Q[2] = -qab[2], Q[3] = qab[3];
	qmul(qh, Q, P);
	e[3] = 2.0 * P[0], e[4] = 2.0 * P[1], e[5] = 2.0 * P[2];
}
// s = e^T W e (W row-major, symmetric) and u = W e
MULLS_HD inline double weighted_square(const double *W, const double *e, double *u)
{
	double s = 0.0;
#pragma unroll
	for (int k = 0; k < 6; k++)
	{
		double a = 0.0;
#pragma unroll
		for (int l = 0; l < 6; l++)
			a += W[6 * k + l] * e[l];
		u[k] = a;
	}
#pragma unroll
	for (int k = 0; k < 6; k++)
		s += e[k] * u[k];
	return s;
}
// rho(s) and the edge's weight w
MULLS_HD inline double robust(double s, int robustify, double delta, double *w)
{
	*w = 1.0;
	const double d2 = delta * delta;
	if (robustify && s > d2)
	{
		const double r = sqrt(s);
		*w = delta / r;
		return (2.0 * delta) * r - d2;
	}
	return s;
}
// the two Jacobians, row-major 6 x 6 (rows: residual)
MULLS_HD inline void jacobians(const double *R, const double *v, const double *P, const double *Q, const double *qh, double *Ja, double *Jb)
{
#pragma unroll
	for (int i = 0; i < 36; i++)
		Ja[i] = 0.0, Jb[i] = 0.0;
#pragma unroll
	for (int r = 0; r < 3; r++)
#pragma unroll
		for (int c = 0; c < 3; c++)
		{
			Ja[6 * r + c] = -R[3 * c + r];
			Jb[6 * r + c] = R[3 * c + r];
		}
	Ja[6 * 0 + 4] = -v[2], Ja[6 * 0 + 5] = v[1];
	Ja[6 * 1 + 3] = v[2], Ja[6 * 1 + 5] = -v[0];
	Ja[6 * 2 + 3] = -v[1], Ja[6 * 2 + 4] = v[0];
#pragma unroll
	for (int c = 0; c < 3; c++)
	{
		const double E[4] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0, 0.0};
		double A[4], T[4], B[4];
		qmul(P, E, A);
		qmul(qh, E, T);
		qmul(T, Q, B);
#pragma unroll
		for (int r = 0; r < 3; r++)
		{
			Ja[6 * (3 + r) + 3 + c] = A[r];
			Jb[6 * (3 + r) + 3 + c] = -B[r];
		}
	}
}
// the candidate of a node: update by d[6], then the projection onto its box around x0 (boxed: 0 / 1)
MULLS_HD inline void step_node(const double *x, const double *d, const double *x0, int boxed, double tl, double rl, int only_translation, double *o)
{
	o[0] = x[0] + d[0], o[1] = x[1] + d[1], o[2] = x[2] + d[2];
	const double dq[4] = {d[3] * 0.5, d[4] * 0.5, d[5] * 0.5, 1.0};
	double q[4];
	qmul(x + 3, dq, q);
	qnormalise(q);
	if (boxed)
	{
#pragma unroll
		for (int c = 0; c < 3; c++)
		{
			const double lo = x0[c] - tl, hi = x0[c] + tl;
			double t = o[c] < lo ? lo : o[c];
			o[c] = t > hi ? hi : t;
		}
		if (!only_translation)
		{
			const double dot = ((q[0] * x0[3] + q[1] * x0[4]) + q[2] * x0[5]) + q[3] * x0[6];
			if (dot < 0.0)
				q[0] = -q[0], q[1] = -q[1], q[2] = -q[2], q[3] = -q[3];
#pragma unroll
			for (int c = 0; c < 4; c++)
			{
				const double lo = x0[3 + c] - rl, hi = x0[3 + c] + rl;
				double t = q[c] < lo ? lo : q[c];
				q[c] = t > hi ? hi : t;
			}
			qnormalise(q);
		}
	}
	o[3] = q[0], o[4] = q[1], o[5] = q[2], o[6] = q[3];
}
} // namespace pgo
