// teaser_math.h — the arithmetic of the TEASER coarse registration (include/mulls_hip.h: mulls_coarse_reg_teaser), one text for the
// device kernels (k_teaser.hip) and for a CPU build (tests/teaser_harness.cpp, which tests/test_teaser.py holds against the numpy restatement bit for bit).
// Everything is double, only + - * / sqrt (and fabs, comparisons), built without contraction; every sum's order is written out here.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TEASER_HD __host__ __device__
#define TEASER_UNROLL _Pragma("unroll")
#else
#define TEASER_HD
#define TEASER_UNROLL
#endif

#define MULLS_TEASER_MAX_POINTS 8192u
#define MULLS_TEASER_PARTIALS 4096u // the strided partial sums of H and of the cost: part of the definition, not a tuning knob
#define MULLS_TEASER_GNC_MAX_ITER 100
#define MULLS_TEASER_GNC_FACTOR 1.4
#define MULLS_TEASER_COST_THRESHOLD 0.005

// |d| = sqrt((dx^2 + dy^2) + dz^2)
TEASER_HD inline double teaser_norm3(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }

// the consistency test of pairs i and j (x, y, z of each point, float, widened first): | |s_j - s_i| - |t_j - t_i| | <= beta.  The squares make it
// the same bits for (i, j) and (j, i); a NaN gives no edge.
TEASER_HD inline bool teaser_edge(const float *si, const float *ti, const float *sj, const float *tj, double beta)
{
	const double ds = teaser_norm3((double)sj[0] - (double)si[0], (double)sj[1] - (double)si[1], (double)sj[2] - (double)si[2]);
	const double dt = teaser_norm3((double)tj[0] - (double)ti[0], (double)tj[1] - (double)ti[1], (double)tj[2] - (double)ti[2]);
	return fabs(ds - dt) <= beta;
}

// measurement k of a clique of C vertices is the pair (a, b), a < b, rows a ascending, b ascending within a row
TEASER_HD inline uint64_t teaser_row_start(uint32_t a, uint32_t C) { return (uint64_t)a * (2ull * C - a - 1ull) / 2ull; }
TEASER_HD inline void teaser_decode(uint64_t k, uint32_t C, uint32_t *a, uint32_t *b)
{
	// the largest a with row_start(a) <= k, by bisection: at most 14 steps for C <= 8192
	uint32_t lo = 0, hi = C - 2u;
	for (int it = 0; it < 16 && lo < hi; it++)
	{
		const uint32_t mid = (lo + hi + 1u) / 2u;
		if (teaser_row_start(mid, C) <= k)
			lo = mid;
		else
			hi = mid - 1u;
	}
	*a = lo;
	*b = lo + 1u + (uint32_t)(k - teaser_row_start(lo, C));
}

// r = |b - R a|^2, R row-major
TEASER_HD inline double teaser_resid(const double *R, const double *a, const double *b)
{
	const double dx = b[0] - ((R[0] * a[0] + R[1] * a[1]) + R[2] * a[2]);
	const double dy = b[1] - ((R[3] * a[0] + R[4] * a[1]) + R[5] * a[2]);
	const double dz = b[2] - ((R[6] * a[0] + R[7] * a[1]) + R[8] * a[2]);
	return (dx * dx + dy * dy) + dz * dz;
}

// the GNC-TLS weight of a residual
TEASER_HD inline double teaser_weight(double r, double mu, double nb2)
{
	const double th1 = ((mu + 1.0) / mu) * nb2, th2 = (mu / (mu + 1.0)) * nb2;
	if (r >= th1)
		return 0.0;
	if (r <= th2)
		return 1.0;
	return sqrt(((nb2 * mu) * (mu + 1.0)) / r) - mu;
}

// mu of iteration 0
TEASER_HD inline double teaser_mu0(double max_r, double nb2) { return 1.0 / ((2.0 * max_r) / nb2 - 1.0); }

// the pairwise tree over the MULLS_TEASER_PARTIALS partial sums, in place: p[t] += p[t + s] for s = PARTIALS / 2, ..., 1 (the CPU form; the device runs the
// same additions in teaser_fit / teaser_cost of k_teaser.hip)
inline double teaser_tree_host(double *p)
{
	for (uint32_t s = MULLS_TEASER_PARTIALS / 2u; s > 0; s >>= 1)
		for (uint32_t t = 0; t < s; t++)
			p[t] = p[t] + p[t + s];
	return p[0];
}

// The rotation of H[a * 3 + b] = sum of w s_a t_b (t ~ R s): Horn's symmetric 4 x 4, ten sweeps of cyclic Jacobi over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3),
// the column of the largest diagonal entry (the first among equals) as a unit quaternion, its rotation matrix, row-major: the operations of
// ransac_math.h horn_fit, steps 2 - 5, with nothing rounded to float.
TEASER_HD inline void teaser_horn_rot(const double *H, double *Rout)
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
TEASER_UNROLL
	for (int r = 0; r < 4; r++)
TEASER_UNROLL
		for (int c = 0; c < 4; c++)
			V[r][c] = r == c ? 1.0 : 0.0;
	for (int sweep = 0; sweep < 10; sweep++)
	{
TEASER_UNROLL
		for (int p = 0; p < 3; p++)
TEASER_UNROLL
			for (int q = p + 1; q < 4; q++)
			{
				const double apq = A[p][q];
				if (apq == 0.0)
					continue;
				const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
				double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
				if (theta < 0.0)
					t = -t;
				const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
TEASER_UNROLL
				for (int k = 0; k < 4; k++) // A <- A J
				{
					const double akp = A[k][p], akq = A[k][q];
					A[k][p] = c * akp - s * akq;
					A[k][q] = s * akp + c * akq;
				}
TEASER_UNROLL
				for (int k = 0; k < 4; k++) // A <- J^T A
				{
					const double apk = A[p][k], aqk = A[q][k];
					A[p][k] = c * apk - s * aqk;
					A[q][k] = s * apk + c * aqk;
				}
TEASER_UNROLL
				for (int k = 0; k < 4; k++) // V <- V J
				{
					const double vkp = V[k][p], vkq = V[k][q];
					V[k][p] = c * vkp - s * vkq;
					V[k][q] = s * vkp + c * vkq;
				}
			}
	}
	double best = A[0][0], q0 = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
TEASER_UNROLL
	for (int k = 1; k < 4; k++)
		if (A[k][k] > best)
			best = A[k][k], q0 = V[0][k], qx = V[1][k], qy = V[2][k], qz = V[3][k];
	const double nrm = sqrt(((q0 * q0 + qx * qx) + qy * qy) + qz * qz);
	q0 = q0 / nrm, qx = qx / nrm, qy = qy / nrm, qz = qz / nrm;
	const double q00 = q0 * q0, qxx = qx * qx, qyy = qy * qy, qzz = qz * qz;
	const double qxy = qx * qy, qxz = qx * qz, qyz = qy * qz, q0x = q0 * qx, q0y = q0 * qy, q0z = q0 * qz;
	Rout[0] = ((q00 + qxx) - qyy) - qzz;
	Rout[1] = 2.0 * (qxy - q0z);
	Rout[2] = 2.0 * (qxz + q0y);
	Rout[3] = 2.0 * (qxy + q0z);
	Rout[4] = ((q00 - qxx) + qyy) - qzz;
	Rout[5] = 2.0 * (qyz - q0x);
	Rout[6] = 2.0 * (qxz - q0y);
	Rout[7] = 2.0 * (qyz + q0x);
	Rout[8] = ((q00 - qxx) - qyy) + qzz;
}

// the state of the GNC loop that the device keeps and the host reads once per iteration
struct TeaserGnc
{
	double R[9];
	double mu, prev_cost, cost, max_r;
	uint32_t stop;	   // 0: go on; 1: mu <= 0 in iteration 0 (no weight update follows); 2: the cost settled (the weight update of this iteration still runs)
	uint32_t n_inlier; // weights >= 0.5 after the last update
};

// what follows the residuals of iteration `iter` (steps 3, 4 and 6 of the definition): S holds R; cost and max_r are this iteration's.  Sets S.mu to the
// value the weight update uses; S.stop; and after the update the caller multiplies mu by the factor (teaser_gnc_next).
TEASER_HD inline void teaser_gnc_decide(TeaserGnc *S, int iter, double cost, double max_r, double nb2)
{
	S->max_r = max_r;
	S->stop = 0;
	if (iter == 0)
	{
		S->prev_cost = INFINITY;
		S->cost = 0.0;
		S->mu = teaser_mu0(max_r, nb2);
		if (S->mu <= 0.0)
		{
			S->stop = 1;
			return;
		}
	}
	S->cost = cost;
	if (fabs(cost - S->prev_cost) < MULLS_TEASER_COST_THRESHOLD)
		S->stop = 2;
}
TEASER_HD inline void teaser_gnc_next(TeaserGnc *S)
{
	S->mu = MULLS_TEASER_GNC_FACTOR * S->mu;
	S->prev_cost = S->cost;
}
