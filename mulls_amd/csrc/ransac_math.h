// ransac_math.h — the rigid-transform estimator of the RANSAC coarse registration (include/mulls_hip.h), one text for the device
// kernels (k_ransac.hip; k_fpfh.hip's SAC-IA hypotheses call fit_three_pairs as well) and for a CPU build (tests/ransac_harness.cpp, which tests/test_ransac.py holds against the numpy restatement bit for bit).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RANSAC_HD __host__ __device__
#define RANSAC_UNROLL _Pragma("unroll")
#else
#define RANSAC_HD
#define RANSAC_UNROLL
#endif

// The estimator's decomposition (this library's definition): H[a * 3 + b] = sum of s_a t_b over the demeaned pairs, cs / ct the centroids.
// Horn's symmetric 4 x 4, ten sweeps of cyclic Jacobi, the eigenvector of the largest diagonal entry as a unit quaternion, R, t = ct - R cs.
RANSAC_HD inline void horn_fit(const double *H, const double *cs, const double *ct, float *out)
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
RANSAC_UNROLL
	for (int r = 0; r < 4; r++)
RANSAC_UNROLL
		for (int c = 0; c < 4; c++)
			V[r][c] = r == c ? 1.0 : 0.0;
	for (int sweep = 0; sweep < 10; sweep++)
	{
RANSAC_UNROLL
		for (int p = 0; p < 3; p++)
RANSAC_UNROLL
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
RANSAC_UNROLL
				for (int k = 0; k < 4; k++) // A <- A J
				{
					const double akp = A[k][p], akq = A[k][q];
					A[k][p] = c * akp - s * akq;
					A[k][q] = s * akp + c * akq;
				}
RANSAC_UNROLL
				for (int k = 0; k < 4; k++) // A <- J^T A
				{
					const double apk = A[p][k], aqk = A[q][k];
					A[p][k] = c * apk - s * aqk;
					A[q][k] = s * apk + c * aqk;
				}
RANSAC_UNROLL
				for (int k = 0; k < 4; k++) // V <- V J
				{
					const double vkp = V[k][p], vkq = V[k][q];
					V[k][p] = c * vkp - s * vkq;
					V[k][q] = s * vkp + c * vkq;
				}
			}
	}
	double best = A[0][0], q0 = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
RANSAC_UNROLL
	for (int k = 1; k < 4; k++)
		if (A[k][k] > best)
			best = A[k][k], q0 = V[0][k], qx = V[1][k], qy = V[2][k], qz = V[3][k];
	const double nrm = sqrt(((q0 * q0 + qx * qx) + qy * qy) + qz * qz);
	q0 = q0 / nrm, qx = qx / nrm, qy = qy / nrm, qz = qz / nrm;
	const double q00 = q0 * q0, qxx = qx * qx, qyy = qy * qy, qzz = qz * qz;
	const double qxy = qx * qy, qxz = qx * qz, qyz = qy * qz, q0x = q0 * qx, q0y = q0 * qy, q0z = q0 * qz;
	double R[3][3];
	R[0][0] = ((q00 + qxx) - qyy) - qzz;
	R[0][1] = 2.0 * (qxy - q0z);
	R[0][2] = 2.0 * (qxz + q0y);
	R[1][0] = 2.0 * (qxy + q0z);
	R[1][1] = ((q00 - qxx) + qyy) - qzz;
	R[1][2] = 2.0 * (qyz - q0x);
	R[2][0] = 2.0 * (qxz - q0y);
	R[2][1] = 2.0 * (qyz + q0x);
	R[2][2] = ((q00 - qxx) - qyy) + qzz;
RANSAC_UNROLL
	for (int r = 0; r < 3; r++)
	{
		const double tr = ct[r] - ((R[r][0] * cs[0] + R[r][1] * cs[1]) + R[r][2] * cs[2]);
		out[r * 4 + 0] = (float)R[r][0];
		out[r * 4 + 1] = (float)R[r][1];
		out[r * 4 + 2] = (float)R[r][2];
		out[r * 4 + 3] = (float)tr;
	}
}

// The rigid transform of three pairs s[k] -> t[k]: the centroids and the demeaned cross-covariance in float, then horn_fit.  out: 3 x 4 row-major.
RANSAC_HD inline void fit_three_pairs(const float (*s)[3], const float (*t)[3], float *out)
{
	float cs[3], ct[3];
RANSAC_UNROLL
	for (int a = 0; a < 3; a++)
	{
		cs[a] = ((s[0][a] + s[1][a]) + s[2][a]) / 3.0f;
		ct[a] = ((t[0][a] + t[1][a]) + t[2][a]) / 3.0f;
	}
	double H[9], csd[3], ctd[3];
RANSAC_UNROLL
	for (int a = 0; a < 3; a++)
	{
RANSAC_UNROLL
		for (int b = 0; b < 3; b++)
		{
			const float h0 = (s[0][a] - cs[a]) * (t[0][b] - ct[b]), h1 = (s[1][a] - cs[a]) * (t[1][b] - ct[b]), h2 = (s[2][a] - cs[a]) * (t[2][b] - ct[b]);
			H[a * 3 + b] = (double)((h0 + h1) + h2);
		}
		csd[a] = (double)cs[a], ctd[a] = (double)ct[a];
	}
	horn_fit(H, csd, ctd, out);
}
