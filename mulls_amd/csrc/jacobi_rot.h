// jacobi_rot.h — the Jacobi rotation of the symmetric 3 x 3 eigen-decompositions: pca_device.h (the neighbourhood PCA, device only) and ndt_math.h (an
// NDT leaf's covariance, host and device) expand the same text.  No include of its own: plain double arithmetic in named scalars.
#pragma once

// one Jacobi rotation annihilating a(p,q)
#define MULLS_PCA_ROT(app, aqq, apq, apr, aqr, vxp, vxq, vyp, vyq, vzp, vzq)                            \
	if (apq != 0.0)                                                                                      \
	{                                                                                                    \
		const double theta = (aqq - app) / (2.0 * apq);                                                  \
		const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));          \
		const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;                                          \
		/* A <- A J : columns p and q */                                                                 \
		const double c_pp = cs * app - sn * apq, c_pq = sn * app + cs * apq;                             \
		const double c_qp = cs * apq - sn * aqq, c_qq = sn * apq + cs * aqq;                             \
		const double c_rp = cs * apr - sn * aqr, c_rq = sn * apr + cs * aqr;                             \
		/* A <- J^T A : rows p and q; the upper triangle is the matrix */                                \
		app = cs * c_pp - sn * c_qp;                                                                     \
		aqq = sn * c_pq + cs * c_qq;                                                                     \
		apq = cs * c_pq - sn * c_qq;                                                                     \
		apr = c_rp;                                                                                      \
		aqr = c_rq;                                                                                      \
		double u = vxp, w = vxq;                                                                         \
		vxp = cs * u - sn * w, vxq = sn * u + cs * w;                                                    \
		u = vyp, w = vyq;                                                                                \
		vyp = cs * u - sn * w, vyq = sn * u + cs * w;                                                    \
		u = vzp, w = vzq;                                                                                \
		vzp = cs * u - sn * w, vzq = sn * u + cs * w;                                                    \
	}
