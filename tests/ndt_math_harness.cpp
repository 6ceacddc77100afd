// C entry points over mulls_amd/csrc/ndt_math.h and detmath.h's exp_cr for tests/test_ndt.py (compiled with g++ -ffp-contract=off, like detmath_harness.cpp)
#include <cstring>

#include "../mulls_amd/csrc/ndt_math.h"

extern "C"
{
	void nh_exp(const double *x, double *out, long n)
	{
		for (long i = 0; i < n; i++)
			out[i] = mulls::det::exp_cr(x[i]);
	}
	// out: mean 3, icov 6, evals 3, n, inflated
	void nh_leaf(int n, const double *s, const double *q, int min_points, double eig_mult, double *out)
	{
		ndt::Leaf L;
		ndt::finalize_leaf(n, s, q, min_points, eig_mult, &L);
		std::memcpy(out, L.mean, 24), std::memcpy(out + 3, L.icov, 48), std::memcpy(out + 9, L.evals, 24);
		out[12] = (double)L.n, out[13] = (double)L.inflated;
	}
	// frame: R 9, t 3, j 24, h 45
	void nh_frame(const double *p, double *out)
	{
		ndt::Frame F;
		ndt::make_frame(p, &F);
		std::memcpy(out, &F, sizeof(F));
	}
	void nh_transform(const double *p, const float *x, float *out)
	{
		ndt::Frame F;
		ndt::make_frame(p, &F);
		ndt::transform_point(F.R, F.t, x[0], x[1], x[2], out);
	}
	// a[28] += the (point, leaf) term at pose p
	void nh_contribution(const double *p, const double *x, const double *xt, const double *C, double d1, double d2, int with_hessian, double *a)
	{
		ndt::Frame F;
		ndt::make_frame(p, &F);
		ndt::contribution(x, xt, C, F.j, F.h, d1, d2, with_hessian, a);
	}
	void nh_solve6(const double *Hu, const double *g, double *delta) { ndt::solve6(Hu, g, delta); }

	// a scripted run: sums[k] is handed to the state's k-th request.  out per step: xt 6, with_hessian, phase, running, a_t; returns the steps taken;
	// fin: p 6, nr_iterations, evaluations, converged, reversals, inner_steps, trans_probability
	int nh_script(const double *sums, int n_steps, double step_size, double eps, int max_iterations, int max_step_iterations, double n_src, double *out,
				  double *fin)
	{
		ndt::State S;
		ndt::begin(S);
		ndt::Opts o;
		o.step_size = step_size, o.transformation_epsilon = eps, o.mu = 1.e-4, o.nu = 0.9, o.n_src = n_src;
		o.max_iterations = max_iterations, o.max_step_iterations = max_step_iterations;
		int k = 0;
		for (; k < n_steps && S.running; k++)
		{
			ndt::advance(S, sums + 28 * k, o);
			double *r = out + 10 * k;
			std::memcpy(r, S.xt, 48);
			r[6] = S.with_hessian, r[7] = S.phase, r[8] = S.running, r[9] = S.a_t;
		}
		std::memcpy(fin, S.p, 48);
		fin[6] = S.nr_iterations, fin[7] = S.evaluations, fin[8] = S.converged, fin[9] = S.reversals, fin[10] = S.inner_steps, fin[11] = S.trans_probability;
		return k;
	}
}
