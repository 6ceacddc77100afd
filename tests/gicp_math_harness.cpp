// A stand-alone program over mulls_amd/csrc/gicp_math.h for tests/test_gicp.py (built with g++ -ffp-contract=off; it may also be built with
// -fsanitize=address,undefined): argv[1] names the piece, doubles come in on stdin and go out on stdout, both raw.
//   cov K       m x K x 3 neighbours in order              -> m x 6
//   exp         m x 3                                      -> m x 9
//   explog      m x 3                                      -> m x 3: log(exp(w))
//   term        m x 27: a' 3, C_A 6, mean 3, cov_B 6, R 9  -> m x 28 (added to sums that start at +0)
//   step        m x 27: the upper triangle 21, J^T e 6     -> m x 7: delta, ok
//   run I RE TE s0 s1 s2     m x 29: the 28 sums and n_corr of consecutive evaluations; max_iterations, the epsilons, start_rotvec
//                                                          -> m x 21: r 3, t 3, R 9, loss, n_corr, iterations, converged, stop, running
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../mulls_amd/csrc/gicp_math.h"

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	std::vector<double> in;
	double buf[1024];
	size_t got;
	while ((got = fread(buf, sizeof(double), 1024, stdin)) > 0)
		in.insert(in.end(), buf, buf + got);
	std::vector<double> out;
	const std::string op = argv[1];
	if (op == "cov" && argc == 3)
	{
		const int k = atoi(argv[2]);
		if (k < 1 || k > 64)
			return 2;
		for (size_t at = 0; at + 3 * (size_t)k <= in.size(); at += 3 * (size_t)k)
		{
			double C[6];
			gicp::point_covariance(in.data() + at, k, C);
			out.insert(out.end(), C, C + 6);
		}
	}
	else if (op == "exp" || op == "explog")
		for (size_t at = 0; at + 3 <= in.size(); at += 3)
		{
			double R[9], w[3];
			gicp::so3_exp(in.data() + at, R);
			gicp::so3_log(R, w);
			if (op == "exp")
				out.insert(out.end(), R, R + 9);
			else
				out.insert(out.end(), w, w + 3);
		}
	else if (op == "term")
		for (size_t at = 0; at + 27 <= in.size(); at += 27)
		{
			const double *p = in.data() + at;
			double a[28];
			for (int k = 0; k < 28; k++)
				a[k] = 0.0;
			gicp::point_term(p, p + 3, p + 9, p + 12, p + 18, a);
			out.insert(out.end(), a, a + 28);
		}
	else if (op == "step")
		for (size_t at = 0; at + 27 <= in.size(); at += 27)
		{
			double d[7] = {0, 0, 0, 0, 0, 0, 0};
			d[6] = (double)gicp::solve_step(in.data() + at, in.data() + at + 21, d);
			out.insert(out.end(), d, d + 7);
		}
	else if (op == "run" && argc == 8)
	{
		const int max_it = atoi(argv[2]);
		const double re = atof(argv[3]), te = atof(argv[4]);
		const float start[3] = {(float)atof(argv[5]), (float)atof(argv[6]), (float)atof(argv[7])};
		gicp::State S;
		gicp::begin(S, start);
		for (size_t at = 0; at + 29 <= in.size() && S.running; at += 29)
		{
			gicp::advance(S, in.data() + at, (uint32_t)in[at + 28], max_it, re, te);
			out.insert(out.end(), S.r, S.r + 3), out.insert(out.end(), S.t, S.t + 3), out.insert(out.end(), S.R, S.R + 9);
			const double tail[6] = {S.loss, (double)S.n_corr, (double)S.iterations, (double)S.converged, (double)S.stop, (double)S.running};
			out.insert(out.end(), tail, tail + 6);
		}
	}
	else
		return 2;
	if (!out.empty() && fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size())
		return 3;
	return 0;
}
