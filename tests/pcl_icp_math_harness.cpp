// A stand-alone program over mulls_amd/csrc/pcl_icp_math.h for tests/test_pcl_icp.py (built with g++ -ffp-contract=off; it may also be built with
// -fsanitize=address,undefined): argv[1] names the piece, doubles come in on stdin and go out on stdout, both raw.
//   normal      records of k, p (3), k x 3 neighbours in order   -> m x 3 (the float normal, widened)
//   term        m x 9: s 3, t 3, n 3                              -> m x 28 (added to sums that start at +0)
//   plane       m x 27: the upper triangle 21, A^T b 6            -> m x 13: R 9, t 3 (0 when not ok), ok
//   rigid       m x 15: H 9, cs 3, ct 3                           -> m x 12: R 9, t 3
//   run M I TE EE   m x 29: the 28 sums and the number of pairs of consecutive iterations; the metric, max_iter_num, the epsilons
//                                                                 -> m x 32: R 9, t 3, Rs 9, ts 3, mse, prev_mse, n_corr, iterations, converged, stop,
//                                                                    running, moved
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../mulls_amd/csrc/pcl_icp_math.h"

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
	if (op == "normal")
	{
		size_t at = 0;
		while (at + 4 <= in.size())
		{
			const double kd = in[at];
			if (!(kd >= 0.0 && kd <= 1048576.0))
				return 2;
			const size_t k = (size_t)kd;
			if (at + 4 + 3 * k > in.size())
				return 2;
			float n[3];
			pcl_icp::point_normal(in.data() + at + 4, (int)k, in[at + 1], in[at + 2], in[at + 3], n);
			for (int c = 0; c < 3; c++)
				out.push_back((double)n[c]);
			at += 4 + 3 * k;
		}
	}
	else if (op == "term")
		for (size_t at = 0; at + 9 <= in.size(); at += 9)
		{
			double a[pcl_icp::N_SUMS];
			for (int k = 0; k < pcl_icp::N_SUMS; k++)
				a[k] = 0.0;
			pcl_icp::plane_term(in.data() + at, in.data() + at + 3, in.data() + at + 6, a);
			out.insert(out.end(), a, a + pcl_icp::N_SUMS);
		}
	else if (op == "plane")
		for (size_t at = 0; at + 27 <= in.size(); at += 27)
		{
			double r[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, R[9], t[3];
			if (pcl_icp::plane_step(in.data() + at, R, t))
			{
				memcpy(r, R, sizeof(R)), memcpy(r + 9, t, sizeof(t));
				r[12] = 1.0;
			}
			out.insert(out.end(), r, r + 13);
		}
	else if (op == "rigid")
		for (size_t at = 0; at + 15 <= in.size(); at += 15)
		{
			double r[12];
			pcl_icp::rigid_step(in.data() + at, in.data() + at + 9, in.data() + at + 12, r, r + 9);
			out.insert(out.end(), r, r + 12);
		}
	else if (op == "run" && argc == 6)
	{
		const int metric = atoi(argv[2]), max_it = atoi(argv[3]);
		const double te = atof(argv[4]), ee = atof(argv[5]);
		pcl_icp::State S;
		pcl_icp::begin(S);
		for (size_t at = 0; at + 29 <= in.size() && S.running; at += 29)
		{
			pcl_icp::advance(S, metric, in.data() + at, (uint32_t)in[at + 28], max_it, te, ee);
			out.insert(out.end(), S.R, S.R + 9), out.insert(out.end(), S.t, S.t + 3), out.insert(out.end(), S.Rs, S.Rs + 9), out.insert(out.end(), S.ts, S.ts + 3);
			const double tail[8] = {S.mse,			 S.prev_mse,	  (double)S.n_corr,	 (double)S.iterations,
									(double)S.converged, (double)S.stop, (double)S.running, (double)S.moved};
			out.insert(out.end(), tail, tail + 8);
		}
	}
	else
		return 2;
	if (!out.empty() && fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size())
		return 3;
	return 0;
}
