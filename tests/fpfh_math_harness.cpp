// A stand-alone program over mulls_amd/csrc/fpfh_math.h for tests/test_fpfh.py (built with g++ -ffp-contract=off; it may also be built with
// -fsanitize=address,undefined): argv[1] names the piece, doubles come in on stdin and go out on stdout, both raw.
//   pair        m x 12: p 3, n_p 3, q 3, n_q 3 (floats, widened)  -> m x 7: adds (0 / 1), f1 f2 f3, the three bins (zeros when the pair adds nothing)
//   bins        m x 3: f1 f2 f3                                   -> m x 4: adds (0 / 1: no NaN), the three bins
//   spfh        m x 2: the count, k                               -> m x 1
//   norm        m x 33: the weighted sums                         -> m x 33 (the float histogram, widened)
//   error       m x 3: e, thr (floats, widened), huber (0 / 1)    -> m x 1
//   order       m x 4: two errors with their indices (ea, ia, eb, ib) -> m x 1: is a before b (fpfh::error_before)
//   dist        m x 66: two descriptors (floats, widened)         -> m x 1
//   draw N K I D S   the source's 3 N coordinates; k_eff, iterations, min_sample_distance, the seed
//                                                                 -> I x 6: the samples 3, the ranks 3; then one row: min_sample_distance at the end, 0 x 5
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../mulls_amd/csrc/fpfh_math.h"

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
	if (op == "pair")
	{
		for (size_t at = 0; at + 12 <= in.size(); at += 12)
		{
			float v[12];
			for (int k = 0; k < 12; k++)
				v[k] = (float)in[at + k];
			double f[3] = {0, 0, 0};
			int b[3] = {0, 0, 0};
			const bool adds = fpfh::pair_feature(v, v + 3, v + 6, v + 9, f) && fpfh::bins_of(f, b);
			out.push_back(adds ? 1.0 : 0.0);
			for (int k = 0; k < 3; k++)
				out.push_back(adds ? f[k] : 0.0);
			for (int k = 0; k < 3; k++)
				out.push_back(adds ? (double)b[k] : 0.0);
		}
	}
	else if (op == "bins")
	{
		for (size_t at = 0; at + 3 <= in.size(); at += 3)
		{
			int b[3] = {0, 0, 0};
			const bool adds = fpfh::bins_of(&in[at], b);
			out.push_back(adds ? 1.0 : 0.0);
			for (int k = 0; k < 3; k++)
				out.push_back(adds ? (double)b[k] : 0.0);
		}
	}
	else if (op == "spfh")
	{
		for (size_t at = 0; at + 2 <= in.size(); at += 2)
			out.push_back((double)fpfh::spfh_of_count((uint32_t)in[at], (uint32_t)in[at + 1]));
	}
	else if (op == "norm")
	{
		for (size_t at = 0; at + MULLS_FPFH_DIMS <= in.size(); at += MULLS_FPFH_DIMS)
			for (int s = 0; s < 3; s++)
			{
				float h[MULLS_FPFH_BINS];
				fpfh::normalise(&in[at + MULLS_FPFH_BINS * s], h);
				for (int b = 0; b < MULLS_FPFH_BINS; b++)
					out.push_back((double)h[b]);
			}
	}
	else if (op == "error")
	{
		for (size_t at = 0; at + 3 <= in.size(); at += 3)
			out.push_back(fpfh::error_term((float)in[at], (float)in[at + 1], in[at + 2] != 0.0));
	}
	else if (op == "order")
	{
		for (size_t at = 0; at + 4 <= in.size(); at += 4)
			out.push_back(fpfh::error_before(in[at], (uint32_t)in[at + 1], in[at + 2], (uint32_t)in[at + 3]) ? 1.0 : 0.0);
	}
	else if (op == "dist")
	{
		for (size_t at = 0; at + 2 * MULLS_FPFH_DIMS <= in.size(); at += 2 * MULLS_FPFH_DIMS)
		{
			float a[MULLS_FPFH_DIMS], b[MULLS_FPFH_DIMS];
			for (int k = 0; k < MULLS_FPFH_DIMS; k++)
				a[k] = (float)in[at + k], b[k] = (float)in[at + MULLS_FPFH_DIMS + k];
			out.push_back((double)fpfh::desc_dist2(a, b));
		}
	}
	else if (op == "draw" && argc == 7)
	{
		const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10), k_eff = (uint32_t)strtoul(argv[3], nullptr, 10);
		const int iters = atoi(argv[4]);
		const float min_d = (float)strtod(argv[5], nullptr);
		const uint32_t seed = (uint32_t)strtoul(argv[6], nullptr, 10);
		if (n < 3 || k_eff < 1 || iters < 1 || in.size() != 3 * (size_t)n)
			return 2;
		std::vector<float> xyz(in.begin(), in.end());
		std::vector<int32_t> samples, ranks;
		const float end = fpfh::draw_all(xyz.data(), n, k_eff, 3, iters, min_d, seed, samples, ranks);
		for (int it = 0; it < iters; it++)
		{
			for (int s = 0; s < 3; s++)
				out.push_back((double)samples[3 * it + s]);
			for (int s = 0; s < 3; s++)
				out.push_back((double)ranks[3 * it + s]);
		}
		out.push_back((double)end);
		for (int k = 0; k < 5; k++)
			out.push_back(0.0);
	}
	else
		return 2;
	fwrite(out.data(), sizeof(double), out.size(), stdout);
	return 0;
}
