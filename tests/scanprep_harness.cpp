// scanprep_harness.cpp — mulls_scan_prepare / mulls_mapper_add on the CPU: the arithmetic the kernels compile (mulls_amd/csrc/scan_math.h) and the host's
// planning (scan_host.h: refusals, a frame's transforms, the capacity rule) driven chunk by chunk as k_scan.hip drives them — per-chunk survivor counts, their
// exclusive scan, the thinning as arithmetic on ranks, the time-stamp folds per chunk and then per frame — on one thread.  tests/test_scanprep.py builds it with
// -fsanitize=address,undefined and compares its output with tests/scanprep_restated.py; tools/gpu_mapper.py times it.
//   scanprep_harness selfcheck            the thinning-count formula against a loop; 0 when it holds
//   scanprep_harness run IN OUT [REPS]    IN: u32 n_frames, u32 with_pose, u64 room, mulls_scan_prep_params, then per frame u32 n, i32 compensate,
//                                         double pose[16], adjacent_tran[16], n 48-byte records.  OUT: i32 rc, u32 frames_written, u64 needed, per frame
//                                         (u32 n_dist, u32 n_out, double first, last, float duration, u32 0), then the written records.  REPS > 1: the run
//                                         is repeated and "ms_per_run <value>" printed.
//   scanprep_harness asin|atan2 IN OUT    IN: doubles u (asin) or pairs y, x (atan2); OUT: detmath.h's asin_cr(u) / atan2_cr(y, x)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../mulls_amd/csrc/scan_host.h"

using namespace mulls::scan;

struct Rec
{
	float w[12]; // x y z . nx ny nz . intensity curvature . .
};
struct Frame
{
	uint32_t n;
	int32_t compensate;
	double pose[16], adj[16];
	std::vector<Rec> pts;
};
struct Stat
{
	uint32_t n_dist, n_out;
	double first, last;
	float duration;
	uint32_t pad;
};

static int run(const std::vector<Frame> &frames, const mulls_scan_prep_params &given, bool with_pose, uint64_t room, std::vector<Stat> &stats, std::vector<Rec> &out,
			   uint32_t *written, uint64_t *needed)
{
	if (refusal(given))
		return MULLS_E_INVALID;
	const mulls_scan_prep_params params = with_pose ? mapper_params(given) : given; // (with poses: mulls_mapper_add)
	const Prep P = derive(params);
	const uint32_t ratio = (uint32_t)P.ratio;
	stats.assign(frames.size(), Stat{});
	out.clear();
	*written = 0;
	Appender app{0, room, true};
	std::vector<std::vector<uint8_t>> flags(frames.size());
	std::vector<std::vector<uint32_t>> bases(frames.size());
	// the counting passes
	for (size_t f = 0; f < frames.size(); f++)
	{
		const Frame &fr = frames[f];
		const uint32_t nch = chunks_of(fr.n);
		flags[f].assign(fr.n, 0);
		bases[f].assign(nch, 0);
		uint32_t running = 0, thinned = 0;
		for (uint32_t c = 0; c < nch; c++)
		{
			uint32_t cnt = 0;
			for (uint32_t i = c * MULLS_SCAN_CHUNK; i < fr.n && i < (c + 1) * MULLS_SCAN_CHUNK; i++)
				cnt += flags[f][i] = survives(fr.pts[i].w[0], fr.pts[i].w[1], fr.pts[i].w[2], P);
			bases[f][c] = running;
			thinned += thin_count(running, cnt, ratio); // the chunk's share of the frame's output
			running += cnt;
		}
		Stat &s = stats[f];
		s.n_dist = running, s.n_out = multiples_below(running, ratio);
		if (thinned != s.n_out)
			return -1; // the per-chunk counts do not add up to the frame's
		s.first = MULLS_SCAN_FIRST_SEED, s.last = MULLS_SCAN_LAST_SEED;
		s.duration = params.scan_duration_ms;
		if (P.ts_mode == 1)
		{
			for (uint32_t c = 0; c < nch; c++)
			{
				double first = MULLS_SCAN_FIRST_SEED, last = MULLS_SCAN_LAST_SEED;
				uint32_t rank = bases[f][c];
				for (uint32_t i = c * MULLS_SCAN_CHUNK; i < fr.n && i < (c + 1) * MULLS_SCAN_CHUNK; i++)
					if (flags[f][i] && rank++ % ratio == 0)
					{
						const double v = (double)fr.pts[i].w[9];
						if (v != v)
							return MULLS_E_INVALID;
						first = fold_first(first, v), last = fold_last(last, v);
					}
				s.first = fold_first(s.first, first), s.last = fold_last(s.last, last);
			}
			s.duration = stamp_duration(s.first, s.last, params.scan_duration_ms);
		}
	}
	// the capacity rule, then the write pass
	for (size_t f = 0; f < frames.size(); f++)
	{
		bool fits;
		const uint64_t at = app.place(stats[f].n_out, &fits);
		if (!fits)
			continue;
		const Frame &fr = frames[f];
		FrameMove M = frame_move_of(with_pose ? fr.pose : nullptr, fr.adj, fr.compensate != 0);
		M.last = stats[f].last, M.duration = stats[f].duration;
		out.resize(at + stats[f].n_out);
		uint32_t rank = 0;
		for (uint32_t i = 0; i < fr.n; i++)
			if (flags[f][i] && rank++ % ratio == 0)
			{
				Rec r = fr.pts[i];
				finish_point(r.w[0], r.w[1], r.w[2], r.w[9], P, M);
				out[at + (rank - 1) / ratio] = r;
			}
		*written = (uint32_t)f + 1;
	}
	*needed = app.at;
	return MULLS_OK;
}

static int selfcheck()
{
	for (uint32_t ratio = 1; ratio <= 9; ratio++)
		for (uint32_t base = 0; base <= 40; base++)
			for (uint32_t count = 0; count <= 40; count++)
			{
				uint32_t want = 0;
				for (uint32_t r = base; r < base + count; r++)
					want += r % ratio == 0;
				if (thin_count(base, count, ratio) != want)
				{
					std::printf("thin_count(%u, %u, %u) = %u, the loop counts %u\n", base, count, ratio, thin_count(base, count, ratio), want);
					return 1;
				}
			}
	for (uint32_t n : {0u, 1u, MULLS_SCAN_CHUNK - 1u, MULLS_SCAN_CHUNK, MULLS_SCAN_CHUNK + 1u, 3u * MULLS_SCAN_CHUNK + 7u})
		if (chunks_of(n) != (n + MULLS_SCAN_CHUNK - 1u) / MULLS_SCAN_CHUNK)
			return 1;
	mulls_scan_prep_params p;
	std::memset(&p, 0, sizeof(p));
	p.min_dist = 1.0, p.max_dist = 120.0, p.scan_duration_ms = 100.0f;
	if (refusal(p))
		return 1;
	p.max_dist = INFINITY;
	if (!refusal(p))
		return 1;
	std::printf("selfcheck ok\n");
	return 0;
}

template <typename T>
static bool rd(FILE *f, T *v, size_t count = 1) { return std::fread(v, sizeof(T), count, f) == count; }

static int math_mode(bool is_asin, const char *in, const char *out)
{
	FILE *f = std::fopen(in, "rb"), *o = std::fopen(out, "wb");
	if (!f || !o)
		return 2;
	double a[2];
	while (rd(f, a, is_asin ? 1 : 2))
	{
		const double r = is_asin ? mulls::det::asin_cr(a[0]) : mulls::det::atan2_cr(a[0], a[1]);
		std::fwrite(&r, 8, 1, o);
	}
	std::fclose(f);
	std::fclose(o);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && std::string(argv[1]) == "selfcheck")
		return selfcheck();
	if (argc == 4 && (std::string(argv[1]) == "asin" || std::string(argv[1]) == "atan2"))
		return math_mode(argv[1][1] == 's', argv[2], argv[3]);
	if (argc < 4 || std::string(argv[1]) != "run")
		return 2;
	FILE *f = std::fopen(argv[2], "rb");
	if (!f)
		return 2;
	uint32_t n_frames = 0, with_pose = 0;
	uint64_t room = 0;
	mulls_scan_prep_params params;
	if (!rd(f, &n_frames) || !rd(f, &with_pose) || !rd(f, &room) || !rd(f, &params))
		return 2;
	std::vector<Frame> frames(n_frames);
	for (Frame &fr : frames)
	{
		if (!rd(f, &fr.n) || !rd(f, &fr.compensate) || !rd(f, fr.pose, 16) || !rd(f, fr.adj, 16))
			return 2;
		fr.pts.resize(fr.n);
		if (fr.n && !rd(f, fr.pts.data(), fr.n))
			return 2;
	}
	std::fclose(f);
	const int reps = argc >= 5 ? std::atoi(argv[4]) : 1;
	std::vector<Stat> stats;
	std::vector<Rec> out;
	uint32_t written = 0;
	uint64_t needed = 0;
	int32_t rc = 0;
	const auto t0 = std::chrono::steady_clock::now();
	for (int r = 0; r < (reps > 1 ? reps : 1); r++)
		rc = run(frames, params, with_pose != 0, room, stats, out, &written, &needed);
	if (reps > 1)
		std::printf("ms_per_run %.4f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps);
	FILE *o = std::fopen(argv[3], "wb");
	if (!o)
		return 2;
	std::fwrite(&rc, 4, 1, o);
	std::fwrite(&written, 4, 1, o);
	std::fwrite(&needed, 8, 1, o);
	if (rc == 0)
	{
		if (!stats.empty())
			std::fwrite(stats.data(), sizeof(Stat), stats.size(), o);
		uint64_t n_rec = 0;
		for (uint32_t k = 0; k < written; k++)
			n_rec += stats[k].n_out;
		if (n_rec)
			std::fwrite(out.data(), sizeof(Rec), n_rec, o);
	}
	std::fclose(o);
	return 0;
}
