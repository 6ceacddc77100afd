// scan.cpp — mulls_scan_prepare and mulls_mapper_*: the raw-scan steps of CFilter in front of the feature extraction (test/mulls_slam.cpp:359-362, :404-412) and
// the merged map the run exports (:959-1015), on the device (k_scan.hip).  Host side: argument checks, the frames of a call cut into sub-batches (host
// frames staged into one buffer sized by a byte budget, device frames read where they are), per sub-batch the counting passes, one download of the frames'
// counts and time-stamp ranges, the capacity rule, the write pass.  include/mulls_hip.h has the definition this file follows.
#include <chrono>
#include <cmath>

#include "ctx.h"
#include "scan_host.h"
#include "scan_launch.h"
#include "subbatch.h"

// a context's scratch of these entry points: one device arena (tables, per-chunk arrays, staged host frames), the records mulls_scan_prepare keeps on
// their way back, one pinned host buffer for the tables; grow-only
struct mulls_scan_scratch
{
	unsigned char *dev = nullptr, *out = nullptr, *pin = nullptr;
	size_t dev_cap = 0, out_cap = 0, pin_cap = 0;
};

struct mulls_mapper
{
	float4 *buf = nullptr;
	uint32_t cap = 0, n = 0;
};

namespace
{
using namespace mulls::scan;
constexpr size_t REC = MULLS_POINT_BYTES;
constexpr size_t STAGE_BUDGET_BYTES = (size_t)512 << 20; // host frames staged per sub-batch (a frame beyond it travels alone)
constexpr uint32_t MAX_FRAMES_PER_SUBBATCH = 4096u, MAX_CHUNKS_PER_SUBBATCH = 1u << 20;

bool on_device(mulls_ctx *ctx, const void *pts, size_t bytes)
{
	if (mulls_is_map_memory(ctx, pts, bytes))
		return true;
	hipPointerAttribute_t at;
	std::memset(&at, 0, sizeof(at));
	if (hipPointerGetAttributes(&at, pts) == hipSuccess)
		return at.type == hipMemoryTypeDevice;
	(void)hipGetLastError(); // (an ordinary host pointer: the query reports an error on some runtimes — cleared)
	return false;
}

struct FrameIn
{
	const void *pts;
	uint32_t n;
	bool dev;
	FrameMove move;
};

// frames[0 .. F) through the passes; their kept records go to dest in frame order while they fit into `room` records.  stats: every frame's counts (and the
// duration each used, mode 1); *written: how many frames were written; *needed: the records all of them have.  MULLS_E_INVALID (NaN time stamp): whatever was
// written is to be forgotten by the caller.
int scan_run(mulls_ctx *ctx, const char *who, std::vector<FrameIn> &frames, const mulls_scan_prep_params &params, float4 *dest, uint64_t room,
			 std::vector<ScanFrameStat> &stats, std::vector<float> &durations, uint32_t *written, uint64_t *needed)
{
	const Prep P = derive(params);
	const uint32_t F = (uint32_t)frames.size();
	stats.assign(F, ScanFrameStat{});
	durations.assign(F, params.scan_duration_ms);
	*written = 0, *needed = 0;
	if (!ctx->scanprep)
		ctx->scanprep = new mulls_scan_scratch();
	mulls_scan_scratch &sc = *ctx->scanprep;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	Appender app{0, room, true};
	for (uint32_t f0 = 0; f0 < F;)
	{
		// the sub-batch [f0, f1)
		uint32_t f1 = f0, G = 0;
		size_t staged = 0;
		while (f1 < F && f1 - f0 < MAX_FRAMES_PER_SUBBATCH)
		{
			const size_t bytes = frames[f1].dev ? 0 : up256((size_t)frames[f1].n * REC);
			if (f1 > f0 && (staged + bytes > STAGE_BUDGET_BYTES || G + chunks_of(frames[f1].n) > MAX_CHUNKS_PER_SUBBATCH))
				break;
			staged += bytes;
			G += chunks_of(frames[f1].n);
			f1++;
		}
		const uint32_t Fs = f1 - f0;
		size_t off = 0;
		auto take = [&](size_t bytes) {
			const size_t o = off;
			off += up256(bytes);
			return o;
		};
		const size_t o_frames = take(Fs * sizeof(ScanFrame)), o_chunk0 = take((Fs + 1u) * 4u), o_stats = take(Fs * sizeof(ScanFrameStat));
		const size_t o_ballots = take((size_t)G * MULLS_SCAN_WAVES * 8u), o_base = take((size_t)G * 4u), o_first = take((size_t)G * 8u), o_last = take((size_t)G * 8u);
		const size_t o_nan = take((size_t)G * 4u), o_stage = take(staged);
		if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
			return rc;
		const size_t table_bytes = o_stats; // frames and chunk0, contiguous
		if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, table_bytes + up256(Fs * sizeof(ScanFrameStat)), hipHostMallocDefault))
			return rc;
		unsigned char *d = sc.dev, *h = sc.pin;
		ScanFrame *hf = reinterpret_cast<ScanFrame *>(h + o_frames);
		uint32_t *hc = reinterpret_cast<uint32_t *>(h + o_chunk0);
		ScanFrameStat *hs = reinterpret_cast<ScanFrameStat *>(h + table_bytes);
		size_t so = o_stage;
		uint32_t g = 0;
		for (uint32_t k = 0; k < Fs; k++)
		{
			const FrameIn &fr = frames[f0 + k];
			std::memset(&hf[k], 0, sizeof(ScanFrame));
			hf[k].n = fr.n, hf[k].chunk0 = hc[k] = g;
			hf[k].move = fr.move;
			g += chunks_of(fr.n);
			if (fr.dev)
				hf[k].in = static_cast<const float4 *>(fr.pts);
			else
			{
				hf[k].in = reinterpret_cast<const float4 *>(d + so);
				if (fr.n)
					HIPCHK(ctx, hipMemcpyAsync(d + so, fr.pts, (size_t)fr.n * REC, hipMemcpyHostToDevice, st));
				so += up256((size_t)fr.n * REC);
			}
		}
		hc[Fs] = g;
		ScanBatch B;
		B.frames = reinterpret_cast<const ScanFrame *>(d + o_frames), B.chunk0 = reinterpret_cast<const uint32_t *>(d + o_chunk0);
		B.stats = reinterpret_cast<ScanFrameStat *>(d + o_stats), B.ballots = reinterpret_cast<uint64_t *>(d + o_ballots);
		B.base = reinterpret_cast<uint32_t *>(d + o_base), B.chunk_first = reinterpret_cast<double *>(d + o_first), B.chunk_last = reinterpret_cast<double *>(d + o_last);
		B.chunk_nan = reinterpret_cast<uint32_t *>(d + o_nan);
		B.F = Fs, B.G = G;
		HIPCHK(ctx, hipMemcpyAsync(d, h, table_bytes, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, launch_scan_flag(st, B, P));
		HIPCHK(ctx, launch_scan_ranks(st, B, P));
		if (P.ts_mode == 1)
			HIPCHK(ctx, launch_scan_minmax(st, B, P));
		HIPCHK(ctx, hipMemcpyAsync(hs, B.stats, Fs * sizeof(ScanFrameStat), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		// the counts are known: the time-stamp refusal, the durations, where every frame goes, how many fit
		uint32_t fit = 0;
		for (uint32_t k = 0; k < Fs; k++)
		{
			stats[f0 + k] = hs[k];
			if (P.ts_mode == 1)
			{
				if (hs[k].nan_stamp)
				{
					ctx->err = std::string(who) + ": a time stamp is NaN";
					return MULLS_E_INVALID;
				}
				hf[k].move.last = hs[k].last;
				hf[k].move.duration = durations[f0 + k] = stamp_duration(hs[k].first, hs[k].last, params.scan_duration_ms);
			}
			bool fits;
			hf[k].out = dest + (size_t)app.place(hs[k].n_out, &fits) * 3; // (past the room for a frame that is not appended: never launched)
			if (fits)
				fit = k + 1;
		}
		if (fit)
		{
			B.F = fit, B.G = hc[fit];
			HIPCHK(ctx, hipMemcpyAsync(d, h, table_bytes, hipMemcpyHostToDevice, st));
			HIPCHK(ctx, launch_scan_write(st, B, P));
			HIPCHK(ctx, hipStreamSynchronize(st)); // (the tables and the staged frames are reused by the next sub-batch)
			*written = f0 + fit;
		}
		f0 = f1;
	}
	*needed = app.at;
	return MULLS_OK;
}

int check_common(mulls_ctx *ctx, const char *who, const mulls_scan_prep_params *params)
{
	if (const char *why = refusal(*params))
	{
		ctx->err = std::string(who) + ": " + why;
		return MULLS_E_INVALID;
	}
	return MULLS_OK;
}

int prepare_impl(mulls_ctx *ctx, void *pts, uint32_t n, uint32_t stride, const mulls_scan_prep_params *params, uint32_t *n_out, mulls_scan_prep_report *report)
{
	const auto t0 = std::chrono::steady_clock::now();
	if (!ctx || !params || !n_out || (n && !pts))
		return MULLS_E_INVALID;
	*n_out = 0;
	if (report)
		std::memset(report, 0, sizeof(*report));
	if (stride != MULLS_POINT_BYTES)
	{
		ctx->err = "mulls_scan_prepare: stride (48)";
		return MULLS_E_INVALID;
	}
	if (int rc = check_common(ctx, "mulls_scan_prepare", params))
		return rc;
	if (n == 0)
		return MULLS_OK;
	if (n > MULLS_SCAN_MAX_POINTS)
	{
		ctx->err = "mulls_scan_prepare: more than 2^24 = 16777216 points";
		return MULLS_E_UNSUPPORTED;
	}
	HIPCHK(ctx, hipSetDevice(ctx->device));
	std::vector<FrameIn> frames(1);
	frames[0].pts = pts, frames[0].n = n, frames[0].dev = on_device(ctx, pts, (size_t)n * REC);
	frames[0].move = frame_move_of(nullptr, nullptr, false);
	if (!ctx->scanprep)
		ctx->scanprep = new mulls_scan_scratch();
	if (int rc = grow(ctx, &ctx->scanprep->out, &ctx->scanprep->out_cap, (size_t)n * REC))
		return rc;
	std::vector<ScanFrameStat> stats;
	std::vector<float> durations;
	uint32_t written = 0;
	uint64_t needed = 0;
	if (int rc = scan_run(ctx, "mulls_scan_prepare", frames, *params, reinterpret_cast<float4 *>(ctx->scanprep->out), n, stats, durations, &written, &needed))
		return rc;
	const uint32_t kept = stats[0].n_out;
	if (kept)
	{
		HIPCHK(ctx, hipMemcpyAsync(pts, ctx->scanprep->out, (size_t)kept * REC, frames[0].dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	}
	*n_out = kept;
	if (report)
	{
		report->n_in = n, report->n_after_dist = stats[0].n_dist, report->n_out = kept;
		report->first_timestamp = stats[0].first, report->last_timestamp = stats[0].last;
		report->scan_duration_used = durations[0];
		report->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	}
	return MULLS_OK;
}

bool owns(const mulls_ctx *ctx, const mulls_mapper *m) { return std::find(ctx->mappers.begin(), ctx->mappers.end(), m) != ctx->mappers.end(); }

int add_impl(mulls_ctx *ctx, mulls_mapper *m, const mulls_mapper_frame *in, uint32_t n_frames, const mulls_scan_prep_params *prep, uint32_t *frame_n_out,
			 mulls_mapper_report *report)
{
	const auto t0 = std::chrono::steady_clock::now();
	if (!ctx || !m || !prep || (n_frames && !in))
		return MULLS_E_INVALID;
	if (report)
		std::memset(report, 0, sizeof(*report));
	if (!owns(ctx, m))
	{
		ctx->err = "mulls_mapper_add: the mapper does not belong to this context";
		return MULLS_E_INVALID;
	}
	if (int rc = check_common(ctx, "mulls_mapper_add", prep))
		return rc;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	const mulls_scan_prep_params params = mapper_params(*prep);
	std::vector<FrameIn> frames(n_frames);
	for (uint32_t f = 0; f < n_frames; f++)
	{
		const mulls_cloud &c = in[f].scan;
		if ((c.n && !c.pts) || c.stride != MULLS_POINT_BYTES)
		{
			ctx->err = "mulls_mapper_add: a frame's scan (stride 48)";
			return MULLS_E_INVALID;
		}
		if (c.n > MULLS_SCAN_MAX_POINTS)
		{
			ctx->err = "mulls_mapper_add: a frame of more than 2^24 = 16777216 points";
			return MULLS_E_UNSUPPORTED;
		}
		for (int k = 0; k < 16; k++)
			if (!std::isfinite(in[f].pose[k]) || (in[f].compensate && !std::isfinite(in[f].adjacent_tran[k])))
			{
				ctx->err = "mulls_mapper_add: a frame's pose or adjacent_tran is not finite";
				return MULLS_E_INVALID;
			}
		frames[f].pts = c.pts, frames[f].n = c.n, frames[f].dev = c.n && on_device(ctx, c.pts, (size_t)c.n * REC);
		frames[f].move = frame_move_of(in[f].pose, in[f].adjacent_tran, in[f].compensate != 0);
	}
	std::vector<ScanFrameStat> stats;
	std::vector<float> durations;
	uint32_t written = 0;
	uint64_t needed = 0;
	if (int rc = scan_run(ctx, "mulls_mapper_add", frames, params, m->buf + (size_t)m->n * 3, (uint64_t)(m->cap - m->n), stats, durations, &written, &needed))
		return rc;
	uint32_t added = 0;
	for (uint32_t f = 0; f < n_frames; f++)
	{
		if (frame_n_out)
			frame_n_out[f] = stats[f].n_out;
		if (f < written)
			added += stats[f].n_out;
	}
	const uint32_t before = m->n;
	m->n += added;
	if (report)
	{
		report->frames_added = written, report->n_before = before, report->n_after = m->n;
		report->n_needed = (uint64_t)before + needed;
		report->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	}
	if (written < n_frames)
	{
		ctx->err = "mulls_mapper_add: the map is full";
		return MULLS_E_UNSUPPORTED;
	}
	return MULLS_OK;
}
} // namespace

void mulls_scan_release(mulls_ctx *ctx)
{
	while (!ctx->mappers.empty())
		mulls_mapper_destroy(ctx, ctx->mappers.back());
	if (!ctx->scanprep)
		return;
	staggered_free(ctx->scanprep->dev);
	staggered_free(ctx->scanprep->out);
	if (ctx->scanprep->pin)
		(void)hipHostFree(ctx->scanprep->pin);
	delete ctx->scanprep;
	ctx->scanprep = nullptr;
}

extern "C"
{
	void mulls_scan_prep_default_params(mulls_scan_prep_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->downsample_ratio = 1;
		p->scan_duration_ms = 100.0f;		   // cfilter.hpp:414
		p->vertical_ang_correction_deg = 0.0;  // :250
		p->min_dist = 1.0, p->max_dist = 120.0; // test/mulls_slam.cpp:52-53
		p->scan_begin_ang_deg = 180.0;		   // cfilter.hpp:414
	}

	int mulls_scan_prepare(mulls_ctx *ctx, void *pts, uint32_t n, uint32_t stride, const mulls_scan_prep_params *params, uint32_t *n_out,
						   mulls_scan_prep_report *report)
	try
	{
		return prepare_impl(ctx, pts, n, stride, params, n_out, report);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_mapper_create(mulls_ctx *ctx, uint32_t capacity_points, mulls_mapper **out)
	try
	{
		if (!ctx || !out)
			return MULLS_E_INVALID;
		*out = nullptr;
		if (capacity_points > MULLS_SCAN_MAX_POINTS)
		{
			ctx->err = "mulls_mapper_create: more than 2^24 = 16777216 points";
			return MULLS_E_UNSUPPORTED;
		}
		HIPCHK(ctx, hipSetDevice(ctx->device));
		mulls_mapper *m = new mulls_mapper();
		if (hipMalloc((void **)&m->buf, std::max<size_t>((size_t)capacity_points * REC, 256)) != hipSuccess)
		{
			delete m;
			ctx->err = "mulls_mapper_create: hipMalloc failed";
			return MULLS_E_HIP;
		}
		m->cap = capacity_points;
		ctx->mappers.push_back(m);
		*out = m;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	void mulls_mapper_destroy(mulls_ctx *ctx, mulls_mapper *m)
	{
		if (!ctx || !m || !owns(ctx, m))
			return;
		ctx->mappers.erase(std::remove(ctx->mappers.begin(), ctx->mappers.end(), m), ctx->mappers.end());
		(void)hipSetDevice(ctx->device);
		(void)hipFree(m->buf);
		delete m;
	}

	int mulls_mapper_add(mulls_ctx *ctx, mulls_mapper *mapper, const mulls_mapper_frame *frames, uint32_t n_frames, const mulls_scan_prep_params *prep,
						 uint32_t *frame_n_out, mulls_mapper_report *report)
	try
	{
		return add_impl(ctx, mapper, frames, n_frames, prep, frame_n_out, report);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_mapper_cloud(mulls_ctx *ctx, const mulls_mapper *m, mulls_cloud *out)
	try
	{
		if (!ctx || !m || !out || !owns(ctx, m))
			return MULLS_E_INVALID;
		out->pts = m->buf, out->n = m->n, out->stride = MULLS_POINT_BYTES;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_mapper_download(mulls_ctx *ctx, const mulls_mapper *m, uint32_t first, void *pts, uint32_t cap, uint32_t *n)
	try
	{
		if (!ctx || !m || !n || (cap && !pts) || !owns(ctx, m) || first > m->n)
			return MULLS_E_INVALID;
		*n = m->n - first;
		const uint32_t take = std::min(*n, cap);
		if (take)
		{
			HIPCHK(ctx, hipSetDevice(ctx->device));
			HIPCHK(ctx, hipMemcpyAsync(pts, m->buf + (size_t)first * 3, (size_t)take * REC, hipMemcpyDeviceToHost, ctx->stream));
			HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		}
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_mapper_clear(mulls_ctx *ctx, mulls_mapper *m)
	try
	{
		if (!ctx || !m || !owns(ctx, m))
			return MULLS_E_INVALID;
		m->n = 0;
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}
}
