// batch.h — internals shared by the host driver's translation units: the device-resident batch (mulls_batch), its job tables and staging
// (batch.cpp), the iteration loops (loop.cpp), the variants (variants.cpp) and the stage-level entry points (stage.cpp).  Nothing here is ABI.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mulls_hip.h"
#include "device_types.h"
#include "hostmath.h"
#include "icp_step.h"
#include "launch.h"
#include "ctx.h"

// Several small uploads and device-to-device copies as ONE launch (k_copy_segs) instead of one copy command each: a fill stages a pair's device-resident clouds
// and four tables, a run up to a dozen job tables — at 5-10 us a command that was 0.3 ms of a single scan-to-map registration's 1.2 ms.  Host data waits
// in the context's host-mapped mailbox until the kernel has read it: the caller synchronises the stream before the next SegCopier of the context is filled.
struct SegCopier
{
	mulls_ctx *ctx;
	std::vector<CopySeg> segs;
	struct Pending
	{
		void *dst;
		const void *src;
		size_t bytes;
	};
	std::vector<Pending> host; // copied into the mailbox by flush(), once the total is known
	explicit SegCopier(mulls_ctx *c) : ctx(c) {}
	void add_host(void *dst, const void *src, size_t bytes)
	{
		if (bytes)
			host.push_back({dst, src, bytes});
	}
	void add_dev(void *dst, const void *src, size_t bytes)
	{
		// (CopySeg carries a 32-bit size: a range of 4 GiB or more — a device-resident cloud of 89 M records — goes in as several segments, each a multiple of 16 bytes)
		const size_t piece = (size_t)0xfffffff0u;
		for (size_t off = 0; off < bytes; off += piece)
		{
			const size_t b = std::min(piece, bytes - off);
			segs.push_back({(unsigned long long)(uintptr_t)dst + off, (unsigned long long)(uintptr_t)src + off, (uint32_t)b, 0u});
		}
	}
	int flush(hipStream_t st); // batch.cpp
};

// (the device arrays the launch wrappers read are the base: BatchDev, launch.h)
struct mulls_batch : BatchDev
{
	int n = 0;
	size_t n_src = 0, n_tgt = 0; // staged points over all pairs and classes
	std::vector<CloudDesc> descs_h;
	std::vector<PairSetup> setup_h;
	std::vector<Job> setup_jobs_h; // k_clone_src's jobs: those of the pairs that need them whatever the run is first (n_setup_jobs_rest), then those of the pairs
								   // k_src_setup can take (src_one_wg)
	uint32_t n_setup_jobs_rest = 0;
	std::vector<uint8_t> src_one_wg; // per pair: no source cloud cropped segment-wise and at most MULLS_SRC_SETUP_CAP staged source points (batch_fill)
	// the setup's index tables (build_jobs; device copy: setup_tab).  tg_split: k_tgt_grid's size buckets, LDS-tier class clouds as pair * MULLS_NC + class.
	// crop_split: k_crop's workgroups, (pair * MULLS_NC + class) * 2 + side — [0, 1) source sides of the pairs outside src_one_wg, [1, 2) target sides off the LDS
	// tier, [2, 3) target sides on it (k_tgt_grid crops those when the setup is fused).  srcp_split: the pairs of src_one_wg.
	std::vector<uint32_t> setup_tab_h;
	uint32_t tg_split[MULLS_TG_BUCKETS + 1] = {}, crop_split[4] = {}, srcp_split[2] = {};
	size_t cap_setup_tab = 0;
	std::vector<Job> big_segs_h, big_clouds_h; // class clouds cropped segment-wise (k_crop_big_*): segments, clouds (Job::cls carries MULLS_BIG_SRC_SIDE for a source cloud)
	uint32_t n_big_tgt = 0;					   // ... how many of those clouds are targets
	std::vector<Job> jobs_h;
	std::vector<Job> cjobs_h; // one entry per (pair, used class) with source points: the LDS tier's unit of work
	std::vector<Job> cjobs_dev_h; // the same entries as uploaded: inside each sub-batch's slice the most expensive class clouds come first
	std::vector<Job> bjobs_h; // global-memory tier (k_cert_big): class-level jobs (MULLS_JOB_CLASS) and 512-point chunk-level jobs of the MULLS_TIER_BM clouds, pair order
	std::vector<Job> fjobs_h; // ... the chunk-level ones among them: k_filter finishes those clouds
	std::vector<Job> ejobs_h; // ... and every MULLS_TIER_BM cloud as chunk-level jobs, for the first iterations of a mixed batch (empty when bjobs_h holds no class-level job):
							  // while most points still need a search, many (splittable) workgroups per cloud + k_filter beat one workgroup per cloud
	std::vector<uint32_t> lclouds_h; // the used class clouds on a bitmap grid (pair * MULLS_NC + class), in grid_slot order
	int tier_mode = -1;		  // what the descriptors' tier fields were assigned for: 0 / 1 / 2 one tier for the whole batch, 3 per class cloud (assign_tiers)
	std::vector<Job> tjobs_h; // target-side chunks (256 points) of the bitmap-grid clouds, for the grid build
	std::vector<uint32_t> ajobs_h; // jobs that start a trip of 1024 source slots: k_accum's workgroups (indices into jobs_h) — per sub-batch slice,
								   // and inside a slice grouped by trip length (ajob_split)
	uint32_t ajob_split[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}; // [sub-batch][0..3]: the slice's trips of > 512, 257..512, <= 256 slots
	IcpOut *icp_outs_pin = nullptr; // the result records of a device-stepped run, downloaded into pinned memory (results_from_device)
	size_t cap_icp_pin = 0;
	std::string jobs_key;
	uint32_t njobs = 0;
	// device (besides BatchDev's)
	uint4 *nn_cand = nullptr; // per source point: candidate record of the k-candidate certificates (RunParams::cand)
	LiveWord *live_mask = nullptr; // live-point compaction: one word per 64 source slots and one more per class cloud (RunParams::live_mask, device_types.h)
	size_t cap_live = 0;
	uint32_t tick = 1; // duplicate-table epoch counter of THIS batch's winner table, monotone between resets (take_epochs)
	size_t cap_outs = 0;
	size_t cap_big[4] = {};
	size_t cap_bjobs[4] = {};
	size_t cap_bm_cs = 0;
	size_t cap_bm_rank = 0;
	size_t cap_ajobs = 0;
	size_t cap_icp_outs = 0;
	size_t cap_steps = 0;
	uint32_t epoch2 = 0, epoch3 = 0; // the device-stepped loop's last epochs issued on its 8-byte words (words 32-33 / 48-49 of epoch_h: one per sub-batch)
	int nsub = 1;		 // sub-batches the job tables are laid out for (build_jobs)
	double fill_ms = 0.0, fill_pack_ms = 0.0; // the last batch_fill: wall time, host packing time ...
	uint64_t fill_bytes = 0;				   // ... and bytes staged
	size_t cap_wl = 0;
	unsigned long long *dbg = nullptr; // diagnostics (MULLS_OPT_DEBUG_STOP = 20): RunParams::dbg_ticks
	size_t cap_bm = 0, cap_pf = 0;
	// pinned, device-mapped host memory (zero-copy): per-iteration pair states in, per-pair sums out, completion epoch
	PairState *states_h = nullptr;
	PairOut *outs_h = nullptr;
	volatile uint32_t *epoch_h = nullptr;
	uint32_t *epoch_dev = nullptr;
	uint32_t epoch = 0;			// last epoch issued on word 0 (sub-batch 0 and the single-shot entry points)
	uint32_t epoch1 = 0;		// last epoch issued on word 16 (sub-batch 1)
	uint32_t *bbox_h = nullptr;
	uint8_t *upload_h = nullptr; // pinned staging buffer of the caller's point records
	CloudDesc *descs_init = nullptr; // pristine descriptors (device): restored into `descs` by a D2D copy every run
	uint32_t *bbox_init = nullptr;
	std::string dev_key;			 // jobs_key of the tables currently resident on the device
	size_t cap_jobs[6] = {}, cap_cells[2] = {};
	// capacities (elements) of the grow-only arrays
	size_t cap_stage = 0, cap_src[13] = {}, cap_tgt[5] = {}, cap_pairs[5] = {}, cap_setup_jobs = 0, cap_pin[4] = {};
};

namespace mulls_drv
{
using mulls::Mat4;
using mulls::Mat6;

inline float ord_to_float(uint32_t k)
{
	const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
	float f;
	std::memcpy(&f, &u, sizeof(f));
	return f;
}
inline int metric_of(int c) { return (c == MULLS_PILLAR || c == MULLS_BEAM) ? 1 : (c == MULLS_VERTEX ? 2 : 0); }
// packed index of (r,c), r <= c, in the row-major-upper enumeration used by k_accum
inline int packed(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }
void rows12(const double colmajor[16], double out[12]);

// host-side life of one pair during a run: the shared per-iteration state (icp_step.h) + host-only bookkeeping
struct PairHost : mulls::PairIter
{
	bool first = true;
	uint32_t alive_prev[MULLS_NC];
};

void fill_crop_box(const RunParams &rp, const double tgt_bound[6], const uint32_t keys[6], mulls_result &R);
int check_params(mulls_ctx *ctx, const mulls_params *P);
void init_cert(const mulls_ctx *ctx, RunParams &rp);
int subbatch_count(const mulls_ctx *ctx, int n);
void options_init(mulls_ctx *ctx);
bool option_value_ok(int option, double *value);
uint32_t lds_dedup_max_pts();
void assign_tiers(mulls_batch *B, const uint8_t used[MULLS_NC], int mode);
void build_jobs(mulls_batch *B, const mulls_params *P, int nsub, int mode);
// `last`: while profiling, the event recorded behind the k_finish that publishes `want` — waiting on it (instead of the whole stream) leaves the
// other sub-batch's kernels running
int wait_epoch_word(mulls_ctx *ctx, volatile uint32_t *word, uint32_t want, hipEvent_t last = nullptr, hipStream_t stream = nullptr);
inline int wait_epoch(mulls_ctx *ctx, mulls_batch *B) { return wait_epoch_word(ctx, B->epoch_h, B->epoch); }
void unpack_out(const mulls_batch *B, const uint8_t used[MULLS_NC], int p, PairOut &o, bool comb = false);
uint32_t lds_cells_for(uint32_t cap);
// P_mixed: the caller can run a batch whose class clouds are on different tiers (mulls_batch_run): auto mode may answer 3
int choose_tier(const mulls_ctx *ctx, const mulls_batch *B, const uint8_t used[MULLS_NC], uint32_t *lds_cap, const mulls_params *P_mixed = nullptr);
int batch_fill(mulls_ctx *ctx, mulls_batch *B, const mulls_pair *pairs, int n, const mulls_params *P = nullptr);
// nsub: sub-batches the lock-step job tables are laid out for (0 = subbatch_count)
int prepare_run(mulls_ctx *ctx, mulls_batch *B, const mulls_params *P_jobs, RunParams &rp, uint32_t *lds_cap_out, int *tier_out, int nsub = 0, bool allow_mixed = false);
// the launch sequences the entry points share (batch.cpp, behind prepare_run); st: where the set-up goes, ctx->stream otherwise
void queue_clone_crop(hipStream_t st, const mulls_batch *B, const RunParams &rp);
bool setup_former_shape(const RunParams &rp);
int apply_keep_masks(mulls_ctx *ctx, const mulls_batch *B, const std::vector<uint8_t> &skeep, const std::vector<uint8_t> &tkeep, const char *what);
void queue_target_grids(hipStream_t st, const mulls_batch *B, const RunParams &rp, int tier, bool fused_tgt);
int queue_tier_search(mulls_ctx *ctx, const mulls_batch *B, const RunParams &rp, int tier, uint32_t lds_cap, uint32_t parity);
mulls::IcpConst icp_const(const mulls_params *P);
int take_epochs(mulls_ctx *ctx, mulls_batch *B, uint32_t n, RunParams &rp);

struct EvTimer
{
	mulls_ctx *ctx;
	hipStream_t stream = nullptr; // where its events are recorded (default: ctx->stream)
	int base = 0; // first event of this timer's set in ctx->ev
	int used = 0;
	bool open = false;
	double *slot[5];
	void begin(double *acc)
	{
		open = ctx->profiling == 1 || (ctx->profiling == 2 && acc == &ctx->prof.ms_nn);
		if (!open)
			return;
		slot[used / 2] = acc;
		(void)hipEventRecord(ctx->ev[base + used], stream ? stream : ctx->stream);
	}
	void end()
	{
		if (!open)
			return;
		open = false;
		(void)hipEventRecord(ctx->ev[base + used + 1], stream ? stream : ctx->stream);
		used += 2;
	}
	hipEvent_t last() const { return (ctx->profiling == 1 && used) ? ctx->ev[base + used - 1] : nullptr; }
	void collect() // after the last recorded event completed
	{
		for (int i = 0; i < used; i += 2)
		{
			float ms = 0;
			if (hipEventElapsedTime(&ms, ctx->ev[base + i], ctx->ev[base + i + 1]) != hipSuccess)
			{
				(void)hipEventSynchronize(ctx->ev[base + i + 1]);
				(void)hipEventElapsedTime(&ms, ctx->ev[base + i], ctx->ev[base + i + 1]);
			}
			*slot[i / 2] += ms;
		}
		used = 0;
	}
};
} // namespace mulls_drv
