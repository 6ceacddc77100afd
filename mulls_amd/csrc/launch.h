// launch.h — host-callable wrappers around the kernels in k_setup / k_grid / k_search / k_reduce .hip (each unit defines its own).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "device_types.h"

#include <hip/hip_vector_types.h>
#include <mutex>

// Launch state that belongs to a DEVICE, not to the process: hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the device that is current at the call, and
// the CU count is the device's.  mulls_create(device) allows contexts on several GPUs of one process (and every host thread may own one), so each launch wrapper
// keeps one DevLaunch per device, set up under a lock by the first launch on that device.  TAG: one table per wrapper.
struct DevLaunch
{
	bool ready = false, ok = false;
	size_t dyn_max[2] = {0, 0}; // dynamic LDS the wrapper's kernels may ask for on this device
	uint32_t n_cu = 256;
};
template <int TAG, class Init>
inline DevLaunch dev_launch(Init init)
{
	static std::mutex mu;
	static DevLaunch table[64];
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
		dev = 0;
	std::lock_guard<std::mutex> lock(mu);
	DevLaunch &D = table[dev];
	if (!D.ready)
	{
		int cus = 0;
		if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
			D.n_cu = (uint32_t)cus;
		D.ok = init(D);
		D.ready = true;
	}
	return D;
}
namespace mulls
{
struct IcpConst;
struct StepState;
} // namespace mulls
// The device arrays of a batch, as the wrappers below hand them to the kernels (mulls_batch, batch.h, derives from it and owns the memory: capacities, host mirrors
// and epochs live there).  A wrapper takes the view and, besides it, only what its call sites choose: a slice of a job table, counts, a parity, an epoch.
struct BatchDev
{
	float4 *stage = nullptr;
	float4 *tmp_pos = nullptr, *tmp_nrm = nullptr;
	float4 *spos = nullptr, *snrm = nullptr, *tpos = nullptr, *tnrm = nullptr;
	uint8_t *flag = nullptr;
	int32_t *match = nullptr, *nn_idx = nullptr, *nn_hint = nullptr;
	float4 *mq = nullptr; // per source point: position and direction of its matched target (2 records), written with match[]
	float *wd = nullptr, *nn_d2 = nullptr;
	unsigned long long *winner = nullptr;
	CloudDesc *descs = nullptr;
	PairSetup *setup = nullptr;
	PairState *states = nullptr;	 // HBM copy of the pair states (filled by k_push_states every iteration)
	PairState *states_pin = nullptr; // device address of the pinned host array states_h
	PairOut *outs = nullptr;		 // HBM: filled by k_finish
	PairOut *outs_pin = nullptr;	 // device address of the pinned host array outs_h (packed records, k_pull_outs)
	uint32_t *bbox = nullptr;
	Job *setup_jobs = nullptr;
	uint32_t *setup_tab = nullptr; // the setup's index tables, one array (mulls_batch::setup_tab_h): k_tgt_grid's buckets, k_crop's workgroups, k_src_setup's pairs
	Job *big_segs = nullptr, *big_clouds = nullptr;
	uint32_t *seg_cnt = nullptr, *big_box = nullptr;
	Job *jobs = nullptr;
	double *partial = nullptr;
	Job *tjobs = nullptr;
	Job *cjobs = nullptr;
	Job *bjobs = nullptr, *fjobs = nullptr, *ejobs = nullptr;
	uint32_t *lclouds = nullptr;
	uint32_t *bm_cs = nullptr;	 // bitmap grids: first sorted position of every occupied cell (indexed like cell_cnt)
	uint32_t *bm_rank = nullptr; // bitmap grids: every target point's (cell counter index, arrival number in its cell), from k_bm_count to k_bm_scatter — the scatter is
								 // pure data movement: one pass of atomics per build instead of two
	uint32_t *ajobs = nullptr;
	IcpOut *icp_outs = nullptr;
	mulls::StepState *steps = nullptr; // lock-step loop with the device step: per-pair loop state
	uint32_t *wl = nullptr;		// LDS tier: class clouds k_cert queued for k_nn_lds (one slot per class-level job)
	uint32_t *wl_ctr = nullptr; // ... and the queue counters: per sub-batch 8 words = (queued, taken) x launch parity
	GridDesc *grids = nullptr;
	float4 *tsorted = nullptr;
	uint16_t *tmap = nullptr; // LDS tier without a cropped copy of the target clouds (k_tgt_grid): rank in the cropped cloud -> staged index
	uint32_t *cell_cnt = nullptr, *cell_start = nullptr; // bitmap grids: per-occupied-cell counters (start positions: bm_cs); LDS tier: dense cell tables
	unsigned long long *bm = nullptr;					  // global tier: occupancy words of every grid
	uint32_t *pf = nullptr;								  // global tier: occupied cells before each word
	uint32_t *ticket = nullptr; // device: arrival counters of k_finish (one per sub-batch, 16 words apart)
};
// clone + initial guess of the `njobs` setup jobs (b.setup_jobs)
void launch_clone_src(hipStream_t st, const BatchDev &b, const RunParams &rp, uint32_t njobs);
// nbig_segs / nbig_clouds: entries of b.big_segs / b.big_clouds (class clouds cropped segment-wise)
// wgs / nwgs: the (pair, class, side) workgroups k_crop starts (device table; null: every side of the `npairs` pairs)
void launch_crop(hipStream_t st, const BatchDev &b, const RunParams &rp, uint32_t npairs, uint32_t nbig_segs, uint32_t nbig_clouds, const uint32_t *wgs = nullptr, uint32_t nwgs = 0);
// clone + box + crop of the source side of the `npairs` pairs listed in `pairs` (device), one workgroup each (k_src_setup: runs that do not undistort)
void launch_src_setup(hipStream_t st, const BatchDev &b, const RunParams &rp, const uint32_t *pairs, uint32_t npairs);
// n byte ranges in one launch per MULLS_COPY_SEGS of them (device_types.h: CopySeg)
void launch_copy_segs(hipStream_t st, const CopySeg *segs, uint32_t n);
// CFilter::apply_motion_compensation on `n` 48-byte records in device memory (q: w x y z of Tran's rotation, t: its translation)
void launch_motion_comp(hipStream_t st, float4 *recs, uint32_t n, const double q[4], const double t[3], float thre);
void launch_thin(hipStream_t st, const BatchDev &b, uint32_t npairs, const uint8_t *src_keep, const uint8_t *tgt_keep);
// LDS tier with rp.tgt_map: crop + grid build of every target class cloud (<= MULLS_LDS_MAXPTS points) in one pass, no working copy (k_grid.hip)
// clouds / split: size-bucket tables of the LDS-tier class clouds (device) and their MULLS_TG_BUCKETS + 1 bounds; null: one full-reach workgroup per class cloud
int launch_tgt_grid(hipStream_t st, const BatchDev &b, const RunParams &rp, uint32_t npairs, const uint32_t *clouds = nullptr, const uint32_t *split = nullptr);
const uint32_t *tgt_grid_bucket_trips(); // [MULLS_TG_BUCKETS]: x 512 points = the largest cloud of each bucket
// LDS tier without the fused setup (k_crop wrote the cropped copies)
void launch_grid_build_sort(hipStream_t st, const BatchDev &b, const RunParams &rp, uint32_t npairs);
// bitmap grids of the `nl` class clouds b.lclouds[] (pair * MULLS_NC + class each); ntjobs: their 256-point chunks (b.tjobs)
void launch_bm_build(hipStream_t st, const BatchDev &b, uint32_t nl, uint32_t ntjobs);
size_t nn_lds_bytes(uint32_t cap, uint32_t maxcells, bool dedup);
// wl, wl_ctr: the slice's part of b.wl and the sub-batch's counters in b.wl_ctr
int launch_nn_lds(hipStream_t st, const BatchDev &b, const RunParams &rp, const Job *jobs, uint32_t njobs, uint32_t cap, uint32_t *wl, uint32_t *wl_ctr, uint32_t parity,
				  bool first = false);
// a small mixed batch: the class clouds of both tiers in one launch (k_cert_mixed); returns 1 when it launched, 0 when the caller has to launch the tiers separately
int launch_cert_mixed(hipStream_t st, const BatchDev &b, const RunParams &rp, const Job *cjobs, uint32_t n_lds, const Job *bjobs, uint32_t n_big, uint32_t max_wgs, uint32_t rounds,
					  uint32_t cap, bool first = false);
// global-memory tier (big_tier.h): class-level (MULLS_JOB_CLASS) and chunk-level jobs; max_wgs: chunk-level jobs are shared by 2 / 4 / 8 / 16 workgroups while
// the launch stays within this many
void launch_cert_big(hipStream_t st, const BatchDev &b, const RunParams &rp, const Job *jobs, uint32_t njobs, uint32_t max_wgs);
void launch_nn(hipStream_t st, const BatchDev &b, const RunParams &rp, const Job *jobs, uint32_t njobs);
void launch_nn_shoot(hipStream_t st, const BatchDev &b, const RunParams &rp, const Job *jobs, uint32_t njobs);
void launch_filter(hipStream_t st, const BatchDev &b, const RunParams &rp, const Job *jobs, uint32_t njobs, bool big = false);
// b.ajobs: job indices of the trip starts, grouped by trip length (split[0..3]: see k_reduce.hip)
void launch_accum(hipStream_t st, const BatchDev &b, const RunParams &rp, const uint32_t split[4], bool single = false, uint32_t wave_min_trips = 0);
// whether launch_accum sums these trips by one wave each (k_accum_wave) — the accumulation that reads a compacted class cloud (RunParams::live_mask)
bool accum_takes_waves(const RunParams &rp, const uint32_t split[4], uint32_t wave_min_trips);
void launch_finish(hipStream_t st, const BatchDev &b, const RunParams &rp, uint32_t pair_base, uint32_t npairs, uint32_t *ticket, volatile uint32_t *host_epoch, uint32_t epoch);
void launch_push_states(hipStream_t st, const BatchDev &b, uint32_t pair_base, uint32_t npairs);
// lock-step loop with the O(1) half of the iteration on the device: initial per-pair state and first PairState; k_finish followed by the step (k_step)
void launch_step_init(hipStream_t st, const BatchDev &b, const mulls::IcpConst &K, uint32_t npairs);
void launch_finish_step(hipStream_t st, const BatchDev &b, const RunParams &rp, const mulls::IcpConst &K, uint32_t pair_base, uint32_t npairs, unsigned long long *host_word, uint32_t epoch,
						int brute, uint32_t *ticket = nullptr, bool sum_step = false); // ticket: two zeroed device words -> finish, step and publication in one launch (small batches);
						// sum_step (large batches): one wave per pair sums and steps (k_sum_step) instead of k_finish + k_step
void launch_transform_aos(hipStream_t st, float4 *recs, uint32_t n, const double *T12);
// cs, ct, cd: the caller's correspondence list (device copies), forced into the batch's flag / match / wd / mq arrays
void launch_set_corr(hipStream_t st, const BatchDev &b, uint32_t src_off, const int32_t *cs, const int32_t *ct, const float *cd, uint32_t n, uint32_t tgt_off);
