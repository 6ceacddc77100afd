/*
 * mulls_hip.h — C ABI of libmulls_hip.so, the MI355X (gfx950) implementation of the MULLS-ICP hot path.
 *
 * What this boundary replaces (all citations relative to the MULLS reference tree):
 *   CRegistration<PointT>::mm_lls_icp()            include/common/cregistration.hpp:1114-1440
 *   CRegistration<PointT>::determine_corres()      include/common/cregistration.hpp:1701-1835
 *   multi_metrics_lls_tran_estimation() + pt2pl/pt2li/pt2pt summations
 *                                                  include/common/cregistration.hpp:1869-2275
 *   get_multi_metrics_lls_residual()               include/common/cregistration.hpp:2518-2677
 *   intersection_filter()                          include/common/cregistration.hpp:2894-2922
 *
 * The reference has no FFI: mm_lls_icp is a member of a header-only class template.  The drop-in is therefore
 * (i) this C ABI (plain pointers + sizes, no C++/torch types) and (ii) include/cregistration_hip.hpp, which
 * re-creates the member function with its verbatim signature and marshals pcl clouds into the structs below
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - Feature-class index == character index of the reference's `used_feature_type` string
 *     (cregistration.hpp:1196-1201, :1213-1232): 0 ground, 1 pillar, 2 facade, 3 beam, 4 roof, 5 vertex.
 *   - Points are pcl::PointXYZINormal records (48 B): x@0 y@4 z@8 | normal_x@16 normal_y@20 normal_z@24 |
 *     intensity@32 curvature@36.  `stride` is the byte distance between records (48 for PCL clouds).
 *   - Matrices are column-major doubles (Eigen's default), 4x4 -> [16], 6x6 -> [36].
 *   - Every entry point returns 0 on success or a negative MULLS_E_* infrastructure error.  The reference's
 *     registration status (1, -1, -2, -3, 0; cregistration.hpp:1131-1136) is returned in mulls_result.code.
 *     Nothing is thrown across the ABI.
 *   - Caller memory is only borrowed for the duration of a call.
 */
#ifndef MULLS_HIP_H
#define MULLS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MULLS_NCLASS 6
#define MULLS_POINT_BYTES 48

enum mulls_class
{
	MULLS_GROUND = 0, /* point-to-plane */
	MULLS_PILLAR = 1, /* point-to-line  */
	MULLS_FACADE = 2, /* point-to-plane */
	MULLS_BEAM = 3,	  /* point-to-line  */
	MULLS_ROOF = 4,	  /* point-to-plane */
	MULLS_VERTEX = 5  /* point-to-point */
};

enum mulls_error
{
	MULLS_OK = 0,
	MULLS_E_INVALID = -100,	   /* bad argument */
	MULLS_E_HIP = -101,		   /* a HIP runtime call failed (see mulls_last_error) */
	MULLS_E_NO_DEVICE = -102,  /* no gfx950 device / kernels could not be loaded */
	MULLS_E_UNSUPPORTED = -103, /* option not implemented by this build */
	MULLS_E_IO = -104,		   /* file could not be opened / is not in the expected format */
	MULLS_E_NOMEM = -105	   /* a host allocation failed (e.g. sizes that cannot be real) */
};

/* One feature-class cloud, borrowed from the caller (AoS of 48-byte PointXYZINormal records). */
/* pts may also be a device pointer obtained from mulls_map_cloud() (stride 48 only). */
typedef struct mulls_cloud
{
	const void *pts;
	uint32_t n;
	uint32_t stride;
} mulls_cloud;

/* One registration problem = the reference's constraint_t inputs (utility.hpp:561-590).
 *   tgt[c]      block1->pc_{ground,pillar,facade,beam,roof,vertex}                 (cregistration.hpp:1180)
 *   src[c]      block2->pc_*_down, or block2->pc_* when use_more_points; src[5] is always block2->pc_vertex (:1181)
 *   src_down[c] block2->pc_*_down, only read when params.undistort (cregistration.hpp:1251-1253); may be all-zero
 *   tgt_bound   block1->local_bound as {min_x,min_y,min_z,max_x,max_y,max_z}       (cregistration.hpp:2916)
 *   init_guess  the by-value Eigen::Matrix4d initial_guess, column-major           (cregistration.hpp:1120) */
typedef struct mulls_pair
{
	mulls_cloud tgt[MULLS_NCLASS];
	mulls_cloud src[MULLS_NCLASS];
	mulls_cloud src_down[MULLS_NCLASS];
	double tgt_bound[6];
	double init_guess[16];
} mulls_pair;

/* The positional arguments of mm_lls_icp (cregistration.hpp:1114-1123), in order, plus ABI-only knobs at the end. */
typedef struct mulls_params
{
	int32_t max_iter_num;			 /* 20 */
	float dis_thre_unit;			 /* 1.5 */
	float converge_translation;		 /* 0.002 */
	float converge_rotation_d;		 /* 0.01 */
	float dis_thre_min;				 /* 0.4 */
	float dis_thre_update_rate;		 /* 1.1 */
	char used_feature_type[8];		 /* "111110" */
	char weight_strategy[8];		 /* "1101" */
	float z_xy_balanced_ratio;		 /* 1.0 */
	float pt2pt_residual_window;	 /* 0.1 */
	float pt2pl_residual_window;	 /* 0.1 */
	float pt2li_residual_window;	 /* 0.1 */
	uint8_t apply_intersection_filter; /* true */
	uint8_t apply_motion_undistortion; /* false */
	uint8_t normal_shooting_on;		   /* false */
	uint8_t use_more_points;		   /* false (only decides which clouds the adapter passes as src[]) */
	float normal_bearing;			 /* 45.0 */
	uint8_t keep_less_source_points; /* false */
	uint8_t faithful;				 /* ABI-only. 1 = reproduce reference quirks (pt2li off-diagonals dropped,
										vertex residual weighted by d^2); 0 = mathematically intended version */
	uint8_t rejector_strict;		 /* ABI-only. 1 (default): pcl::registration::CorrespondenceRejectorDistance::getRemainingCorrespondences as PCL 1.7-1.12 ship it
										(registration/src/correspondence_rejection_distance.cpp: `original_correspondences[i].distance < max_distance_`,
										max_distance_ = the float square set by setMaximumDistance; a NaN distance is dropped).  0: `distance <= max^2` (NaN kept),
										the reading SURVEY.md A.4-3 wrote down.  The two differ only on correspondences whose float distance equals the float
										threshold exactly (tests/test_pcl_operators.py counts them: none on the bench workload) */
	uint8_t reserved_;
	float sigma_thre;				 /* 0.5 */
	float min_neccessary_corr_ratio; /* 0.03 */
	float max_bearable_rotation_d;	 /* 45.0 */
	uint64_t rng_seed;				 /* ABI-only. keep_less_source_points thins with an order-preserving selection sampling (Knuth's
										Algorithm S driven by splitmix64(rng_seed ^ cloud id)); the reference uses pcl::RandomSample
										seeded with time(NULL) (cfilter.hpp:620), i.e. a different subset on every run */
} mulls_params;

/* Optional per-iteration record (debug / parity triage).  Filled when mulls_result.trace != NULL. */
typedef struct mulls_iter_trace
{
	int32_t iter;
	uint32_t ncorr[MULLS_NCLASS]; /* correspondences that entered the estimation (after all rejectors) */
	uint32_t nsrc[MULLS_NCLASS];  /* live source points of the class after this iteration's search */
	float thr[MULLS_NCLASS];	  /* dis_thre used by this iteration's search */
	double atpa[36];			  /* normal matrix after the mirror step (cregistration.hpp:1924-1938) */
	double atpb[6];
	double x[6];				  /* tx ty tz roll pitch yaw of this step */
} mulls_iter_trace;

typedef struct mulls_result
{
	int32_t code;		/* 1 ok, -1 step too large, -2 too few correspondences, -3 sigma too large, 0 loop never ran */
	int32_t iters;		/* iterations whose correspondence search ran */
	double T[16];		/* constraint_t::Trans1_2, column-major (cregistration.hpp:1405) */
	double info[36];	/* constraint_t::information_matrix, column-major (:1418) */
	float sigma;		/* constraint_t::sigma (:1419) */
	float confidence;	/* constraint_t::confidence (:1420) */
	uint32_t ncorr[MULLS_NCLASS]; /* correspondences per class at the last search */
	uint32_t nsrc0[MULLS_NCLASS]; /* source points per class after the intersection filter */
	uint32_t ntgt0[MULLS_NCLASS]; /* target points per class after the intersection filter */
	int32_t singular;			  /* ABI-only: 1 if a non-finite solve was observed (reference does not check, B-11) */
	int32_t cropped;			  /* 1 if the intersection filter ran (cregistration.hpp:1186-1188) */
	double crop_box[6];			  /* its box {min_x,min_y,min_z,max_x,max_y,max_z} (utility.hpp:857-865); the adapter re-creates
									 the reference's kd-tree side effect on block1 from it */
	float ms_total;				  /* wall time of this registration inside the library (batch: batch time / n) */
	mulls_iter_trace *trace;	  /* in: caller array or NULL */
	int32_t trace_cap;			  /* in: capacity of trace[] */
	int32_t trace_len;			  /* out */
} mulls_result;

/* Per-kernel device time of the last mulls_batch_run, measured with hipEvents on the library's stream
 * when mulls_set_profiling(ctx, 1) is on (adds one event pair per launch group and waits on events; keep off for throughput runs).
 * mulls_set_profiling(ctx, 2): only the correspondence search is bracketed (ms_nn, launches_nn and the counters; the other ms_* stay 0) —
 * two events per iteration, the iteration hand-over as without profiling. */
typedef struct mulls_profile
{
	double ms_setup;	  /* clone + initial guess + intersection filter kernels */
	double ms_nn;		  /* correspondence-search kernel, summed over launches */
	double ms_filter;	  /* duplicate / distance / direction rejection kernel */
	double ms_accum;	  /* normal-equation accumulation kernel (+ partial finish) */
	double ms_residual;	  /* posterior residual kernel */
	int32_t launches_nn;  /* number of correspondence-search launches in the run */
	int32_t iterations;	  /* lock-step iterations executed by the run */
	uint64_t nn_pair_evals; /* source-target distance evaluations issued by those launches */
	uint64_t nn_src_pts;	/* live source points searched, summed over launches */
	uint64_t nn_tgt_pts;	/* target points streamed into LDS (once per 512-source job), summed over launches */
	double ms_host_step;	/* host time spent in the per-iteration algebra (6x6 solves, tests, next states), summed over iterations; 0 when the
							   loop steps on the device (every run without per-iteration traces) */
	double ms_host_wait;	/* host time spent waiting for the device epoch, summed over iterations */
	double ms_host_launch;	/* host time spent enqueueing the launch set, summed over iterations */
	uint64_t nn_tgt_unique; /* target points of the searched class clouds (once per cloud), summed over launches */
	uint64_t nn_corr_pts;	/* loop stepped on the device: correspondences that entered the estimation, summed over the iterations (0 when the
							   host steps the loop) */
	double icp_fused_ms[6];	/* diagnostics of a loop stepped on the device, 0 otherwise.  MULLS_OPT_DEBUG_STOP = 20: k_cert's phase clocks summed over
							   its workgroups ([0..4], ms) and the workgroup count ([5]); = 21: the global-memory tier's leftover queries ([0]) and
							   its workgroup time ([1], ms) */
	double icp_search_ms[24]; /* ... MULLS_OPT_DEBUG_STOP = 20: k_cert's k-candidate certificates — points the plain certificate left over, points
							   given the second chance, points it certified, points searched ([0..3]); [4]: slots the live-point compaction took out of the
						   later searches' walks (0: nothing was compacted); 0 otherwise */
	double icp_phase_ms[6]; /* ... MULLS_OPT_DEBUG_STOP = 20: k_nn_lds's phase clocks summed over its class clouds ([0..3], ms) and the class cloud
							   count ([4]); 0 otherwise, and [5] always */
	double ms_stage;		/* mulls_icp / mulls_icp_batch: wall time of staging the caller's clouds (host gather into pinned memory + upload), */
	double ms_stage_pack;	/* ... of which the host gather, */
	uint64_t stage_bytes;	/* ... and the bytes that crossed PCIe */
} mulls_profile;

typedef struct mulls_ctx mulls_ctx;		/* one per host thread / HIP stream */
typedef struct mulls_batch mulls_batch; /* device-resident set of pairs */

void mulls_default_params(mulls_params *p);

int mulls_create(int device, mulls_ctx **out);
void mulls_destroy(mulls_ctx *ctx);
const char *mulls_last_error(const mulls_ctx *ctx);
int mulls_set_profiling(mulls_ctx *ctx, int on);
int mulls_get_profile(const mulls_ctx *ctx, mulls_profile *out);
/* correspondence-search tier: 0 = auto, 1 = LDS-tiled brute force, 2 = uniform grid in global memory, 3 = uniform grid staged in LDS with lock-step
 * launches (MULLS_E_INVALID when a searched target class cloud exceeds 9728 points), 4 = the same as 3 (kept for existing callers).
 * Auto: searched target class clouds of <= 9728 points -> the grid staged in LDS, stepped by lock-step launch sets (the O(1) half of the iteration
 * on the device too); larger targets -> the grid in global memory.  All tiers are exact and return bit-identical results (tests/test_gpu_stages.py,
 * test_gpu_icp.py). */
int mulls_set_nn_mode(mulls_ctx *ctx, int mode);
/* Execution options of a context (none of them changes a result: every path returns the same bits).  mulls_create presets each from the environment
 * variable named after it (MULLS_OPT_HOST_STEP <- MULLS_HOST_STEP=1, ...: diagnostics and the A/B scripts under tools/); nothing reads the
 * environment after that.
 * The tests that hold the options to "the same bits" (a form's every output field against the default form's, the default's against the oracle):
 * tests/test_gpu_icp.py and tests/test_gpu_mixed.py (the launch forms, k-candidate certificates, fused target setup, tiers), tests/test_gpu_options.py
 * (certificates and their slack, cell edges, LDS_DEDUP, FIRST_DIRECT, sub-batches and streams, the split window, LEAN_STAGING). */
enum mulls_option
{
	MULLS_OPT_HOST_STEP = 0,			  /* [0] 1: the lock-step loop is stepped by the host (what per-iteration traces switch on anyway) */
										  /* 1, 2: reserved (mulls_set_option / mulls_get_option return MULLS_E_INVALID) */
	MULLS_OPT_FEW_LAUNCHES_MAX_PAIRS = 3, /* [640; 384 until round 6: +1 % at 384 - 512 pairs] lock-step loop: batches up to this size run 3 - 4 launches per iteration instead of 7 (one accumulation launch;
											 finish + step + publication as one kernel; light and heavy pass of the search as one launch while there are at most
											 two class clouds per CU) — small batches are bound by the launch count */
	MULLS_OPT_SUBBATCHES = 4,			  /* [0 = by batch size] host-stepped loop: sub-batches in flight (1 or 2) */
	MULLS_OPT_TWO_STREAMS = 5,			  /* [0] host-stepped loop: the second sub-batch on a second stream */
	MULLS_OPT_CERTIFICATES = 6,			  /* [1] LDS tier: certified correspondences (0: every point is searched every iteration; MULLS_NO_CERT=1) */
	MULLS_OPT_CERT_SLACK_MIN = 7,		  /* [0.02 m] how much farther than the hinted target a searched query sweeps: */
	MULLS_OPT_CERT_SLACK_MAX = 8,		  /* [0.10 m]   clamp(rate * distance moved, min, max)                          */
	MULLS_OPT_CERT_SLACK_RATE = 9,		  /* [1.0] */
	MULLS_OPT_LDS_DEDUP = 10,			  /* [1] LDS tier: duplicate rule and rejection chain inside the search kernels (0: k_filter; MULLS_NO_LDS_DEDUP=1) */
	MULLS_OPT_GRID_H0 = 11,				  /* [0 = 1.3 m] LDS tier: preferred cell edge */
	MULLS_OPT_BM_H0 = 12,				  /* [0 = from the point spacing] global-memory tier: one fixed cell edge for every cloud */
	MULLS_OPT_LEAN_STAGING = 13,		  /* [0] mulls_icp / mulls_icp_batch stage only what the registration reads: the classes of used_feature_type (plus the
											 source ground / pillar / facade clouds the intersection box is taken from).  mulls_result.nsrc0 / ntgt0 of the
											 classes left out report 0; every output of the reference's interface is unchanged.  The C++ bridge switches it on. */
	MULLS_OPT_DEBUG_STOP = 14,			  /* [0] kernel bring-up switches (tools/gpu_time_nn.py; the values: tools/README.md).  30: the setup of a run in its
											 former shape — k_clone_src + k_crop for every pair, one 19-trip k_tgt_grid workgroup per class cloud.  31: no live-point
										 compaction after iteration 0's staged search (the searches walk every slot of every class cloud, as they did before it) */
	MULLS_OPT_DEBUG_TICK = 15,			  /* [0] tests: start a fresh batch's duplicate-table epoch counter here */
	MULLS_OPT_SPLIT_MIN_PAIRS = 16,		  /* [96]    lock-step loop stepped on the device: batches of MIN .. MAX pairs iterate as two sub-batches on two streams, */
	MULLS_OPT_SPLIT_MAX_PAIRS = 17,		  /* [2^30]  so that one half's kernels fill the gaps of the other's (MAX < MIN: never; not while profiling: +3 % at */
										  /*         128 - 4096 pairs, nothing below 96, profiles/r03_modes.txt) */
	MULLS_OPT_FUSED_TGT_SETUP = 18,		  /* [1] LDS tier: the target class clouds are cropped and their grids built in one pass without a cropped working */
										  /*     copy (k_tgt_grid); 0 = k_crop + k_grid_build_sort.  Same results */
	MULLS_OPT_STAGGER = 19,				  /* [4352] bytes by which the k-th per-point array of a batch starts into its 2 MiB-aligned allocation (k x this): the same index of a dozen
										     arrays is then not the same offset into a dozen pages (+1.3 % at 4096 pairs, profiles/r03_sweeps.txt) */
	MULLS_OPT_STEP_LAUNCH_MAX_PAIRS = 20, /* [640] lock-step loop: batches up to this size run finish + step + publication as one launch (k_finish_step) even when they are
											 above FEW_LAUNCHES_MAX_PAIRS (which implies it): +2 % at 512 pairs, -2 % at 1024, -7 % at 4096 (one atomic per pair on one word) */
	MULLS_OPT_MIXED_TIERS = 21,			  /* [1] auto mode picks the search tier per (pair, class) cloud: the LDS tier for the down-sampled clouds, the global-memory
											 tier (certified correspondences on an occupancy-bitmap grid) for larger ones, both in one launch set; 0 = one tier per
											 batch, decided by its largest searched target cloud (rounds 1 - 3) */
	MULLS_OPT_BIG_EARLY_SETS = 22,		  /* [5; 2 until round 6: 32 scans against a 961 k-point map 5 940 -> 6 420 /s, 64 scans against 20 000-point maps unchanged] mixed batches: the first iterations run every global-memory-tier cloud as chunk-level jobs shared by several workgroups
											 (+ k_filter) — while most points still need a search that beats one workgroup per class cloud; from this iteration on the
											 down-sampled source clouds are class-level jobs (certificates, leftovers, rejection chain in one workgroup, no k_filter) */
	MULLS_OPT_KCERT = 23,				  /* [1] k-candidate certificates: a point whose hinted target fails the certificate evaluates the few nearest targets its last search
											 saw before it is searched again (0: round 4's certificates only).  In force on the global-memory tier (+4 ... 8 % there); the LDS tier's
											 kernels are built without them by default (keeping the records costs more than the look returns, lds_tier.h: MULLS_LDS_KCERT) */
	MULLS_OPT_KCERT_MIN = 24,			  /* [64] LDS tier, builds with MULLS_LDS_KCERT=1 only: leftover lists shorter than this skip the look (it costs one chain of round trips whatever the length) */
	MULLS_OPT_ACCUM_WAVE_MIN_TRIPS = 25,  /* [768; 2048 until round 6, when the kernel lost its memo and two thirds of its divisions: 512 pairs 185 -> 201 k/s, 768 pairs 211 -> 235 k/s] lock-step loop: from this many 1024-slot trips per launch on the normal equations are summed by one wave per trip (k_accum_wave:
											 the slots of a lane in sequence, the running sums in registers — no term buffer, no barriers; same bits; -0.26 ms of a 17.8 ms
											 step at 4096 pairs, profiles/r05_experiments.txt); 0 = always one workgroup per trip (k_accum).  Read when a batch is filled
											 and at every launch */
	MULLS_OPT_FIRST_DIRECT = 26,		  /* [1] LDS tier, lock-step loop: the setup applies iteration 0's rigid step (the identity) where it writes the cropped source clouds, and
											 iteration 0 runs no light pass — without hints it could only list every point and hand the class clouds over, or search a small
											 cloud unhinted against the grid in global memory: every called class cloud goes straight to the staged search.  0 = light pass
											 first, as in every other iteration.  Same bits */
	MULLS_OPT_SUM_STEP = 27,			  /* [1] lock-step loop stepped on the device, batches beyond STEP_LAUNCH_MAX_PAIRS: one wave per pair sums the pair's trip partials AND steps it
											 (k_sum_step) instead of k_finish followed by k_step — one launch less per iteration; a batch in which some class cloud has more than four
											 1024-slot trips (run_device_step in loop.cpp checks the batch's job tables before the first launch set) keeps the
											 two kernels.  0 = k_finish + k_step.  Same bits */
	MULLS_OPT_TEASER_DEVICE_SEARCH = 28,  /* [0] 1: the exact maximum-clique search of mulls_coarse_reg_teaser / mulls_coarse_reg_teaser_indexed runs on the device (k_teaser_clique.hip: a
											 chain of bounded launches, one wavefront per branch of the search tree) instead of on one host core.  Every result field is the same
											 bits whenever the search completes; clique_nodes, the effort, is not (see the TEASER block below).  Values other than 0 and 1 are
											 refused.  MULLS_TEASER_DEVICE_SEARCH=1 */
	MULLS_OPT_COUNT = 29
};
int mulls_set_option(mulls_ctx *ctx, int option, double value);
int mulls_get_option(const mulls_ctx *ctx, int option, double *value);
/* raw hipStream_t the library launches on (so callers can bracket it with their own events) */
void *mulls_stream(mulls_ctx *ctx);

/* replaces one mm_lls_icp call: upload, register, release */
int mulls_icp(mulls_ctx *ctx, const mulls_pair *pair, const mulls_params *params, mulls_result *result);

/* n independent pairs advanced in lock-step (one launch set + one host sync per ICP iteration for the batch) */
int mulls_icp_batch(mulls_ctx *ctx, const mulls_pair *pairs, int n, const mulls_params *params, mulls_result *results);

/* ---- independent scan pairs over several contexts of one process ("one host thread + one HIP stream set per GPU") ----
 * The reference has one kind of caller: a C++ program that holds its clouds in host memory (test/mulls_slam.cpp).  These two forms give such a caller
 * what bench.py's torch.distributed launcher gives the benchmark, without a second process:
 *
 * mulls_icp_batch_sharded: the n pairs block-partitioned over n_ctx contexts — pair p goes to context floor(p * n_ctx / n), as mulls_amd/shard.py does —
 *   one per GPU of the node (mulls_create(device k)), or several on one GPU; the calling thread drives the first shard, one host thread each of the others;
 *   results[p] is pair p's, the very bits mulls_icp_batch returns on one context.  No collective: the shards share nothing.  Returns the first failing
 *   shard's code (its context has the text).  The contexts must be distinct and not in use by another thread. */
int mulls_icp_batch_sharded(mulls_ctx *const *ctxs, int n_ctx, const mulls_pair *pairs, int n, const mulls_params *params, mulls_result *results);

/* mulls_pipe: calls from host buffers in flight on `depth` alternating contexts of one device, so that call k + 1's host gather and PCIe upload run under
 *   call k's kernels (a serial mulls_icp_batch caller waits for 9 ms of staging in front of 3.7 ms of kernels per 1024 pairs).
 *   mulls_icp_batch_begin returns a ticket (>= 0) at once — or, when the lane it falls on (ticket mod depth) is still running its previous call, as soon as
 *   that call has finished; a negative value is an error code.  pairs, the clouds they point to and results belong to the call until mulls_icp_batch_end(ticket)
 *   has returned its code (MULLS_OK: results[] are written).  A ticket can be waited for until its lane is given another call.
 *   mulls_pipe_set_option applies a mulls_option to every lane (it waits for running calls); mulls_pipe_ctx hands out a lane's context (profile, error text). */
typedef struct mulls_pipe mulls_pipe;
int mulls_pipe_create(int device, int depth, mulls_pipe **out);
void mulls_pipe_destroy(mulls_pipe *pipe);
int mulls_pipe_depth(const mulls_pipe *pipe);
mulls_ctx *mulls_pipe_ctx(mulls_pipe *pipe, int lane);
int mulls_pipe_set_option(mulls_pipe *pipe, int option, double value);
int mulls_icp_batch_begin(mulls_pipe *pipe, const mulls_pair *pairs, int n, const mulls_params *params, mulls_result *results);
int mulls_icp_batch_end(mulls_pipe *pipe, int ticket);

/* the n result records as rows of 56 doubles — T (16, column-major), information matrix (36), code, iterations, sigma, confidence — the table bench.py's ranks
 * gather over RCCL (mulls_amd/shard.py: RECORD); host code, no context */
void mulls_pack_results(const mulls_result *results, int n, double *table);

/* device-resident form: stage once, run many times (each run re-clones the staged clouds like
 * cloudblock_t::clone_feature does, utility.hpp:524-550) */
int mulls_batch_create(mulls_ctx *ctx, const mulls_pair *pairs, int n, mulls_batch **out);
int mulls_batch_run(mulls_ctx *ctx, mulls_batch *batch, const mulls_params *params, mulls_result *results);
void mulls_batch_destroy(mulls_ctx *ctx, mulls_batch *batch);

/* ---- variants of the path ---- */

/* lls_icp_3dof_ground (cregistration.hpp:1443-1582): ground class only, unknowns (roll, pitch, z).  Reads the like-named
 * fields of mulls_params: max_iter_num, dis_thre_unit, converge_translation, converge_rotation_d, dis_thre_min,
 * dis_thre_update_rate, weight_strategy[1..3], keep_less_source_points (+ rng_seed), max_bearable_rotation_d (the
 * reference's default for it is 10).  Only result->T and result->code are outputs of this variant (the reference
 * returns the code cast to bool). */
int mulls_icp_3dof_ground(mulls_ctx *ctx, const mulls_pair *pair, const mulls_params *params, mulls_result *result);
int mulls_icp_3dof_ground_batch(mulls_ctx *ctx, const mulls_pair *pairs, int n, const mulls_params *params, mulls_result *results);

/* mm_lls_icp_4dof_global (cregistration.hpp:1584-1681): sweeps the heading of the source about `station`
 * (block2->local_station) in steps of heading_step_d degrees; every trial is a full mm_lls_icp with classes "111110" and
 * weights "1001", all trials run as one lock-step batch; the trial maximising confidence / sigma wins.  pair->init_guess
 * is ignored.  converge_rotation_d and max_bearable_rotation_d are accepted for signature fidelity; the reference does
 * not use them (it passes converge_translation twice).  result->iters returns the number of trials.  *success: 0 = no trial
 * succeeded (the reference returns false), 1 = `result` is the best succeeded trial, 2 = trials succeeded but none scored above 0 (a NaN
 * sigma): the reference returns true and leaves the constraint untouched — `result` is then a placeholder (identity, sigma FLT_MAX). */
int mulls_icp_4dof_global(mulls_ctx *ctx, const mulls_pair *pair, float heading_step_d, const double station[3], int max_iter_num,
						  float dis_thre_unit, float converge_translation, float converge_rotation_d, float dis_thre_min,
						  float dis_thre_update_rate, float max_bearable_rotation_d, mulls_result *result, int *success,
						  float *best_heading_d);

/* ---- device-resident local map ----
 * MapManager::update_local_map (src/map_manager.cpp:18-140) with the six undown class clouds of `local_map` kept in HBM
 * between frames: the scan-to-map target is never re-uploaded (mulls_map_cloud() yields device clouds that mulls_pair.tgt
 * accepts), and map-based dynamic-object removal (map_manager.cpp:149-256) runs as an exact nearest-neighbour pass on the
 * device instead of querying the kd-trees mm_lls_icp left on block1.
 * Held to the oracle bit for bit on every record and report figure: tests/test_map.py and tests/test_gpu_map.py (update sequences),
 * tests/test_map_edges.py and tests/test_gpu_map_edges.py (inputs of tests/map_edges.py: clouds of many compaction segments, trees of
 * one to four search chunks with queries exactly on the removal's thresholds, neighbourhoods with ties at rank K, empty and non-finite
 * clouds, and these entry points by raw calls: packed strides, short downloads, NULL arguments, device-resident sources). */
typedef struct mulls_map mulls_map;

typedef struct mulls_map_params
{
	/* the positional arguments of update_local_map after the two blocks, in order (map_manager.h:21-31) */
	float local_map_radius;			   /* 80 */
	int max_num_pts;				   /* 20000 */
	int kept_vertex_num;			   /* 800 */
	float last_frame_reliable_radius;  /* 60; unused by the reference too */
	int map_based_dynamic_removal_on;  /* false */
	char used_feature_type[8];		   /* "111110" */
	float dynamic_removal_center_radius; /* 30.0 */
	float dynamic_dist_thre_min;	   /* 0.3 */
	float dynamic_dist_thre_max;	   /* 3.0 */
	float near_dist_thre;			   /* 0.03 */
	int recalculate_feature_on;		   /* true: principal directions of the map's pillar / beam points recomputed from their own
										  neighbourhoods, points that are not linear / steep / flat enough dropped (map_manager.cpp:98-118, :258-292) */
	/* not in the reference's signature */
	uint64_t rng_seed; /* random_downsample_pcl: the ABI's seeded selection sampling (see mulls_params.rng_seed) */
	int tree_mode;	   /* what block1->tree_* held after the last mm_lls_icp against this map (cregistration.hpp:1209-1232):
						* 0 = nothing (dynamic removal is skipped), 1 = the whole class clouds, 2 = the class clouds cropped to
						* tree_box (mulls_result.crop_box of that registration) */
	char tree_used[8]; /* used_feature_type of that registration: a class without a tree is left alone */
	double tree_box[6];
} mulls_map_params;

typedef struct mulls_map_report
{
	uint32_t n[6];			/* class cloud sizes of the map after the update */
	uint32_t frame_n[6];	/* sizes of the frame's clouds as appended (pc_*_down after dynamic removal; [5] = pc_vertex) */
	int feature_point_num;	/* ground + facade + roof + pillar + beam */
	int dynamic_removal_ran;
	double local_bound[6];	/* local_map->local_bound (min xyz, max xyz) */
	double bound[6];		/* local_map->bound: the same points moved by pose_lo */
	float ms_total;
} mulls_map_report;

void mulls_map_default_params(mulls_map_params *p);
int mulls_map_create(mulls_ctx *ctx, mulls_map **out);
/* a map belongs to its context: mulls_destroy(ctx) also destroys the maps still alive (their handles become invalid) */
void mulls_map_destroy(mulls_ctx *ctx, mulls_map *map);
/* (re)initialise the map from host clouds (e.g. the first frame's undown features) and its pose_lo (column-major) */
int mulls_map_set(mulls_ctx *ctx, mulls_map *map, const mulls_cloud clouds[6], const double pose_lo[16]);
/* update_local_map(local_map = map, last_target_cblock = {frame_down, frame_pose_lo}).  frame_down[0..4] = pc_*_down,
 * frame_down[5] = pc_vertex, all in the frame's own coordinates; they are not modified (the reference transforms and
 * filters last_target_cblock->pc_*_down in place: mulls_map_frame_download returns that state).  The call is mulls_map_update_batch (below) with one item,
 * without the batch's own refusals: a frame cloud may be a device cloud of any map or block of the context, this map's included.  Refused for a cloud with
 * points but no pointer or a stride below 48 (MULLS_E_INVALID), it has zeroed `report` and left the map untouched. */
int mulls_map_update(mulls_ctx *ctx, mulls_map *map, const mulls_cloud frame_down[6], const double frame_pose_lo[16],
					 const mulls_map_params *params, mulls_map_report *report);
/* Many maps, one update each, in lock step (map_batch.cpp): whoever drives several sequences side by side — a dataset's drives replayed together, several
 * vehicles, a parameter sweep over one drive — runs mulls_extract_features_batch and mulls_icp_batch for all streams and then this.
 *
 * What every item gets: the bytes of its own mulls_map_update call — every record of the six class clouds, the six frame clouds mulls_map_frame_download
 * returns, the pose, the status and every field of the report except ms_total (here: the wall time of the item's group) — whatever the batch size, the item's
 * position, the other items and the cuts into groups are.  Parameters are per item (params; NULL: shared_params); nothing assumes they are shared.
 *
 * Lock step: the items are cut into groups of max_lockstep (0: 64, which keeps the pinned staging of KITTI-sized frames near 20 MB).  Within a group every
 * device step of the update runs once for all items — one launch, or one fixed launch set, whose workgroups find their map, class and block in a table in
 * device memory, the grid being the sum of the items' work — and every host wait of an update happens at most once: behind the dynamic removal (only if
 * some item's removal runs), behind dist_filter, and behind the bounds and the pillar / beam refresh together.  The thinning masks of all maps are computed
 * on the host after the one read of dist_filter's counts and go up in one copy.  Each map keeps its own buffers; a buffer that has to grow is replaced at once
 * and the old one freed behind the phase's wait, so growth costs no wait.  stats->n_syncs and n_kernel_launches do not depend on the number of items in a group.
 *
 * Refused before anything is written (MULLS_E_INVALID; maps and results untouched): NULL items or results, a NULL or repeated map, a map of another context,
 * a frame_down cloud that lies in the memory of a map this batch updates, an item without params while shared_params is NULL.
 * Refused per item: a NULL frame_down, a used_feature_type / tree_used of fewer than 6 characters, a cloud with points but no pointer or a stride below 48 give
 * that item the status of its single call (results[i].status, report zeroed) and leave its map untouched to the byte; every other item is undisturbed.
 * Returns the status of the lowest-index item that is not MULLS_OK (mulls_last_error names it); n_items == 0: MULLS_OK.  After MULLS_E_HIP the maps of the
 * running group are unspecified until mulls_map_set, as after a failed mulls_map_update; the items of later groups are not run and report MULLS_E_HIP too.
 * results[i].path: 0 = lock step; 1 = handed to the single-map path inside the call — never taken: no input is known that the lock-step path cannot serve. */
typedef struct mulls_map_update_item
{
	mulls_map *map;
	const mulls_cloud *frame_down; /* [6], as mulls_map_update takes them: host or device clouds */
	double frame_pose_lo[16];	   /* column-major */
	const mulls_map_params *params; /* NULL: the call's shared params */
} mulls_map_update_item;
typedef struct mulls_map_batch_result
{
	int32_t status;
	uint32_t path;
	mulls_map_report report;
} mulls_map_batch_result;
typedef struct mulls_map_batch_stats
{
	uint32_t n_groups, n_lockstep, n_single_path, n_kernel_launches, n_syncs;
} mulls_map_batch_stats;
int mulls_map_update_batch(mulls_ctx *ctx, const mulls_map_update_item *items, uint32_t n_items, const mulls_map_params *shared_params,
						   uint32_t max_lockstep, mulls_map_batch_result *results, mulls_map_batch_stats *stats /* may be NULL */);
/* class cloud c of the map as a device cloud (48-B records); valid until the next mulls_map_set / _update / _destroy */
int mulls_map_cloud(mulls_ctx *ctx, const mulls_map *map, int cls, mulls_cloud *out);
int mulls_map_pose(mulls_ctx *ctx, const mulls_map *map, double pose_lo[16]);
/* copy class cloud c back to the host (48-B records); *n receives its size, at most cap records are written */
int mulls_map_download(mulls_ctx *ctx, const mulls_map *map, int cls, void *pts, uint32_t cap, uint32_t *n);
int mulls_map_frame_download(mulls_ctx *ctx, const mulls_map *map, int cls, void *pts, uint32_t cap, uint32_t *n);

/* ---- on-disk formats either side of the path; host code, no context needed ----
 * Readers follow the two-call pattern: *n receives the number of points, at most `cap` 48-byte records are written. */
/* DataIo::read_bin_file (dataio.hpp:357-378): KITTI x y z intensity float32 quadruples, intensity * 255; like the
 * reference the cloud ends with one extra all-zero point (its read loop tests the stream after pushing). */
int mulls_io_read_kitti_bin(const char *path, void *pts, uint32_t cap, uint32_t *n);
/* DataIo::read_pcd_file (dataio.hpp:279-287) = pcl::io::loadPCDFile<PointXYZINormal>: PCD v0.7, DATA ascii or binary,
 * float32 fields matched by name (x y z intensity normal_x normal_y normal_z curvature), others ignored / left 0. */
int mulls_io_read_pcd(const char *path, void *pts, uint32_t cap, uint32_t *n);
/* DataIo::write_pcd_file (dataio.hpp:288-312): WIDTH 1, HEIGHT n, eight float32 fields, binary or ascii */
int mulls_io_write_pcd(const char *path, const void *pts, uint32_t n, uint32_t stride, int as_binary);
/* DataIo::write_lo_pose_overwrite / _append (dataio.hpp:1896-1926): the top three rows of T (column-major), 8 significant digits */
int mulls_io_write_pose(const char *path, const double T[16], int append);

/* ---- feature extraction, first stage: CFilter::fast_ground_filter (include/common/cfilter.hpp:1658-2036),
 * the two-threshold grid ground filter that splits a (voxel-down-sampled) scan into ground and non-ground points ---- */

/* its positional parameters (cfilter.hpp:1663-1672; values of script/config/lo_gflag_list_kitti_urban.txt in brackets) */
typedef struct mulls_ground_params
{
	int32_t min_grid_pt_num;			   /* gf_grid_min_pt_num [6] */
	float grid_resolution;				   /* gf_grid_size [2.5] */
	float max_height_difference;		   /* gf_in_grid_h_thre [0.25] */
	float neighbor_height_diff;			   /* gf_neigh_grid_h_thre [1.5] */
	float max_ground_height;			   /* gf_max_h [2.0] */
	int32_t ground_random_down_rate;	   /* gf_ground_down_rate [12] */
	int32_t ground_random_down_down_rate;  /* gf_down_down_rate [3] */
	int32_t nonground_random_down_rate;	   /* gf_nonground_down_rate [3] */
	int32_t reliable_neighbor_grid_num_thre; /* gf_reliable_neighbor_grid_thre [0] */
	int32_t estimate_ground_normal_method; /* 0: (0,0,1).  1 / 2: pcl::NormalEstimationOMP over cloud_ground with every neighbour within normal_estimation_radius /
											  with the 2 * min_grid_pt_num nearest (pca.hpp:66-119), non-finite normals replaced by 0.577 (check_normal, :462-475).
											  3 [the shipped configs and extract_semantic_pts' default]: one PCL plane RANSAC per grid cell (cfilter.hpp:1909,
											  :2038-2056 -> cprocessing.hpp:67-106: SACSegmentation, 20 iterations, threshold 0.3 * max_height_difference, refit to the
											  inliers); the cell's ground points are the refined plane's inliers, every ground_random_down_rate-th of them kept with the
											  plane's normal if abs(normal_z) > 0.8.  PCL is not in this image: what it computes inside these calls is restated —
											  PCL's own deterministic sample sequence (boost::mt19937 seeded 12345, draw = output / 2, partial shuffles carried from
											  draw to draw), its float expressions, the neighbours of methods 1 / 2 ascending by (distance, index); the plane through
											  the inliers / neighbours is the smallest eigenvector of PCL's float covariance by Jacobi rotations in double instead of
											  pcl::eigen33's closed form (its largest component positive for method 3; turned towards the sensor for 1 / 2, as PCL
											  does) — "parity unpinned" for that part, everything MULLS wrote around the calls is pinned */
	int32_t distance_weight_downsampling_method; /* dist_inverse_sampling_method: 0 off, 1 linear, 2 quadratic [2].  Upstream the per-cell rates of 1 / 2
											  go through a variable shared by the threads of an OpenMP loop (cfilter.hpp:1829-1840: a data race); here
											  every cell uses its own value, i.e. the loop's sequential semantics */
	float standard_distance;			   /* [15.0] */
	uint8_t fixed_num_downsampling;		   /* ground_down by a fixed number instead of every down_down_rate-th point */
	uint8_t apply_grid_wise_outlier_filter; /* extract_semantic_pts passes apply_scanner_filter here (cfilter.hpp:2361) */
	uint8_t reserved_[2];
	int32_t down_ground_fixed_num;		   /* ground_down_fixed_num [800] */
	float intensity_thre;				   /* intensity_thre_nonground [150]; FLT_MAX disables */
	float outlier_std_scale;			   /* 3.0 */
	float normal_estimation_radius;		   /* [2.0] estimate_ground_normal_method 1 only (cfilter.hpp:1669) */
	uint32_t reserved2_;
	uint64_t rng_seed;					   /* ABI-only: fixed_num_downsampling thins with the seeded order-preserving selection of mulls_params.rng_seed
											  (upstream: pcl::RandomSample seeded with time(NULL)) */
} mulls_ground_params;

void mulls_ground_default_params(mulls_ground_params *p);

/* fast_ground_filter on `n` points (48-byte records, `stride` bytes apart).  Outputs (48-byte records, host memory, capacities in
 * points): ground = cloud_ground (normal (0,0,1)), ground_down = cloud_ground_down, unground = cloud_unground with data[3] (the
 * float at byte offset 12) = height above ground as the reference stores it.  n_out[3] = the three sizes; a cloud larger than its
 * capacity is truncated to it (its size is still reported).  The input is not modified (upstream writes normals and data[3] into
 * cloud_in: the copies handed out carry them).  One workgroup per scan; grids of more than 65536 cells or scans of more than 500000 points -> MULLS_E_UNSUPPORTED. */
int mulls_ground_filter(mulls_ctx *ctx, const void *pts, uint32_t n, uint32_t stride, const mulls_ground_params *params, void *ground, uint32_t cap_ground,
						void *ground_down, uint32_t cap_ground_down, void *unground, uint32_t cap_unground, uint32_t n_out[3]);

/* ---- feature extraction, second stage: CFilter::classify_nground_pts (include/common/cfilter.hpp:2058-2290) ---- */

/* its positional parameters (cfilter.hpp:2068-2082); defaults = what extract_semantic_pts (:2301-2318) passes when test/mulls_reg.cpp
 * calls it with script/run_mulls_reg.sh's flags */
typedef struct mulls_classify_params
{
	float neighbor_searching_radius; /* pca_neighbor_radius [1.0] */
	int32_t neighbor_k;				 /* pca_neighbor_count [50]; at most 64 */
	int32_t neigh_k_min;			 /* pca_neighbor_k_min [8] */
	int32_t pca_down_rate;			 /* [1]: every pca_down_rate-th point is a query, all are neighbours */
	float edge_thre, planar_thre;	 /* linearity_thre, planarity_thre [0.65, 0.65] */
	float edge_thre_down, planar_thre_down; /* [0.75, 0.75]; only read when sharpen_with_nms = 0 */
	int32_t extract_vertex_points_method;	/* [2]; 0 = no promotion of high-curvature points to pillar / beam */
	float curvature_thre;					/* [0.10] */
	float vertex_curvature_non_max_radius;	/* unused upstream too (1.5 * radius) */
	float linear_vertical_sin_high_thre, linear_vertical_sin_low_thre; /* [0.94, 0.17]: pillar above, beam below */
	float planar_vertical_sin_high_thre, planar_vertical_sin_low_thre; /* [0.98, 0.34]: roof above, facade below */
	uint8_t fixed_num_downsampling;			/* [0] */
	uint8_t sharpen_with_nms;				/* [1] */
	uint8_t use_distance_adaptive_pca;		/* [0] */
	uint8_t reserved_;
	int32_t pillar_down_fixed_num, facade_down_fixed_num, beam_down_fixed_num, roof_down_fixed_num, unground_down_fixed_num; /* [200, 800, 200, 200, 20000] */
	float beam_height_max, roof_height_min; /* [FLT_MAX, 0.0] */
	float feature_pts_ratio_guess;			/* [0.3] */
	uint64_t rng_seed;						/* ABI-only: the fixed-number down-samplings use the seeded order-preserving selection of mulls_params.rng_seed */
} mulls_classify_params;

void mulls_classify_default_params(mulls_classify_params *p);

enum mulls_classify_cloud
{
	MULLS_CL_PILLAR = 0,
	MULLS_CL_BEAM = 1,
	MULLS_CL_FACADE = 2,
	MULLS_CL_ROOF = 3,
	MULLS_CL_PILLAR_DOWN = 4,
	MULLS_CL_BEAM_DOWN = 5,
	MULLS_CL_FACADE_DOWN = 6,
	MULLS_CL_ROOF_DOWN = 7,
	MULLS_CL_VERTEX = 8, /* the key points this call appends to cloud_vertex */
	MULLS_CL_COUNT = 9
};

/* classify_nground_pts on the `n` non-ground points of a scan (48-byte records, `stride` bytes apart; normally mulls_ground_filter's
 * `unground`).  out[k] / cap[k] / n_out[k], k = enum mulls_classify_cloud: host buffers of 48-byte records, capacities in points, sizes; a
 * cloud larger than its capacity is truncated to it (its size is still reported); out[k] may be NULL with cap[k] = 0.
 * cloud_in_after (NULL, or room for n records) / n_cloud_in_after (NULL or a count): cloud_in as upstream leaves it — the function writes the
 * estimated normals into the cloud it is given, and thins it first when fixed_num_downsampling is on.  `pts` itself is not modified.
 * Neighbourhoods are exact (the neighbor_k nearest within the radius, by (distance, index)); what pcl::PCA / Eigen compute is restated (float
 * covariance in neighbour order, Jacobi in double; a direction's largest component is positive) — see DESIGN.md section 11 for what that means
 * for points within ~1e-6 of a threshold.  non_max_suppress's visiting order (and the order the class clouds are left in) is std::sort's by
 * normal[3] descending, ties included: the keys are sorted by the host's std::sort, the one order upstream's own build would produce. */
int mulls_classify_nground(mulls_ctx *ctx, const void *pts, uint32_t n, uint32_t stride, const mulls_classify_params *params, void *const out[MULLS_CL_COUNT],
						   const uint32_t cap[MULLS_CL_COUNT], uint32_t n_out[MULLS_CL_COUNT], void *cloud_in_after, uint32_t *n_cloud_in_after);

/* ---- feature extraction, the whole chain: CFilter::extract_semantic_pts (include/common/cfilter.hpp:2294-2413) ---- */

/* The per-frame front end of test/mulls_slam.cpp:359-365 / :404-421 in one call: dist_filter (:806-832, --apply_dist_filter) -> scanner filter
 * (:2338-2346, :914-929) -> voxel_downsample (:83-160, off below 0.001 m as in every shipped configuration: cloud_down_res 0) ->
 * fast_ground_filter -> classify_nground_pts.  The scan goes up once and the clouds stay on the device between the stages.  Not part of it: the
 * semantic-mask filters (semantic_assisted), the adaptive parameter update (host arithmetic on the cloud sizes, :2416-2444). */
typedef struct mulls_extract_params
{
	mulls_ground_params ground;
	mulls_classify_params classify;
	uint8_t apply_scanner_filter; /* extract_semantic_pts passes the same flag to fast_ground_filter as apply_grid_wise_outlier_filter: set ground.* yourself */
	uint8_t apply_dist_filter;	  /* keep min_dist_used^2 < x^2 + y^2 < max_dist_used^2 (float range, double limits), ahead of everything else */
	uint8_t reserved_[2];
	float self_ring_radius;			/* [1.75] */
	float ghost_radius;				/* [20.0] */
	float z_min;					/* -approx_scanner_height - 4.0: ghost points below it within ghost_radius go */
	float z_min_min;				/* -approx_scanner_height + underground_thre: everything below it goes */
	float vf_downsample_resolution; /* [0.0] voxel edge in metres; < 0.001: pc_down = pc_raw */
	double min_dist_used;			/* [1.0]  */
	double max_dist_used;			/* [120.0] */
} mulls_extract_params;

void mulls_extract_default_params(mulls_extract_params *p);

enum mulls_extract_cloud
{
	MULLS_EX_RAW = 0,		  /* pc_raw after the distance and scanner filters */
	MULLS_EX_GROUND = 1,	  /* pc_ground */
	MULLS_EX_GROUND_DOWN = 2, /* pc_ground_down */
	MULLS_EX_UNGROUND = 3,	  /* pc_unground as classify_nground_pts leaves it (written only if its capacity holds the whole cloud) */
	MULLS_EX_PILLAR = 4,	  /* ... followed by the nine clouds of enum mulls_classify_cloud in that order */
	MULLS_EX_VERTEX = 12,
	MULLS_EX_DOWN = 13, /* pc_down: pc_raw after voxel_downsample (the same cloud when that is off; ask for it with a capacity only when it is on) */
	MULLS_EX_COUNT = 14
};

/* out[k] / cap[k] / n_out[k], k = enum mulls_extract_cloud: host buffers of 48-byte records, capacities in points, sizes (a cloud larger than its
 * capacity is truncated, its size still reported; out[k] may be NULL with cap[k] = 0).  Results are those of mulls_ground_filter followed by
 * mulls_classify_nground on its `unground`. */
int mulls_extract_features(mulls_ctx *ctx, const void *scan, uint32_t n, uint32_t stride, const mulls_extract_params *params, void *const out[MULLS_EX_COUNT],
						   const uint32_t cap[MULLS_EX_COUNT], uint32_t n_out[MULLS_EX_COUNT]);

/* ---- device-resident feature block: the cloudblock_t of one scan kept in HBM ----
 * The per-frame loop of test/mulls_slam.cpp (:359-442, :642-693) hands one cloudblock_t from extract_semantic_pts to mm_lls_icp to update_local_map.
 * mulls_extract_features_resident is mulls_extract_features with the feature clouds left on the device: mulls_block_cloud() yields device clouds
 * (48-byte records) that mulls_pair.src[] / tgt[] and mulls_map_update's frame_down[] accept the way they accept mulls_map_cloud() — raw scan in, pose
 * out, nothing but the scan, a few selection indices and the 4x4 crossing PCIe (the *_down clouds the fixed-number samplers thin on the host — a few
 * thousand points — make one round trip when fixed_num_downsampling is on).  A block holds the clouds of enum mulls_extract_cloud except MULLS_EX_RAW and
 * MULLS_EX_DOWN; they are valid until the block is extracted into again or destroyed (mulls_destroy destroys the blocks still alive). */
typedef struct mulls_block mulls_block;
int mulls_block_create(mulls_ctx *ctx, mulls_block **out);
void mulls_block_destroy(mulls_ctx *ctx, mulls_block *block);
int mulls_extract_features_resident(mulls_ctx *ctx, const void *scan, uint32_t n, uint32_t stride, const mulls_extract_params *params, mulls_block *block,
									uint32_t n_out[MULLS_EX_COUNT]);
int mulls_block_cloud(mulls_ctx *ctx, const mulls_block *block, int which, mulls_cloud *out);
/* copy cloud `which` back to the host (48-byte records); *n receives its size, at most cap records are written */
int mulls_block_download(mulls_ctx *ctx, const mulls_block *block, int which, void *pts, uint32_t cap, uint32_t *n);

/* ---- many scans per call: mulls_extract_features_resident in lock step ----
 * mulls_extract_features_batch runs extract_semantic_pts' chain (dist_filter -> scanner_filter -> voxel_downsample -> fast_ground_filter -> classify_nground_pts)
 * on n_scans scans with one `params` (rng_seed included: every scan's fixed-number selections are its single call's) and leaves the feature clouds of scan i
 * in blocks[i].  Every scan gets the bytes of its own mulls_extract_features_resident call — the fourteen n_out counts, every record of the twelve clouds a
 * block holds, the return code — whatever the batch size, the scan's position, the other scans and the cuts into sub-batches are.
 *   scans[i]   48-byte records `stride` bytes apart in host memory or in a device cloud of this context (detected as the single call detects it)
 *   blocks[i]  live blocks of this context, all different, overwritten; a null or repeated block: MULLS_E_INVALID before anything is written
 *   scratch_limit_bytes  bound of one sub-batch's device arena (0: MULLS_EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES, which holds 64 scans of 121 k returns under the
 *              KITTI parameters); consecutive scans share a sub-batch while they fit, a scan larger than the limit runs alone
 *   results[i] status: what the scan's single call returns (a refused scan — a grid of more than 65 536 cells, non-finite coordinates reaching the
 *              classification, more than 500 000 points — leaves its block with all sizes zero and disturbs no other scan); path; n_out
 *   stats      optional (may be NULL)
 * Within a sub-batch every device step runs once for all scans (one launch whose workgroups find their scan in a table in device memory) and every host
 * wait of a scan's chain happens once; both fixed-point loops run in lock step until no scan has an undecided point.  Two steps have no lock-step form and
 * run scan-locally: voxel_downsample (vf_downsample_resolution >= 0.001: a host sort per scan either way) and the ground normals of
 * estimate_ground_normal_method 1 / 2 (their own neighbour grid and error word).  With either, and with parameters every scan is refused for, each scan is
 * a sub-batch of its own, whatever the limit: the same code and the same bits, one scan at a time (path = 1; these scans count in n_single_path and in
 * nothing else of the statistics).  Everything else runs in lock step (path = 0).  The single calls (mulls_extract_features, _resident, mulls_ground_filter,
 * mulls_classify_nground) are this chain, or one stage of it, on a batch of one.
 * Returns the status of the lowest-index scan whose status is not MULLS_OK (mulls_last_error names it), else MULLS_OK; n_scans == 0: MULLS_OK. */
typedef struct mulls_extract_batch_result
{
	int32_t status;					/* this scan's code: what its single call returns */
	uint32_t path;					/* 0 = ran in lock step, 1 = ran alone, with the two scan-local steps */
	uint32_t n_out[MULLS_EX_COUNT];
} mulls_extract_batch_result;
typedef struct mulls_extract_batch_stats
{
	uint32_t n_subbatches, n_lockstep, n_single_path;
	uint32_t n_kernel_launches, n_syncs; /* of the lock-step part: kernels enqueued, host waits on the stream */
	uint32_t promote_rounds, nms_rounds; /* rounds launched, summed over sub-batches */
} mulls_extract_batch_stats;
#define MULLS_EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES (12ull << 30)
int mulls_extract_features_batch(mulls_ctx *ctx, const mulls_cloud *scans, uint32_t n_scans, const mulls_extract_params *params, mulls_block *const *blocks,
								 uint64_t scratch_limit_bytes, mulls_extract_batch_result *results, mulls_extract_batch_stats *stats);

/* ---- motion compensation of a frame after its registration (test/mulls_slam.cpp:703-712, on in the 32- and 128-beam configurations) ----
 * mulls_motion_compensate = CFilter::apply_motion_compensation(pc_in_out, Tran, s_ambigous_thre) (cfilter.hpp:470-491), in place on `n` 48-byte records: every
 * point whose time stamp t (the curvature field, pts time-stamp ratio in the frame) lies in [thre, 1 - thre] is moved by the fraction t of Tran — slerp of the
 * rotation from the identity, t times the translation, double arithmetic, float store; directions are left as they are.  Tran: 4 x 4, column-major.
 * pts: host memory (one upload, one download) or a device-resident cloud (mulls_block_cloud, mulls_map_cloud: in place, nothing crosses PCIe).
 * mulls_block_motion_compensate = the two batch_apply_motion_compensation calls of mulls_slam.cpp:706-710 on a device-resident feature block: its ground /
 * pillar / facade / beam / roof clouds and their *_down clouds (the vertex cloud only with undistort_keypoints, which no caller of the reference sets). */
int mulls_motion_compensate(mulls_ctx *ctx, void *pts, uint32_t n, uint32_t stride, const double Tran[16], float s_ambiguous_thre);
int mulls_block_motion_compensate(mulls_ctx *ctx, mulls_block *block, const double Tran[16], int undistort_keypoints);

/* CFilter::voxel_downsample (cfilter.hpp:83-160): one point per occupied voxel of edge voxel_size, voxels in increasing index
 * ((vx * ny + vy) * nz + vz from the cloud's minimum corner), the point of a voxel being the one std::sort leaves first among that voxel's
 * (voxel, index) pairs, exactly as upstream (bounding box and voxel indices on the device, that one sort on the host).  voxel_size < 0.001
 * copies the cloud.  MULLS_E_INVALID for a non-finite coordinate, MULLS_E_UNSUPPORTED beyond 2^21 voxels along an axis or 500000 points.
 * out: host buffer of cap 48-byte records; *n_out = size of pc_down (truncated to cap when larger). */
int mulls_voxel_downsample(mulls_ctx *ctx, const void *pts, uint32_t n, uint32_t stride, float voxel_size, void *out, uint32_t cap, uint32_t *n_out);

/* ---- key-point descriptor matching: CRegistration<PointT>::find_feature_correspondence_ncc (include/common/cregistration.hpp:409-601) ----
 * The correspondence stage of the reference's global (coarse) registration (test/mulls_reg.cpp:170-179, test/mulls_slam.cpp:532-540): the key points of two
 * scans (pc_vertex, MULLS_EX_VERTEX) are matched by the L1 distance of their 11-entry "neighbourhood category context" descriptors — the two packed codes
 * encode_stable_points left in normal[0] / normal[1], the intensity normalised by the TARGET's range, normal[3] (curvature) and data[3] (height above
 * ground).  mulls_coarse_reg_ransac(_indexed) and mulls_coarse_reg_teaser(_indexed) below are the solvers that consume the pairs.
 *   not fixed_num_corr: every target key point i with the first source key point j* at the strictly smallest distance (a row without any distance below
 *     FLT_MAX yields j* = 0), in ascending i; with reciprocal_on only while no other target is strictly closer to j*.
 *   fixed_num_corr: the corr_num smallest of the Nt * Ns distances in ascending order, a pair being skipped once its target or its source point has been
 *     used seven times (`count > 6`, :578).  Upstream orders them with a std::sort that looks at the distance only and is not stable: the order among exactly
 *     equal distances is whatever that sort leaves.  THIS LIBRARY DEFINES IT as ascending flat index i * Ns + j (a stable sort of the table).  NaN distances are
 *     never selected.  MULLS_E_UNSUPPORTED: Nt * Ns > INT32_MAX in this mode (upstream's int index overflows), corr_num > 65536.  corr_num <= 0: no pairs.
 * The Nt x Ns table is never stored: the nearest-neighbour modes take 65536 x 65536 key points and more. */
typedef struct mulls_ncc_params
{
	int32_t fixed_num_corr; /* [0] cregistration.hpp:411 */
	int32_t corr_num;		/* [2000] */
	int32_t reciprocal_on;	/* [1]; ignored when fixed_num_corr, as upstream */
	int32_t reserved;
} mulls_ncc_params;
void mulls_ncc_default_params(mulls_ncc_params *p);
/* returns 1: the reference's `true` (n_corr pairs, possibly 0); 0: its `false` (fewer than 10 key points on a side, *n_corr = 0); < 0: MULLS_E_*.
 * tgt_idx[k] / src_idx[k]: indices into the two clouds, in the reference's push_back order.  *n_corr is the full count; at most cap pairs are written.
 * The clouds are host memory (any stride that is a multiple of 4 and at least 36; the 20 bytes per key point the descriptor reads go up) or device-resident
 * clouds of 48-byte records (mulls_block_cloud(..., MULLS_EX_VERTEX, ...), mulls_map_cloud). */
int mulls_ncc_correspond(mulls_ctx *ctx, const mulls_cloud *tgt_kpts, const mulls_cloud *src_kpts, const mulls_ncc_params *params, int32_t *tgt_idx,
						 int32_t *src_idx, uint32_t cap, uint32_t *n_corr);

/* ---- many key-point matching problems per call: the candidate edges of one loop-closure event (test/mulls_slam.cpp:517-596 matches them one after
 * another), or one scan against a list of submaps; the stage in front of mulls_coarse_reg_teaser_batch, whose index lists are the ones written here.
 * results[b] and the pairs written to problems[b].tgt_idx / src_idx are THE BITS mulls_ncc_correspond RETURNS for problem b with the same params: the return
 * value (ret: 1 for the reference's `true`, 0 for its `false`), the full n_corr, the pairs in the reference's push_back order, at most cap of them written.
 * No arithmetic or order is redefined; the fixed-number tie rule stays ascending flat index i * Ns + j.
 * Every device step runs once per sub-batch for all its problems: a table pass is one launch whose workgroups each belong to one
 * problem, the fixed-number selection's six digit levels run in lock-step (one histogram and one pick launch per level; a problem whose selection is settled
 * is skipped on the device), the sub-batch has one upload and one download.  The ordering of the at most 65536 keys and upstream's seven-per-point walk
 * run on the host per problem, as in the single call.
 *   per problem   fewer than 10 key points on a side: ret 0, n_corr 0 (cregistration.hpp:421-425); fixed_num_corr with corr_num <= 0: ret 1, no pairs.
 *                 The rest of the batch runs.
 *   whole call    checked for every problem before any device work: a problem the single call would refuse (a bad stride, a NULL it needs,
 *                 n > INT32_MAX, fixed_num_corr with Nt * Ns > INT32_MAX or corr_num > 65536) and a NULL params make the call return the single call's
 *                 code, name the first such problem's index in mulls_last_error, and leave every result at ret 0 / n_corr 0.
 *   shared clouds the same cloud may appear in several problems; a host cloud is staged once per distinct (pts, n, stride) of a sub-batch.  No result
 *                 depends on it.
 *   scratch_limit_bytes  bounds the call's device arena (per problem: 20 bytes per staged key point, 56 per key point of descriptors and keys, the
 *                 output — 8 Nt bytes, or 8 (K + 1) in fixed-number mode — and in that mode 49 KB of selection state).  The batch is cut into consecutive
 *                 sub-batches that fit; a problem larger than the limit runs alone.  0: MULLS_NCC_BATCH_DEFAULT_SCRATCH_BYTES, a value chosen without a
 *                 measurement.  The arena belongs to the context, grows only, and is released with it.
 * n_problems = 0: MULLS_OK. */
#define MULLS_NCC_BATCH_DEFAULT_SCRATCH_BYTES (512ull << 20)
typedef struct mulls_ncc_problem
{
	mulls_cloud tgt, src;		/* host or device-resident key-point clouds, by the single call's rules (strides included) */
	int32_t *tgt_idx, *src_idx; /* cap entries each, or NULL with cap = 0 */
	uint32_t cap;
	uint32_t reserved;
} mulls_ncc_problem;

typedef struct mulls_ncc_result
{
	int32_t ret;	 /* mulls_ncc_correspond's return value for this problem: 1 or 0 */
	uint32_t n_corr; /* the full count; min(n_corr, cap) pairs were written */
} mulls_ncc_result;

int mulls_ncc_correspond_batch(mulls_ctx *ctx, const mulls_ncc_problem *problems, uint32_t n_problems, const mulls_ncc_params *params,
							   uint64_t scratch_limit_bytes, mulls_ncc_result *results);

/* ---- RANSAC coarse registration: CRegistration<PointT>::coarse_reg_ransac (include/common/cregistration.hpp:605-661) ----
 * The solver that turns mulls_ncc_correspond's pairs into the initial guess of mulls_icp.  Upstream's body is one call of PCL's
 * CorrespondenceRejectorSampleConsensus (RANSAC over SampleConsensusModelRegistration, then refineModel).  PCL is not available where this library is
 * built and tested, so nothing below was checked against it: the lines marked [PCL] restate PCL 1.8 - 1.10 from memory
 * (correspondence_rejection_sample_consensus.hpp, ransac.hpp, sac_model.h, sac_model_registration.h, sac.h), the lines marked [LIB] are defined by this
 * library where PCL's result depends on Eigen's decompositions, which cannot be pinned.  tests/ransac_restated.py restates all of it independently in
 * numpy, bit for bit.  DESIGN.md section 7 has the same list with its reasons.  Correspondence i pairs point i of each cloud (:621-627).
 *   draws      [PCL] std::mt19937(12345), rnd() = eng() >> 1; a sample is three steps of a Fisher-Yates shuffle, swap(shuffled[i], shuffled[i + rnd() % (N - i)]),
 *              i = 0, 1, 2, on an index array that is carried from draw to draw; up to 1000 draws until isSampleGood; none found: the loop ends.
 *   sample     [PCL] good when the three pairwise squared distances between the SOURCE sample points exceed sample_dist_thresh.  The distance runs over the
 *              point's four-float map: x, y, z and data[3], which key points use for their height above ground — a quirk, kept.  It is summed as Eigen's
 *              packet reduction does, (dx*dx + dz*dz) + (dy*dy + dw*dw), in float.  sample_dist_thresh = (mean of the square roots of the three
 *              eigenvalues of the source cloud's covariance)^2, in double; the covariance is pcl::computeMeanAndCovarianceMatrix's (float raw moments
 *              summed in index order, divided by N, E[xx^T] - c c^T).   [LIB] the eigenvalues: cyclic Jacobi in double on that float covariance.
 *   model      [LIB] the rigid transform of the sample pairs (PCL: float demeaning, H, JacobiSVD<Matrix3f>).  Float centroids ((p0 + p1) + p2) / 3, float
 *              H[a][b] = sum of (s_k[a] - cs[a]) * (t_k[b] - ct[b]) in the samples' order; then in double Horn's symmetric 4 x 4 matrix of H, exactly
 *              10 sweeps of cyclic Jacobi over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), the column of the largest diagonal entry (the first among equals)
 *              normalised to a unit quaternion, its rotation matrix R, t = ct - R cs; all of it rounded to float once.  Only + - * / sqrt, no
 *              contraction.  DESIGN.md section 7 lists it operation by operation.
 *   score      count = #{ i : |T (s_i, 1) - (t_i, 1)|^2 < (double)noise_bound^2 }, float: p_r = ((T_r0 sx + T_r1 sy) + T_r2 sz) + T_r3, d_r = p_r - t_r,
 *              d2 = (dx dx + dy dy) + dz dz, compared as (double)d2 < threshold.
 *   loop       [PCL] iteration i = 0, 1, ...: a count above the best so far installs the model and k = log(1 - 0.99) / log(clamp(1 - (best / N)^3, eps, 1 - eps))
 *              (std::log, std::pow); the loop goes on while iterations < k, and ends once ++iterations > max_iter_num.  The device scores every hypothesis
 *              the loop could reach in one launch and the host applies this rule to the counts: the same result, as the samples do not depend on the counts.
 *   refinement [PCL] refineModel(3.0, 1000): fit all current inliers, select within error_threshold, variance = 2.1981 * the selected squared distances'
 *              element of rank size/2, error_threshold = sqrt(min(noise_bound^2, 9 variance)); repeated while the inlier set changes; a 2-cycle in the
 *              last four set sizes ends it and KEEPS THE UNREFINED model and inliers (PCL returns true there without installing anything); 1000 rounds
 *              or an empty selection: failure.   [LIB] the fit is the model estimator with double sums: centroids, then H of the demeaned doubles; each
 *              sum in the fixed order "256 strided partial sums in ascending index, then a pairwise tree" (DESIGN.md section 7).
 *   outcomes   [PCL] no model (N < 3, no good sample) or fewer than 3 inliers: every correspondence passes with T = identity, so status follows N; a failed
 *              refinement: no inliers, status -1; else status = 1 if n_inliers >= 2 min_inlier_num, 0 if >= min_inlier_num, -1 below.
 * Non-finite coordinates follow the arithmetic above (a NaN covariance means no sample is good: the pass-through outcome). */
typedef struct mulls_ransac_params
{
	float noise_bound;		/* [0.2]   inlier threshold, metres (setInlierThreshold) */
	int32_t min_inlier_num; /* [8]     */
	int32_t max_iter_num;	/* [20000] */
	int32_t refine;			/* [1]     upstream: setRefineModel(true) */
} mulls_ransac_params;

typedef struct mulls_ransac_result
{
	int32_t status;			   /* upstream's return: 1 reliable, 0 need check, -1 failed */
	int32_t iterations;		   /* hypotheses the sequential definition evaluated */
	int32_t best_iteration;	   /* index of the winning hypothesis, -1 if none */
	int32_t refine_iterations; /* rounds of the refinement that fitted a model */
	uint32_t n_inliers;		   /* size of final_corres */
	double T[16];			   /* column-major; upstream's Matrix4f cast to double; identity when status == -1 */
} mulls_ransac_result;

void mulls_ransac_default_params(mulls_ransac_params *p);
/* returns MULLS_OK or MULLS_E_*: MULLS_E_INVALID when the sizes differ (upstream reads out of bounds then), for a non-finite noise_bound or a bad stride;
 * MULLS_E_UNSUPPORTED above 65536 points or max_iter_num > 2^20.  inliers: the indices of final_corres, ascending, at most cap of them (NULL / 0 allowed).
 * The clouds are host memory (any stride that is a multiple of 4 and at least 16: x, y, z, data[3] go up) or device-resident clouds of 48-byte records. */
int mulls_coarse_reg_ransac(mulls_ctx *ctx, const mulls_cloud *tgt_pts, const mulls_cloud *src_pts, const mulls_ransac_params *params,
							mulls_ransac_result *result, int32_t *inliers, uint32_t cap);
/* the same solver on tgt_kpts[tgt_idx[k]] <-> src_kpts[src_idx[k]], k < n_corr: the index lists mulls_ncc_correspond wrote (host memory).  The gather
 * runs on the device; results equal mulls_coarse_reg_ransac on the gathered clouds (inliers are positions k in the lists).  MULLS_E_INVALID for an
 * index outside its cloud. */
int mulls_coarse_reg_ransac_indexed(mulls_ctx *ctx, const mulls_cloud *tgt_kpts, const mulls_cloud *src_kpts, const int32_t *tgt_idx, const int32_t *src_idx,
									uint32_t n_corr, const mulls_ransac_params *params, mulls_ransac_result *result, int32_t *inliers, uint32_t cap);

/* ---- many RANSAC problems per call: the candidate edges of one loop-closure event under --teaser_based_global_registration_on=false
 * (test/mulls_slam.cpp:517-596 tries them one after another), behind mulls_ncc_correspond_batch and in front of mulls_icp_batch.
 * results[b] and problems[b].inliers[] are THE BYTES THE MATCHING SINGLE CALL RETURNS for problem b on the same context (mulls_coarse_reg_ransac when both
 * index lists are NULL, mulls_coarse_reg_ransac_indexed when both are set): every field of the result, every bit of T, the inlier list, the slot behind
 * inlier_cap left alone.  No arithmetic is redefined; every order of summation holds per problem (the float models, the 256 strided partial sums and
 * pairwise tree of the refinement fit, the radix-select median).  The device steps run for all problems of a sub-batch per launch: one launch for all
 * models, one for all counts, one for all winners' masks, and the refinement in lock step, one launch per round with one workgroup per problem that still
 * refines; a problem that has ended is not launched again, so its masks and model are frozen (addendum).  The draws run per
 * problem on the host, the problems side by side.
 *   per problem   PCL's pass-through outcomes (fewer than 3 pairs, no good first sample, fewer than 3 inliers) give the single call's result; the rest of
 *                 the batch runs.
 *   whole call    checked for every problem before any device work and before any result is written: a problem the single call would refuse (a bad
 *                 stride, sizes that differ, an index outside its cloud, more than 65536 pairs, one index list without the other, a NULL it needs),
 *                 max_iter_num > 2^20 and a non-finite noise_bound make the call return the single call's code, name the first such problem's index in
 *                 mulls_last_error (a refused parameter refuses problem 0), and leave every result at status -1, best_iteration -1, identity T.
 *   scratch_limit_bytes  bounds the device arena: per problem the two packed float4 pair arrays, the index lists, max_iter_num + 1 triples, models and
 *                 counts, three masks, the squared distances and one round record.  The batch is cut into consecutive sub-batches that fit; a problem
 *                 larger than the limit runs alone.  0: MULLS_RANSAC_BATCH_DEFAULT_SCRATCH_BYTES, a value chosen without a measurement.
 * n_problems = 0: MULLS_OK. */
#define MULLS_RANSAC_BATCH_DEFAULT_SCRATCH_BYTES (512ull << 20)
typedef struct mulls_ransac_problem
{
	mulls_cloud tgt, src;			  /* host or device-resident clouds, by the single call's rules (strides included) */
	const int32_t *tgt_idx, *src_idx; /* both NULL: pair i = point i of each cloud; both set: the n_corr pairs they name */
	uint32_t n_corr;				  /* read only when the index lists are set */
	uint32_t inlier_cap;
	int32_t *inliers;				  /* inlier_cap entries, or NULL with inlier_cap = 0 */
} mulls_ransac_problem;

int mulls_coarse_reg_ransac_batch(mulls_ctx *ctx, const mulls_ransac_problem *problems, uint32_t n_problems, const mulls_ransac_params *params,
								  uint64_t scratch_limit_bytes, mulls_ransac_result *results);

/* ---- TEASER coarse registration: CRegistration<PointT>::coarse_reg_teaser (include/common/cregistration.hpp:664-759) ----
 * The solver every shipped configuration selects (--teaser_based_global_registration_on=true) between mulls_ncc_correspond's pairs and mulls_icp's initial
 * guess.  Upstream's body is one call of TEASER++'s RobustRegistrationSolver (no scale estimation, maximum clique, GNC-TLS rotation).  TEASER++ is not
 * available where this library is built and tested, so nothing below was checked against it: the lines marked [TEASER] restate TEASER++ as of the
 * reference's date from memory (registration.cc, graph.cc), the lines marked [LIB] are this library's own arithmetic where TEASER++'s result rests on PMC's
 * thread timing or on Eigen's decompositions, which cannot be pinned.  tests/teaser_restated.py restates all of it independently in numpy, bit for bit.
 * DESIGN.md section 7.4 has the same list with its reasons.  Correspondence i pairs point i of each cloud (s_i: source, t_i: target).  All arithmetic is
 * double on coordinates widened from float, only + - * / sqrt, no contraction, every sum in the stated order.
 *   outcomes   [upstream] unequal sizes or N <= 3: MULLS_OK with status -1 (upstream returns -1 there).  [LIB] N > 8192: MULLS_E_UNSUPPORTED.
 *   graph      [TEASER] vertices: the N pairs; edge {i, j} iff | |s_j - s_i| - |t_j - t_i| | <= beta, beta = 2 (double)noise_bound sqrt(cbar2), cbar2 = 1
 *              (:703), |d| = sqrt((dx dx + dy dy) + dz dz).  A NaN comparison gives no edge.  n_edges counts them; max_core is the largest core number.
 *   clique     [LIB] TEASER++ takes *a* maximum clique from PMC, which one depends on thread timing.  This library takes THE LEXICOGRAPHICALLY SMALLEST
 *              MAXIMUM CLIQUE (ascending index lists compared), which no search order can change.  The search is exact up to clique_node_budget visited
 *              nodes; beyond, the largest clique found so far by a deterministic single-threaded search is used and clique_exact = 0 (that clique does
 *              depend on the search: teaser_host.h).  kcore_heuristic_threshold (:710) is not used: upstream leaves the mode at exact.  A graph without
 *              an edge has the clique {0}; clique_size <= 1: status -1.  clique_nodes is the search's effort, not part of the definition.
 *              With MULLS_OPT_TEASER_DEVICE_SEARCH = 1 the same clique comes from a search on the device (mulls_amd/csrc/teaser_search.h): clique
 *              prefixes (a vertex, or a vertex and one later neighbour) are tasks in lexicographic rank order, one wavefront each; a first phase finds
 *              the size (a shared incumbent, raised atomically), a second the list (every task looks for its first clique of that size in ascending
 *              order; the task of the lowest rank that has one holds the smallest list).  Whenever the search completes, every field is the same bits
 *              as the host search's, except: clique_nodes is the number of tree nodes all workers entered (every task that is started counts as one at
 *              least); pruning depends on when a worker sees another's bound, so the number NEED NOT REPEAT from call to call.  clique_node_budget
 *              bounds that total; the host checks it between launches, so the overshoot is at most one launch's quota (2048 workers x 256 nodes).
 *              When the total exceeds the budget, clique_exact = 0 and the clique is THE GREEDY BOUND'S WITNESS (the clique grown from the first vertex
 *              of the largest greedy clique by taking the smallest common neighbour again and again), not the largest clique found so far: an
 *              abandoned search's result does not depend on scheduling either.  Whether a search whose effort lies within one launch of the budget is
 *              abandoned at all may depend on timing, since the effort does.  search_seconds is then the wall time of the device search, from its first
 *              launch to its last readback.
 *   measures   [TEASER] clique vertices c_0 < ... < c_(C-1); measurement k runs over the pairs a < b, a outer, b inner: a_k = s_cb - s_ca,
 *              b_k = t_cb - t_ca; M = C (C - 1) / 2.
 *   rotation   [TEASER] GNC-TLS: at most 100 iterations, factor 1.4, cost threshold 0.005 (:705-711); nb2 = noise_bound^2, 1e-2 when below 1e-16; weights 1,
 *              prev_cost = +inf.  Iteration i: (1) R = fit of the weighted measurements; (2) r_k = |b_k - R a_k|^2, each row (R0 ax + R1 ay) + R2 az,
 *              (dx dx + dy dy) + dz dz; (3) i = 0 only: mu = 1 / ((2 max r) / nb2 - 1), the loop ends if mu <= 0 (cost stays 0, the weights 1);
 *              (4) cost = sum of w_k r_k with the weights before the update; (5) w_k = 0 if r_k >= ((mu + 1) / mu) nb2, 1 if r_k <= (mu / (mu + 1)) nb2,
 *              else sqrt(((nb2 mu) (mu + 1)) / r_k) - mu; (6) the loop ends if |cost - prev_cost| < 0.005, else mu = 1.4 mu, prev_cost = cost.
 *              gnc_iterations = fits made.  Rotation inliers: w_k >= 0.5.
 *              [LIB] the fit: H[p][q] = sum of (w_k a_k[p]) b_k[q]; Horn's symmetric 4 x 4 of H, exactly 10 sweeps of cyclic Jacobi, the column of the
 *              largest diagonal entry (the first among equals) as a unit quaternion, its rotation matrix — mulls_coarse_reg_ransac's steps, kept in double.
 *              [LIB] H's nine sums and the cost: 4096 strided partial sums (partial p adds k = p, p + 4096, ... in ascending order, from 0), then the
 *              pairwise tree p[t] += p[t + s], s = 2048, ..., 1.
 *   translation [TEASER] per axis x_c = t_c - ((R0 sx + R1 sy) + R2 sz) over the C clique points and TEASER's scalar TLS estimator with range noise_bound:
 *              the 2C endpoints x - range (opening), x + range (closing) sorted by (value, opening before closing, index); swept in that order with the
 *              running sums sw, swx, swx2 (w = 1 / range^2; + w, + w x, + (w x) x when opening, - when closing) and the excluded ranges' sum (C times
 *              range added up, - range when opening, + when closing); candidate xhat = swx / sw, cost ((sw xhat) xhat + swx2 - (2 swx) xhat) + excluded;
 *              the first strictly smallest cost wins, a NaN never, none: 0.  Translation inliers: |x_c - that| <= range on all three axes.  Serial and at
 *              most 8192 values: it runs on the host on one download of R and the clique's points.
 *   outcome    [upstream] n = the number of rotation inliers — MEASUREMENTS, not pairs, as TEASER++'s getRotationInliers() of that date returns them: a
 *              clique of 5 reaches min_inlier_num = 8.  A quirk, kept.  status 1 if n >= 2 min_inlier_num, 0 if n >= min_inlier_num, else -1. */
#define MULLS_TEASER_DEFAULT_NODE_BUDGET (1ull << 28)
typedef struct mulls_teaser_params
{
	float noise_bound;			 /* [0.2]  metres (cregistration.hpp:666) */
	int32_t min_inlier_num;		 /* [8]    */
	uint64_t clique_node_budget; /* [MULLS_TEASER_DEFAULT_NODE_BUDGET] nodes the exact clique search may visit */
} mulls_teaser_params;

typedef struct mulls_teaser_result
{
	int32_t status;		   /* upstream's return: 1 reliable, 0 need check, -1 failed */
	int32_t max_core;	   /* largest core number of the graph */
	uint64_t n_edges;
	int32_t clique_size;
	int32_t clique_exact;  /* 1: the search finished within the budget */
	uint64_t clique_nodes; /* nodes the search visited (device search: by all workers together; need not repeat) */
	int32_t gnc_iterations;
	int32_t n_rotation_inliers; /* measurements with weight >= 0.5: upstream's inlier count */
	int32_t n_translation_inliers;
	int32_t reserved;
	double cost;		   /* the last GNC iteration's */
	double search_seconds; /* wall time of the clique search, host or device: a measurement, not a result */
	double T[16];		   /* column-major; written when status >= 0, the identity otherwise */
} mulls_teaser_result;

void mulls_teaser_default_params(mulls_teaser_params *p);
/* returns MULLS_OK or MULLS_E_*: MULLS_E_INVALID for a non-finite or negative noise_bound or a bad stride (mulls_coarse_reg_ransac's rule);
 * MULLS_E_UNSUPPORTED above 8192 pairs.  clique: the clique's pair indices, ascending, at most cap of them (NULL / 0 allowed).  The clouds are host memory
 * (any stride that is a multiple of 4 and at least 16) or device-resident clouds of 48-byte records.
 * The NULL checks of ctx, the clouds, params, result and clique (MULLS_E_INVALID, result untouched) come first, then a cloud with points and no address
 * (MULLS_E_INVALID), noise_bound, and the refusals of the one checker mulls_coarse_reg_teaser_batch (below) uses per problem, with this entry point's name
 * and no problem index in mulls_last_error.  The device steps are the text the batch compiles (k_teaser.hip), launched with arguments instead of a descriptor. */
int mulls_coarse_reg_teaser(mulls_ctx *ctx, const mulls_cloud *tgt_pts, const mulls_cloud *src_pts, const mulls_teaser_params *params,
							mulls_teaser_result *result, int32_t *clique, uint32_t cap);
/* the same solver on tgt_kpts[tgt_idx[k]] <-> src_kpts[src_idx[k]], k < n_corr, gathered on the device as mulls_coarse_reg_ransac_indexed does (clique
 * entries are positions k in the lists).  MULLS_E_INVALID for an index outside its cloud, and for n_corr > 0 with a list that is NULL; n_corr = 0 reads no
 * list and is upstream's "too few correspondences" (MULLS_OK, status -1): the call says that the problem is indexed, where the batch infers it from the
 * lists. */
int mulls_coarse_reg_teaser_indexed(mulls_ctx *ctx, const mulls_cloud *tgt_kpts, const mulls_cloud *src_kpts, const int32_t *tgt_idx, const int32_t *src_idx,
									uint32_t n_corr, const mulls_teaser_params *params, mulls_teaser_result *result, int32_t *clique, uint32_t cap);

/* ---- many TEASER problems per call: the candidate edges of one loop-closure event (test/mulls_slam.cpp:517-596 tries them one after another), or one
 * scan against a list of submaps.  Until the first success the problems are independent: solve them all, then apply the sequential rule to the results.
 * results[b] and problems[b].clique[] are THE BITS THE MATCHING SINGLE CALL RETURNS for problem b on the same context options (mulls_coarse_reg_teaser when
 * both index lists are NULL, mulls_coarse_reg_teaser_indexed when both are set): status, max_core, n_edges, clique_size, clique_exact, gnc_iterations, both
 * inlier counts, the clique list, every bit of cost and T.  No arithmetic is redefined; the summation orders hold per problem.  search_seconds is a
 * measurement; clique_nodes equals the single call's when the host search runs and need not repeat under MULLS_OPT_TEASER_DEVICE_SEARCH, as above.
 * The device steps run for all problems of a sub-batch per launch, and the GNC loop in lock-step: one launch set and one readback per iteration for all
 * of them, a problem that has stopped is skipped on the device with its record and weights frozen.  The clique search and the
 * translation run per problem, in index order, as in the single call.
 *   per problem   upstream's early returns (unequal sizes, N <= 3): status -1, identity T, the clique buffer untouched; the rest of the batch runs.
 *   whole call    checked for every problem before any device work: a problem the single call would refuse (a bad stride, an index outside its cloud,
 *                 N > 8192, one index list without the other, a NULL it needs) and a non-finite or negative noise_bound make the call return the single
 *                 call's code, name the first such problem's index in mulls_last_error, and leave every result at status -1 / identity.
 *   scratch_limit_bytes  bounds each of the two device arenas the call holds: the graph phase's (the two bit matrices, 2 N ceil(N / 64) 8 bytes per
 *                 problem, and the small per-problem arrays: 1.0 MB + 16.8 MB at N = 8192) and the GNC phase's weights (C (C - 1) / 2 doubles per
 *                 problem, C known only after the search).  The batch is cut into consecutive sub-batches that fit, for each phase on its own; a problem
 *                 larger than the limit runs alone.  0: MULLS_TEASER_BATCH_DEFAULT_SCRATCH_BYTES, a value chosen without a measurement.  The device clique search's workers (per problem, as in the
 *                 single call) are not counted.
 * n_problems = 0: MULLS_OK. */
#define MULLS_TEASER_BATCH_DEFAULT_SCRATCH_BYTES (512ull << 20)
typedef struct mulls_teaser_problem
{
	mulls_cloud tgt, src;			  /* host or device-resident clouds, by the single call's rules (strides included) */
	const int32_t *tgt_idx, *src_idx; /* both NULL: pair i = point i of each cloud; both set: the n_corr pairs they name */
	uint32_t n_corr;				  /* read only when the index lists are set */
	uint32_t clique_cap;
	int32_t *clique;				  /* clique_cap entries, or NULL with clique_cap = 0 */
} mulls_teaser_problem;

int mulls_coarse_reg_teaser_batch(mulls_ctx *ctx, const mulls_teaser_problem *problems, uint32_t n_problems, const mulls_teaser_params *params,
								  uint64_t scratch_limit_bytes, mulls_teaser_result *results);

/* ---- statistical outlier removal: CFilter<PointT>::sor_filter (include/common/cfilter.hpp:204-247) ----
 * The filter of the merged map mulls_slam writes at the end of a run (test/mulls_slam.cpp:1009, sor_filter(pc_map_merged, 20, 2.0) under --map_filter_on).
 * Upstream's body is pcl::StatisticalOutlierRemoval.  PCL is not available where this library is built and tested, so nothing below was checked
 * against it: the lines marked [PCL] restate statistical_outlier_removal.hpp of PCL 1.8 - 1.10 from memory, the lines marked [LIB] are defined by this
 * library.  tests/sor_restated.py restates all of it independently in numpy, bit for bit.  DESIGN.md section 7.2 has the same list with its reasons.
 *   neighbours [PCL / FLANN] for point i the mean_k + 1 smallest squared distances to the points of the same cloud, itself included; float
 *              d2 = (dx dx + dy dy) + dz dz, no contraction (L2_Simple).  Only the multiset of the values matters: no tie order is involved.  The
 *              smallest value (0: the point itself or a coincident one) is dropped.
 *   distance   [PCL] dist_i = (float)(sum over the mean_k remaining values, ascending, of sqrt((double)d2) / mean_k), the sum in double.
 *              [LIB] the square root is the double one: PCL writes an unqualified sqrt(nn_dists[k]), and which overload that is depends on the headers in
 *              scope.  (No committed expectation depends on the choice: tests/test_sor.py checks every fixture's keep mask under both readings.)
 *   statistics [PCL] sum = sum of (double)dist_i, sq_sum = sum of (double)(dist_i * dist_i) (the product in float), mean = sum / n,
 *              variance = (sq_sum - sum * sum / n) / (n - 1), stddev = sqrt(variance), threshold = mean + std_mul * stddev, all in double.  A variance
 *              that rounding made negative gives a NaN threshold, and every point passes: the arithmetic is followed, not repaired.
 *              [LIB] the order of the two sums (PCL: index order): 16384 strided partial sums (partial p adds i = p, p + 16384, ... in ascending i),
 *              then a pairwise tree over the partials (half = 8192, 4096, ..., 1: s[p] += s[p + half] for p < half).
 *   selection  [PCL] point i is removed iff (double)dist_i > threshold; the kept points stay in index order.  negative and keep_organized are not offered.
 *   refused    [LIB] n == 0: MULLS_OK, nothing kept.  1 <= n <= mean_k: MULLS_E_INVALID (upstream reads past the k-NN result there).  mean_k < 1:
 *              MULLS_E_INVALID; mean_k > 64: MULLS_E_UNSUPPORTED.  A non-finite coordinate or std_mul: MULLS_E_INVALID (PCL leaves non-finite points out of
 *              the tree and passes them through: not reproduced).  More than 2^24 = 16777216 points: MULLS_E_UNSUPPORTED.
 * The search is exact: a hash of occupied cells (cell edge from the data; part of the implementation, not of the result), Chebyshev rings with a
 * conservative certificate, coarser levels and finally brute force for the queries the rings do not certify. */
typedef struct mulls_sor_params
{
	int32_t mean_k; /* [20] */
	int32_t reserved;
	double std_mul; /* [2.0] */
} mulls_sor_params;

typedef struct mulls_sor_report
{
	uint32_t n_in, n_kept;
	double mean, stddev, threshold;
	float ms_total;		 /* wall time of the call */
	uint32_t n_fallback; /* queries that left the grid walk and were answered by brute force */
} mulls_sor_report;

void mulls_sor_default_params(mulls_sor_params *p);
/* returns MULLS_OK or MULLS_E_* (the list above; MULLS_E_INVALID also for a bad stride).  cloud: host memory (48-byte records at any stride that is a
 * multiple of 4 and at least 48) or a device-resident cloud of 48-byte records (mulls_map_cloud, mulls_block_cloud).  All outputs are host memory.
 * out: the kept records, byte for byte, in index order, at most cap of them (NULL with cap 0 allowed); *n_out: the full kept count.
 * kept_idx: their ascending indices, at most idx_cap (NULL / 0 allowed).  mean_dist: NULL, or n floats: every point's dist_i.  report may be NULL. */
int mulls_sor_filter(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_sor_params *params, void *out, uint32_t cap, uint32_t *n_out, int32_t *kept_idx,
					 uint32_t idx_cap, float *mean_dist, mulls_sor_report *report);

/* ---- key-point non-maximum suppression: CFilter<PointT>::non_max_suppress (include/common/cfilter.hpp:1183-1240 and :1243-1312) ----
 * The thinning of the key points in front of the global registration (test/mulls_reg.cpp:145-149, both clouds, radius 0.25 * pca_neigh_r) and of every new
 * submap's pc_vertex in front of loop closure (test/mulls_slam.cpp:462).  Lines marked [UP] are upstream's, [PCL] restate pcl::search::KdTree::radiusSearch
 * (FLANN's L2_Simple) from memory — PCL is not available where this library is built and tested, nothing was compared with it —, [LIB] are this library's.
 * tests/nms_restated.py restates all of it in numpy; DESIGN.md section 7.3 has the same list with its reasons.
 *   gate     [UP :1189-1191] n < 10: nothing happens.  The cloud is returned unchanged and in input order (kept_idx and order are the identity),
 *            report.ran = 0.
 *   key      [UP :1193] normal[3], the float at byte 28 of the 48-byte record.
 *   order    [UP + this toolchain] std::sort with the comparator a.key > b.key.  Equal keys fall as this toolchain's std::sort leaves them: the keys
 *            are sorted on the host as (key, index) pairs by that std::sort (the lines mulls_classify_nground runs for its class clouds).  The
 *            permutation depends on the keys and on n only.
 *   walk     [UP :1211-1228] visit in that order; the first unvisited point is kept, every point within the radius of a kept point is erased: a point
 *            is kept exactly when no earlier kept point lies within the radius.
 *   radius   [PCL / FLANN] d2 < r2, strict; r2 = (float)((double)r * (double)r); d2 = (dx dx + dy dy) + dz dz in float, no contraction.  A negative
 *            radius follows this arithmetic and so acts as |r|; radius 0 keeps everything, in sorted order.
 *   output   [UP :1230] the kept records, byte for byte, in visiting order.
 *   refused  [LIB] a NaN key: MULLS_E_INVALID (upstream's comparator is then no strict weak order and its sort undefined).  A non-finite coordinate or
 *            radius, a bad stride: MULLS_E_INVALID.  More than MULLS_NMS_MAX_POINTS = 2^18 points: MULLS_E_UNSUPPORTED.  n == 0: MULLS_OK, nothing kept.
 * Not offered: the distance_adaptive_on mode of the out-of-place overload (:1285-1295; no upstream call site sets it); kd_tree_already_built = true
 * (upstream would query a tree built over the unsorted cloud with sorted indices; the one call site that names the argument passes false); the
 * pca_feature_t overload (:1314; its only caller is the commented-out detect_key_pts).
 * Two paths give the same bytes.  Path 1: the whole suppression in one workgroup with the cloud and a hashed cell grid in LDS, at most
 * MULLS_NMS_LDS_MAX_POINTS = 4096 points (32 bytes of LDS per point and 4 per bucket: 144 KiB of the 160 KiB of a CU).  Path 2: the kernels of
 * mulls_classify_nground's class-cloud suppression, any n up to the limit.  Path 0 takes path 2 at every size: path 1 measures slower (0.65 - 0.80 ms
 * against 0.20 - 0.25 ms per call on the demo key points and at 4096 points, profiles/nms_kernel_stats.txt) and runs on request only. */
#define MULLS_NMS_MAX_POINTS (1u << 18)
#define MULLS_NMS_LDS_MAX_POINTS 4096u
typedef struct mulls_nms_params
{
	float non_max_radius; /* [0.25] */
	int32_t path;		  /* 0 = the library chooses, 1 = one workgroup, 2 = multi-launch.  The bytes of every output are the same on each path;
							 1 beyond its size limit: MULLS_E_UNSUPPORTED */
} mulls_nms_params;

typedef struct mulls_nms_report
{
	uint32_t n_in, n_kept;
	int32_t ran;	 /* 0: below the gate, nothing done */
	int32_t path;	 /* the path taken (0 when ran == 0) */
	uint32_t rounds; /* fixed-point rounds until every point was decided: at most the depth of the longest suppression chain */
	float ms_total;	 /* wall time of the call */
} mulls_nms_report;

void mulls_nms_default_params(mulls_nms_params *p); /* radius 0.25, path 0 */
/* returns MULLS_OK or MULLS_E_* (the list above).  cloud: host memory (48-byte records at any stride that is a multiple of 4 and at least 48) or a
 * device-resident cloud of 48-byte records (mulls_map_cloud, mulls_block_cloud); it is never modified.  All outputs are host memory and any may be NULL
 * (out with cap 0, kept_idx with idx_cap 0).  out: the kept records in visiting order, at most cap of them; *n_out: the full count of kept records;
 * kept_idx: their indices into the input, in visiting order, at most idx_cap; order: n ints, the whole visiting permutation (order[i] = the input index
 * of the point visited i-th: what the out-of-place overload leaves cloud_in sorted by). */
int mulls_non_max_suppress(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_nms_params *params, void *out, uint32_t cap, uint32_t *n_out, int32_t *kept_idx,
						   uint32_t idx_cap, int32_t *order, mulls_nms_report *report);

/* Many key-point clouds per call: problem b gets, byte for byte, what mulls_non_max_suppress gives for problems[b].cloud with the same params
 * (reports[b].n_in, n_kept and ran; the records in out, the entries of kept_idx, the whole order): the gate, the key, the host std::sort, the radius
 * test and the cell edge above are not redefined.  reports[b].path is the path problem b took and rounds that path's count; ms_total is the wall time of
 * the whole call, the same in every report.  reports may be NULL.
 *   paths       params->path 0: a problem of 10 .. MULLS_NMS_LDS_MAX_POINTS points takes path 1 — here as ONE launch for the whole sub-batch, one
 *               workgroup per problem (B clouds on B compute units cost about what one costs, and no host poll separates the rounds) —, a larger one
 *               path 2.  path 1: a problem beyond MULLS_NMS_LDS_MAX_POINTS that passes the gate: MULLS_E_UNSUPPORTED.  path 2: every problem through
 *               the multi-launch kernels.  Problems on path 2 run one after another inside the call, each as the single call runs it: they are the
 *               exception (key-point clouds have a few thousand points), and nothing about them is batched.
 *   per problem n == 0: nothing kept.  n < 10: the identity, ran = 0.  The rest of the batch runs.
 *   refused     a problem the single call would refuse (a bad stride, a NULL pointer that is needed, a non-finite coordinate or radius, a NaN key, more
 *               than MULLS_NMS_MAX_POINTS points), or NULL params: the call returns the single call's code, mulls_last_error names the first such
 *               problem ("problem 2"), no output of any problem is written and every report is zeroed.  Host clouds are checked before any device
 *               work; a NaN key or non-finite coordinate of a device-resident cloud is found by the key pass, which runs for the whole call before
 *               anything is written.  n_problems == 0: MULLS_OK.
 *   arena       scratch_limit_bytes (0: MULLS_NMS_BATCH_DEFAULT_SCRATCH_BYTES) bounds the call's device arena, which belongs to the context, only
 *               grows and is released with it.  Per staged point it holds the 48-byte record in visiting order (a device-resident cloud: also its key
 *               and its permutation entry), per problem a header, the kept positions and room for the kept records it may return.  The batch is cut
 *               into consecutive sub-batches that fit; a problem larger than the limit runs alone.  The same cloud may appear in several problems:
 *               it is staged once per distinct (pts, n, stride) of a sub-batch, and no result depends on that.
 * A sub-batch is: one key launch over its device-resident clouds and one download (for all sub-batches, first); the orders on the host's thread pool;
 * one upload of the records in visiting order (device-resident clouds: of the permutations, and one gather launch); the suppression launch; one download
 * of the headers and kept positions and one of the kept records. */
typedef struct mulls_nms_problem
{
	mulls_cloud cloud; /* host or device-resident, by the single call's rules (strides included); never modified */
	void *out;		   /* cap records of 48 bytes, or NULL with cap = 0 */
	int32_t *kept_idx; /* idx_cap entries, or NULL with idx_cap = 0 */
	int32_t *order;	   /* cloud.n entries, or NULL */
	uint32_t cap, idx_cap;
} mulls_nms_problem;

#define MULLS_NMS_BATCH_DEFAULT_SCRATCH_BYTES (512ull << 20) /* a value chosen without a measurement */
int mulls_non_max_suppress_batch(mulls_ctx *ctx, const mulls_nms_problem *problems, uint32_t n_problems, const mulls_nms_params *params,
								 uint64_t scratch_limit_bytes, mulls_nms_report *reports);
/* bytes of the batch entry's device arena as it stands (0 before the first call that needed one): what tests watch grow */
uint64_t mulls_nms_batch_arena_bytes(const mulls_ctx *ctx);

/* ---- scan preparation: the raw-scan steps of CFilter in front of extract_semantic_pts and of the map export (include/common/cfilter.hpp) ----
 * What test/mulls_slam.cpp runs on pc_raw before the feature extraction (:359-362 and :404-412: dist_filter, vertical_intrinsic_calibration,
 * get_pts_timestamp_ratio_in_frame) and per frame of the merged map (:966-974: calibration, dist_filter, random_downsample, time ratio), on the device and
 * in place.  Lines marked [UP] are upstream's, [LIB] this library's.  tests/scanprep_restated.py restates all of it with Python's math functions per
 * element; DESIGN.md section 7.5 has the same list with its reasons.  PCL is not available where this library is built and tested: nothing below (the
 * mapper's pcl::transformPointCloud included) was compared with it.
 *   order        [UP] calib_first = 0: dist filter, calibration (the frame loop, :404-407); 1: calibration, dist filter (the export, :966-969).  Then
 *                random_downsample, then the time ratio, in both.  Each step sees the cloud as the steps before it left it.
 *   calibration  [UP :250-291] angle == 0 (or calib_on = 0): nothing.  angle >= 180.0: every z is negated, nothing else.  Otherwise per point
 *                dist = (double)sqrtf((x x + y y) + z z), products, sum and root in float; v = asin((double)z / dist); vc = v + angle / 180.0 * M_PI;
 *                hs = cos(vc) / cos(v); x = (float)((double)x hs), y likewise, z = (float)(dist sin(vc)).  A point at the origin becomes NaN: the
 *                arithmetic is followed, not repaired.
 *                [LIB] asin, cos and sin are detmath.h's asin_cr, cos_cr, sin_cr (double-double evaluation rounded to double: the correctly rounded
 *                value, the same bits on the host and on the device) where upstream calls the C library; no device math library is involved.
 *   dist filter  [UP :806-831] a point stays iff d2 < max max && d2 > min min with d2 = (double)(x x + y y), products and sum in float, the limits'
 *                squares in double.  (The lines mulls_extract_features runs under apply_dist_filter.)
 *   thinning     [UP :730-747] downsample_ratio > 1: the points whose index i in the cloud as it stands then has i % ratio == 0 stay.
 *   time ratio   [UP :424-441] mode 1: last / first = the max_ / min_ folds (utility.hpp:31-32, seeded with -DBL_MAX / DBL_MAX) of (double)curvature over
 *                the cloud as it stands then (after thinning); last - first < scan_duration_ms * 0.75 replaces the duration by (float)(last - first);
 *                curvature = (float)min_(1.0, max_(0.0, (last - curvature) / duration)).  Equal stamps give 0 / 0: the NaN is stored.
 *                [LIB] a NaN time stamp among the points that stay: MULLS_E_INVALID, the cloud untouched (upstream's folds then depend on the order).
 *                [UP :443-466] mode 2: ang = atan2(y, x), + 2 pi if negative, + begin angle / 180.0 * M_PI, - 2 pi if >= 2 pi;
 *                curvature = (float)((2 pi - ang) / (2 pi)), on the coordinates as they stand then.
 *                [LIB] atan2 is detmath.h's atan2_cr on the coordinates widened to double.  (Upstream writes std::atan2 on two floats, which C++ resolves
 *                to the float overload; the double evaluation is this library's definition and differs from a float atan2 by that function's rounding.)
 *   refused      [LIB] a stride other than 48, min_dist / max_dist / the angles / scan_duration_ms not finite, timestamp_mode outside 0..2:
 *                MULLS_E_INVALID.  More than 2^24 points: MULLS_E_UNSUPPORTED.  n == 0: MULLS_OK.
 * The work runs in chunks of MULLS_SCAN_CHUNK points, one workgroup each; nothing in the result depends on the chunk size or on which workgroup runs first. */
#define MULLS_SCAN_CHUNK 256u
#define MULLS_SCAN_MAX_POINTS (1u << 24)
typedef struct mulls_scan_prep_params
{
	uint8_t calib_on, dist_filter_on;	/* [0, 0] */
	uint8_t calib_first;				/* 0: dist filter -> calibration (frame loop, :404-407); 1: calibration -> dist filter (export, :966-969) */
	uint8_t reserved_;
	int32_t downsample_ratio;			/* [1] random_downsample(ratio), <= 1: off; always after both steps above */
	int32_t timestamp_mode;				/* [0] 0 off, 1 from time stamps, 2 from azimuth; always last */
	float scan_duration_ms;				/* [100] */
	double vertical_ang_correction_deg; /* [0.0] */
	double min_dist, max_dist;			/* [1.0, 120.0] */
	double scan_begin_ang_deg;			/* [180.0]; mulls_slam passes 90.0 */
} mulls_scan_prep_params;

typedef struct mulls_scan_prep_report
{
	uint32_t n_in, n_after_dist, n_out;
	uint32_t reserved;
	double first_timestamp, last_timestamp; /* mode 1; DBL_MAX / -DBL_MAX (the folds' seeds) when nothing stays */
	float scan_duration_used;				/* mode 1: what the ratios were divided by */
	float ms_total;							/* wall time of the call */
} mulls_scan_prep_report;

void mulls_scan_prep_default_params(mulls_scan_prep_params *p);
/* returns MULLS_OK or MULLS_E_* (the list above).  pts: n 48-byte records in host memory (one upload, one download of the records that stay) or in device
 * memory (a cloud of the library's or any device allocation of the caller's: in place, nothing crosses PCIe), told apart as mulls_motion_compensate
 * does.  The records that stay are left packed at the front, in input order, every field but x, y, z and curvature as it was; the records behind
 * *n_out keep what they held.  report may be NULL. */
int mulls_scan_prepare(mulls_ctx *ctx, void *pts, uint32_t n, uint32_t stride, const mulls_scan_prep_params *params, uint32_t *n_out,
					   mulls_scan_prep_report *report);

/* ---- the merged map mulls_slam exports (test/mulls_slam.cpp:959-1015), kept in device memory ----
 * Per frame, in this order: the scan preparation above with calib_first taken as 1 (:966-974); when compensate is set,
 * apply_motion_compensation(pc_raw, adjacent_tran) with threshold 0 (:977-981; mulls_motion_compensate's arithmetic, theta = acos(|q.w|) by the host's
 * C library once per frame); pcl::transformPointCloud by pose (:982: positions in double, stored as float, every other field copied); appended in frame
 * order (:990).  mulls_mapper_cloud hands the result to mulls_sor_filter (:1009).  Many frames per call run in lock step: one launch per pass for all of
 * them.  The viewer's thinning (:991) and write_map_each_frame are not part of this; the ground-truth map (:996-1005) is a second mapper fed pose_gt.
 * The export's picture of the map (:1016-1025, generate_2d_map) is mulls_map_image_2d below, on the map where it lies.
 *   capacity [LIB] frames are appended while they fit.  If frame k does not fit, frames 0 .. k-1 of the call stay appended, frames k onward are not, and
 *            the call returns MULLS_E_UNSUPPORTED with report.frames_added = k and report.n_needed = the size the map would have had with every frame.
 *   refused  [LIB] what mulls_scan_prepare refuses, for any frame: MULLS_E_INVALID and nothing is appended.  A mapper of another context: MULLS_E_INVALID.
 * A mapper belongs to its context: mulls_destroy(ctx) also destroys the mappers still alive. */
typedef struct mulls_mapper mulls_mapper;
typedef struct mulls_mapper_frame
{
	mulls_cloud scan;		 /* host or device, 48-byte records; never modified */
	double pose[16];		 /* pose_optimized, column-major */
	double adjacent_tran[16]; /* pose_i^-1 * pose_{i-1} (:979); read only when compensate is set */
	int32_t compensate;		 /* 1: apply_motion_compensation(pc_raw, adjacent_tran), threshold 0 (:977-981) */
	int32_t reserved;
} mulls_mapper_frame;

typedef struct mulls_mapper_report
{
	uint32_t frames_added; /* frames of this call that were appended */
	uint32_t n_before;	   /* the map's size before the call */
	uint32_t n_after;	   /* ... and after it */
	uint32_t reserved;
	uint64_t n_needed;	   /* the size the map has (or would have had) with every frame of the call appended */
	float ms_total;		   /* wall time of the call */
	uint32_t reserved2;
} mulls_mapper_report;

int mulls_mapper_create(mulls_ctx *ctx, uint32_t capacity_points /* <= 2^24, what mulls_sor_filter takes */, mulls_mapper **out);
void mulls_mapper_destroy(mulls_ctx *ctx, mulls_mapper *mapper);
/* frame_n_out: NULL, or n_frames counts: what each frame contributed (frames that were not appended: what they would have).  report may be NULL. */
int mulls_mapper_add(mulls_ctx *ctx, mulls_mapper *mapper, const mulls_mapper_frame *frames, uint32_t n_frames, const mulls_scan_prep_params *prep,
					 uint32_t *frame_n_out, mulls_mapper_report *report);
/* the map as a device-resident cloud (stride 48), valid until the next add / clear / destroy: for mulls_sor_filter, mulls_non_max_suppress, ... */
int mulls_mapper_cloud(mulls_ctx *ctx, const mulls_mapper *mapper, mulls_cloud *out);
/* records first .. of the map to host memory, at most cap of them; *n: the map's size minus first (pts NULL with cap 0: the size query) */
int mulls_mapper_download(mulls_ctx *ctx, const mulls_mapper *mapper, uint32_t first, void *pts, uint32_t cap, uint32_t *n);
int mulls_mapper_clear(mulls_ctx *ctx, mulls_mapper *mapper);

/* ---- the pictures of a cloud: CloudUtility::get_cloud_cpt (include/common/utility.hpp:800-814), CFilter::generate_2d_map (cfilter.hpp:2751-2790) and
 * CFilter::pointcloud_to_rangeimage (:2714-2746) ----
 * What test/mulls_slam.cpp draws per frame from pc_raw (:722-733: the range image and a 400 x 400 bird's-eye view) and at the export from the merged map
 * (:1016-1025: merged_map_2d.png), on the device: a device-resident cloud (mulls_mapper_cloud, mulls_block_cloud, mulls_map_cloud, any device allocation)
 * crosses PCIe in no direction, only the images and the report come down.  Lines marked [UP] are upstream's, [LIB] this library's, "from memory" marks
 * OpenCV's inside as it is restated here.  OpenCV, PCL and Eigen are not available where this library is built and tested: NOTHING BELOW WAS COMPARED WITH
 * THEM.  tests/images_restated.py restates all of it in numpy float32 / float64 element-wise operations, and every comparison with it is equality of
 * bytes; DESIGN.md section 7.12 says what is upstream's, what is OpenCV's and what is this library's, with the reasons.
 *
 * Centre point (mulls_cloud_centre)
 *   term     [UP :807-809] the term of point i is x_i / (float)n: upstream divides a float by an int, a float division.  The term is widened to double
 *            and added; y and z likewise.  n == 0: (0, 0, 0).  Non-finite coordinates follow the arithmetic.
 *   order    [LIB] MULLS_NDT_TREE's strided-partial rule: lane l adds the terms of the points l, l + MULLS_NDT_TREE, .. in that order, from 0, then for
 *            w = MULLS_NDT_TREE / 2 .. 1: partial[l] += partial[l + w], l < w.  Upstream's sequential order cannot be kept on a device; this is the rule
 *            of every other long sum of this header.
 *   refused  more than MULLS_SCAN_MAX_POINTS points: MULLS_E_UNSUPPORTED.  A stride other than 48: MULLS_E_INVALID.
 *
 * 2-D map image (mulls_map_image_2d)
 *   shift    [UP :2757-2768] shift_x = (float)c.x, shift_y = (float)c.y of the centre above over the same cloud when `shift` is set, else 0.
 *   height   [UP :2775] a point is skipped when (double)z < min_height || (double)z > max_height.  A NaN z passes.
 *   pixel    [UP :2778-2779] dx = (double)(x - shift_x) * m2pix + (double)(map_width / 2): the difference in float, map_width / 2 the integer division;
 *            dy = (double)(-(y - shift_y)) * m2pix + (double)(map_height / 2).  The pixel is (int)dx, (int)dy: truncation toward zero, so every dx in
 *            (-1, 0) lands in column 0.  The quirk is kept.
 *            [LIB] a point takes part iff t = trunc(dx), evaluated in double, has 0 <= t < map_width, and likewise for y.  Upstream's cast of a
 *            non-finite or huge double to int is undefined; such points are skipped (counted as outside the frame).
 *   counts   counts[y * map_width + x] = the number of points in the pixel.
 *   8 bits   [UP shape :2786-2787, OpenCV from memory] map -= min_points_in_pix; map.convertTo(map, CV_8UC1, -255.0 / (max - min), 255).
 *            [LIB] restated: a = (float)(-255.0 / (double)(max_points_in_pix - min_points_in_pix)); v = (float)(count - min_points_in_pix) * a + 255.0f,
 *            the product and the sum in float and not contracted; image = clamp(round-half-to-even(v), 0, 255).  OpenCV's working type (float for
 *            a 32-bit integer source) and its rounding (cvRound, saturate_cast) were restated from memory and not compared with OpenCV.
 *   refused  [LIB] MULLS_E_INVALID with nothing written: max_points_in_pix == min_points_in_pix; map_width or map_height < 1 or their product above
 *            MULLS_IMAGE_MAX_PIXELS; m2pix, min_height or max_height NaN; count_form outside 0..2; a stride other than 48; a NULL image.  More than
 *            MULLS_SCAN_MAX_POINTS points: MULLS_E_UNSUPPORTED.  n == 0: the all-empty image, every pixel what count 0 gives.
 *
 * Range image (mulls_range_image); upstream hard-codes the HDL-64 constants (:2717-2721), which are the defaults of mulls_range_image_params
 *   per point, in this order:
 *            [UP :2730] d = sqrtf((x x + y y) + z z).
 *            [LIB] hor = (float)atan2_cr((double)y, (double)x); a = (float)asin_cr((double)(z / d)), the quotient in float.  atan2_cr and asin_cr are
 *            detmath.h's correctly rounded functions where upstream calls the C library's float overloads: mulls_scan_prepare's convention (the double
 *            evaluation is this library's definition and differs from a float function by that function's rounding).
 *            [UP :2732] ver = (float)(((double)a / M_PI) * 180.0).
 *            [UP :2734] u = (float)((0.5 * (1 - (double)hor / M_PI)) * width).
 *            [UP :2735] v = (1 - (f_up - ver) / (f_up + f_down)) * height, entirely in float.
 *            [UP :2737-2738] c = clamp((int)u, 0, width - 1), r = clamp((int)v, 0, height - 1).
 *            [LIB] a point whose u or v is not finite is skipped (upstream's cast is undefined there; the scanner's own origin is such a point); the
 *            clamp is applied to the truncated float before the conversion to int.
 *            [UP :2743] value = (uint8_t)(255.0 * min_(1.0, (double)(d / max_distance))): the quotient in float, the conversion truncates.
 *            [UP :2743] the value is written at row height - 1 - r, column c.
 *   overlap  [UP] a pixel holds the value of the HIGHEST-INDEX point that lands in it: upstream's sequential overwrite.  Pixels nobody lands in are 0.
 *            [LIB] on the device a pixel is the maximum of the 32-bit words (index << 8) | value: the limit of MULLS_SCAN_MAX_POINTS = 2^24 points is
 *            what makes that word fit, and the maximum is independent of the order the points arrive in.
 *   refused  [LIB] MULLS_E_INVALID with nothing written: width or height < 1 or their product above MULLS_IMAGE_MAX_PIXELS; f_up_deg, f_down_deg or
 *            max_distance not finite, max_distance <= 0 (the value's conversion would be of a negative or NaN double); a stride other than 48; a NULL
 *            image.  More than MULLS_SCAN_MAX_POINTS points: MULLS_E_UNSUPPORTED.
 *
 * Many scans per call (mulls_scan_images_batch): every scan gets the bytes of its single calls, whatever the batch size and its position.  The single
 * calls are this path with one scan.  Per call (per sub-batch of a call whose images and staged host clouds exceed the arena's budget of 1 GiB; a scan
 * beyond it runs alone): one zeroing of all counts and words, one launch per pass over a chunk table of all scans — chunks of MULLS_SCAN_CHUNK points, one
 * workgroup each —, one launch that converts all pixels to 8 bits, one download of all images and reports.  Both images are integer results of commutative
 * atomics (add, max): nothing depends on which workgroup runs first.  A refusal (any scan's) writes no output of the call.  n_scans == 0: MULLS_OK. */
#define MULLS_IMAGE_MAX_PIXELS (1u << 26)
typedef struct mulls_image2d_params
{
	double m2pix;				/* [1] pixels per metre */
	int32_t map_width;			/* [1920] */
	int32_t map_height;			/* [1080] */
	int32_t min_points_in_pix;	/* [20] */
	int32_t max_points_in_pix;	/* [1000] */
	double min_height;			/* [-FLT_MAX] */
	double max_height;			/* [FLT_MAX] */
	int32_t shift;				/* [1] shift_or_not: the picture is centred on the cloud's centre point */
	int32_t count_form;			/* [0] which form of the counting pass runs: 0 the library's choice (form 2, the faster in profiles/images.txt), 1 one atomic add per
								   point, 2 a wave folds runs of equal pixels among neighbouring lanes and one lane per run adds the run's length.  Same bytes. */
} mulls_image2d_params;

typedef struct mulls_image2d_report
{
	double centre[3];		  /* the centre point that was used (computed also when shift is 0) */
	uint32_t n_counted;		  /* points that landed in a pixel */
	uint32_t n_skipped_height; /* points outside [min_height, max_height] */
	uint32_t n_skipped_frame;  /* points of the height range outside the picture (non-finite ones included) */
	float ms_total;			  /* wall time of the call (a batch: of the whole call, in every report) */
} mulls_image2d_report;

typedef struct mulls_range_image_params
{
	int32_t width;		/* [900] */
	int32_t height;		/* [64] */
	float f_up_deg;		/* [3] */
	float f_down_deg;	/* [25] */
	float max_distance; /* [70] */
	int32_t reserved;
} mulls_range_image_params;

void mulls_image2d_default_params(mulls_image2d_params *p);		   /* the export's values (test/mulls_slam.cpp:1018); the bird's-eye view of :731 is
																	  (4, 400, 400, 2, 50, -5, 15, no shift) */
void mulls_range_image_default_params(mulls_range_image_params *p); /* upstream's HDL-64 constants */
/* cloud: host memory or device memory, told apart as mulls_scan_prepare tells them apart; never modified.  All outputs are host memory. */
int mulls_cloud_centre(mulls_ctx *ctx, const mulls_cloud *cloud, double c[3]);
/* image: map_height rows of map_width bytes.  counts: NULL, or as many int32.  report may be NULL. */
int mulls_map_image_2d(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_image2d_params *p, uint8_t *image, int32_t *counts,
					   mulls_image2d_report *report);
/* image: height rows of width bytes */
int mulls_range_image(mulls_ctx *ctx, const mulls_cloud *scan, const mulls_range_image_params *p, uint8_t *image);
/* rp NULL: no range images (range_out is not read); bp NULL: no 2-D map images (bev_out and reports are not read).  range_out / bev_out: n_scans
 * pointers, one image each.  reports: NULL or n_scans of them. */
int mulls_scan_images_batch(mulls_ctx *ctx, const mulls_cloud *scans, uint32_t n_scans, const mulls_range_image_params *rp, const mulls_image2d_params *bp,
							uint8_t *const *range_out, uint8_t *const *bev_out, mulls_image2d_report *reports);
/* a binary PGM (P5, maxval 255) of an 8-bit image: what the export writes where upstream calls cv::imwrite.  Host code; MULLS_E_IO when the file cannot be
 * written, MULLS_E_INVALID for a NULL argument or a width or height < 1. */
int mulls_io_write_pgm(const char *path, const uint8_t *image, int32_t width, int32_t height);

/* ---- pose graph optimisation: GlobalOptimize::optimize_pose_graph_ceres (src/graph_optimizer.cpp:385-417, with set_pgo_problem_ceres :481-636) and update_optimized_edges (:713-776) ----
 * The step behind a closed loop: registration edges (mulls_result.T / .info) and the odometry chain in, one pose per node out — the poses
 * mulls_mapper_add takes.  Upstream hands the problem to Ceres.  Ceres is not available where this library is built and tested, so NOTHING BELOW WAS CHECKED
 * AGAINST CERES: lines marked [upstream] follow the reference's own code, lines marked [Ceres] restate Ceres's documented defaults (trust-region
 * Levenberg-Marquardt), lines marked [LIB] are this library's own choices where upstream's result rests on Ceres internals that cannot be pinned.
 * tests/pgo_restated.py restates all of it independently in numpy, bit for bit: every operation is + - * / sqrt in double, in the order written here
 * (the library is built without FMA contraction).  Matrices are column-major 4 x 4 / 6 x 6, quaternions are (x, y, z, w).
 *
 *   edges used [upstream] an edge is used iff its type is neither NONE nor HISTORY (:493, :540); an edge with a > b is taken as it comes; several edges
 *              between one pair are all summed.  "Edge index" below counts the used edges in input order.
 *   early return [upstream :513] (n_nodes - nodes with `fixed` set) > used edges: status -1, poses_out = pose_init verbatim, no device work; the rest of a
 *              batch still runs.
 *   classes    [upstream :533-629, quirks kept] with_reg = a used REGISTRATION edge exists, m = the smallest `a` among them; stable_index = m when
 *              with_reg, else 0.  For i ascending, the first rule that matches: (1) with_reg && i <= m: fixed; (2) `fixed` set: fixed; (3) `stable` set:
 *              unless free_all_nodes, box (t_limit, r_limit) and stable_index = i (with free_all_nodes neither); (4) otherwise: unless free_all_nodes,
 *              box ((i - stable_index) t_limit, (i - stable_index) r_limit), the factor converted to double first.  [LIB] fixed nodes are constants of
 *              the problem (upstream holds them inside +-1e-10); a box of width 0 is a box: the node stays an unknown and is projected onto its start.
 *              n_fixed / n_boxed / n_free count the three classes; the unknowns are the non-fixed nodes in ascending index, six each (dt, dtheta).
 *   state      [upstream / LIB] per node t and a unit quaternion from pose_init: Eigen's matrix -> quaternion (trace t = m00 + m11 + m22 summed left to
 *              right; t > 0: r = sqrt(t + 1), w = 0.5 r, r = 0.5 / r, x = (m21 - m12) r, y = (m02 - m20) r, z = (m10 - m01) r; else i = 0, i = 1 if
 *              m11 > m00, i = 2 if m22 > m_ii, j = (i + 1) % 3, k = (j + 1) % 3, r = sqrt(((m_ii - m_jj) - m_kk) + 1), q_i = 0.5 r, r = 0.5 / r,
 *              w = (m_kj - m_jk) r, q_j = (m_ji + m_ij) r, q_k = (m_ki + m_ik) r), then normalisation: q / sqrt(((x x + y y) + z z) + w w), four
 *              divisions.  Per edge (t^, q^) from T by the same rule.  The product p (x) q is Eigen's: x = ((pw qx + px qw) + py qz) - pz qy,
 *              y = ((pw qy + py qw) + pz qx) - px qz, z = ((pw qz + pz qw) + px qy) - py qx, w = ((pw qw - px qx) - py qy) - pz qz.  R(q) is Eigen's
 *              toRotationMatrix (utility.hpp:199-212): tx = 2x, ty = 2y, tz = 2z, twx = tx w, twy = ty w, twz = tz w, txx = tx x, txy = ty x,
 *              txz = tz x, tyy = ty y, tyz = tz y, tzz = tz z; R = [1 - (tyy + tzz), txy - twz, txz + twy; txy + twz, 1 - (txx + tzz), tyz - twx;
 *              txz - twy, tyz + twx, 1 - (txx + tyy)].  poses_out = [R(normalise(q)), t; 0 0 0 1] for every node, fixed ones included.
 *   residual   [upstream graph_optimizer.h:87-136] d = t_b - t_a, v_r = (R_0r d_0 + R_1r d_1) + R_2r d_2 with R = R(q_a) (v = R^T d), e_p = v - t^;
 *              P = q^ (x) conj(conj(q_a) (x) q_b), e_r = 2 vec(P); e = [e_p; e_r].
 *   weight W   [upstream / LIB] use_equal_weight: diag(1, 1, 1, r2, r2, r2), r2 = (double)quat_tran_ratio squared; else
 *              use_diagonal_information_matrix: diag(info_jj); else W_kl = 0.5 (info_kl + info_lk).  Upstream multiplies the residual by a matrix square
 *              root; only s = e^T W e enters the objective, so none is taken and a singular info stays legal.  u = W e (u_k = sum_l W_kl e_l),
 *              s = sum_k e_k u_k.  EVERY 6-TERM SUM HERE AND BELOW STARTS FROM 0.0 AND ADDS ITS PRODUCTS IN ASCENDING INNER INDEX.
 *   cost       [LIB] cost = 0.5 sum_edges rho(s).  robustify: d = (double)robust_delta, rho = s and w = 1 for s <= d d, else rho = (2 d) sqrt(s) - d d
 *              and w = d / sqrt(s) (Huber; no second-order correction).  Without robustify rho = s, w = 1.
 *   update     [LIB] t <- t + dt; q <- normalise(q (x) (0.5 dtheta, 1)): a retraction with the exponential map's first-order Jacobian and no
 *              transcendental function.
 *   Jacobians  [LIB] analytic, 6 x 6 per end, rows = residual, columns = (dt, dtheta): Ja = [-R^T, [v]x; 0, A], Jb = [R^T, 0; 0, B] with
 *              [v]x = [0, -v2, v1; v2, 0, -v0; -v1, v0, 0], column c of A = vec(P (x) (e_c, 0)), column c of B = -vec((q^ (x) (e_c, 0)) (x) Q),
 *              Q = conj(conj(q_a) (x) q_b).
 *   per edge   [LIB] WJa = w (W Ja), WJb = w (W Jb), wu = w u (the sum first, then times w); Haa = Ja^T WJa, Hab = Ja^T WJb, Hbb = Jb^T WJb,
 *              ga = Ja^T wu, gb = Jb^T wu (inner index = the residual row).  The block of (b, a) is Hab transposed.
 *   assembly   [LIB] H's block (i, j) and g_i: 0.0 plus the contributions of the used edges that touch them, in ascending edge index.  Only block rows
 *              i >= j are kept, and of a diagonal block only the lower triangle is read.
 *   damped step [Ceres] radius starts at 1e4, nu at 2.  D_jj = min(max(H_jj, 1e-6), 1e32) / radius; solve (H + D) delta = -g;
 *              model decrease md = -0.5 sum_j delta_j (g_j - D_jj delta_j)  ([LIB] this is -delta^T (g + H delta / 2) with H delta replaced by
 *              -g - D delta, the solved system's identity, so that no second matrix product is taken).  The step succeeds iff cost+ is finite, md > 0 and
 *              rr = (cost - cost+) / md > 1e-3; then radius = min(radius / max(1.0 / 3.0, 1 - (u u) u), 1e16) with u = 2 rr - 1, nu = 2; else
 *              radius = radius / nu, nu = 2 nu.  [LIB] a non-positive or non-finite pivot counts as a failed step.
 *   projection [LIB] applied to the candidate before its cost is taken.  A boxed node's t is clamped per component to pose_init's t -+ its limit (lo = t0 - l,
 *              hi = t0 + l; t < lo ? lo : t, then > hi ? hi).  Unless only_limit_translation its quaternion is (1) negated when
 *              ((x x0 + y y0) + z z0) + w w0 < 0, (2) clamped per component to q0 -+ its limit, (3) normalised again.  Upstream's bound is on the raw
 *              4-vector: the clamped 4-vector before the last normalisation is what this contract speaks of.
 *   iteration  [Ceres / LIB] in this order: no unknown -> stop NO_FREE (before anything else); iterations == num_iterations -> stop MAX_ITERATIONS
 *              (successful and failed steps both count); linearise at the state; max |g_j| <= 1e-10 -> stop GRADIENT; iterations += 1; factor and solve
 *              (failure: failed step); max |delta_j| <= 1e-8 -> stop STEP; candidate, projection, cost+, md; success: the state and cost move, and
 *              |cost - cost+| <= function_tolerance * cost (the cost before the step) -> stop FUNCTION_TOLERANCE; failure: radius < 1e-32 -> stop RADIUS.
 *              status 1 covers every stop (Ceres's "usable"); status -2: the initial cost is not finite (poses_out = pose_init verbatim).
 *   linear solve [LIB] H is stored as a block skyline: block row i runs from first_i (its smallest unknown neighbour, or i) to i.  Cholesky L L^T:
 *              block (i, j), j <= i: S = (H + D)_ij; for k = max(first_i, first_j) .. j - 1 ascending: S_rc -= (sum_m L_ik[r][m] L_jk[c][m]);
 *              j < i: L_ij[r][c] = (S_rc - L_ij[r][0] L_jj[c][0] - ... - L_ij[r][c-1] L_jj[c][c-1]) / L_jj[c][c], one subtraction per product, c ascending;
 *              j = i: the scalar Cholesky of the lower triangle, column c ascending: x = S_rc - L[r][0] L[c][0] - ... - L[r][c-1] L[c][c-1];
 *              r = c: the pivot x must be finite and > 0, L[c][c] = sqrt(x); r > c: L[r][c] = x / L[c][c].  Forward, y = -g: for j ascending:
 *              y_j[r] = (y_j[r] - L_jj[r][0] y_j[0] - ... ) / L_jj[r][r], r ascending; then y_i[r] -= (sum_m L_ij[r][m] y_j[m]) for every row i > j that
 *              holds block (i, j).  Backward: for k descending: x_k[r] = (y_k[r] - L_kk[r+1][r] x_k[r+1] - ... - L_kk[5][r] x_k[5]) / L_kk[r][r],
 *              r descending; then y_j[c] -= (sum_m L_kj[m][c] x_k[m]) for j = first_k .. k - 1.  THE VALUE OF EVERY ENTRY IS FIXED, NOT THE SCHEDULE:
 *              the device factors column by column and updates the trailing rows of a column in parallel, with these bits.
 *   sums       [LIB] the cost and md: 256 strided partials (partial l = 0.0 + the terms l, l + 256, ... ascending), then the tree
 *              p[l] += p[l + w] for w = 128, 64, ..., 1; maxima are exact in any order.
 *   edge check [upstream :713-776, :1041-1050] on the host after the solve, per used REGISTRATION / ADJACENT edge (SMOOTH edges enter the solve but not
 *              the check): with the output poses, R = Ra^T Rb, t = Ra^T (tb - ta), Rd = R^T R^, td = R^T (t^ - t)  ([LIB] rigid inverses and 3-term
 *              sums left to right instead of Eigen's general 4 x 4 inverse); wrong iff sqrt((tdx tdx + tdy tdy) + tdz tdz) > (double)translation_thre or
 *              2 atan2(|vec|, |w|) of Rd's normalised quaternion > (double)rotation_thre / 180.0 * pi, atan2 from detmath.h.  edge_wrong[e] (per
 *              input edge, 0 for edges not checked), wrong_edges, correct_reg_edges (REGISTRATION edges not wrong),
 *              edges_ok = !((double)wrong / (double)checked > (double)ratio_thre || correct_reg == 0) (0 checked edges: the quotient is NaN, as upstream's).
 *              The library changes no edge: the bridge (cregistration_hip.hpp) applies upstream's consequences.
 * Capacity: MULLS_PGO_MAX_NODES nodes, MULLS_PGO_MAX_EDGES edges and MULLS_PGO_MAX_BLOCKS skyline blocks per problem (a 4096-node chain has 4095 edges and 8189 blocks, a
 * 512-node graph with every edge 130816 edges and 131328 blocks); above them MULLS_E_UNSUPPORTED. */
#define MULLS_PGO_MAX_NODES 4096u
#define MULLS_PGO_MAX_EDGES 131072u
#define MULLS_PGO_MAX_BLOCKS 262144u
#define MULLS_PGO_BATCH_DEFAULT_SCRATCH_BYTES (256ull << 20) /* a value chosen without a measurement */
enum mulls_pgo_edge_type /* upstream's constraint_type (utility.hpp) */
{
	MULLS_PGO_REGISTRATION = 0,
	MULLS_PGO_ADJACENT = 1,
	MULLS_PGO_HISTORY = 2,
	MULLS_PGO_SMOOTH = 3,
	MULLS_PGO_NONE = 4
};
enum mulls_pgo_termination
{
	MULLS_PGO_TERM_NOT_RUN = 0, /* status -1 / -2 */
	MULLS_PGO_TERM_MAX_ITERATIONS = 1,
	MULLS_PGO_TERM_FUNCTION_TOLERANCE = 2,
	MULLS_PGO_TERM_GRADIENT = 3,
	MULLS_PGO_TERM_STEP = 4,
	MULLS_PGO_TERM_RADIUS = 5,
	MULLS_PGO_TERM_NO_FREE = 6
};
typedef struct mulls_pgo_node
{
	double pose_init[16];	/* cloudblock_t::pose_init, column-major */
	uint8_t fixed, stable;	/* pose_fixed, pose_stable */
	uint8_t reserved[6];
} mulls_pgo_node;
typedef struct mulls_pgo_edge
{
	int32_t a, b;	  /* block1 / block2 ->id_in_strip: indices into the nodes */
	int32_t type;	  /* con_type, enum mulls_pgo_edge_type */
	int32_t reserved;
	double T[16];	  /* Trans1_2, column-major */
	double info[36]; /* information_matrix, column-major */
} mulls_pgo_edge;
typedef struct mulls_pgo_params
{
	int32_t num_iterations;	 /* [100] mulls_slam.cpp:181-182 (max_iter_inter_submap / max_iter_inner_submap; pgo_param_t's own 50, utility.hpp:771, is overwritten at :601) */
	uint8_t robustify;		 /* [0] mulls_slam.cpp:190 robust_kernel_on, set at :599 (utility.hpp:760 says true) */
	uint8_t use_equal_weight; /* [0] utility.hpp:761, mulls_slam.cpp:170 */
	uint8_t use_diagonal_information_matrix; /* [0] utility.hpp:763, mulls_slam.cpp:185 */
	uint8_t free_all_nodes;	 /* [0] utility.hpp:764, mulls_slam.cpp:191 */
	uint8_t only_limit_translation; /* [0] utility.hpp:762 */
	uint8_t reserved0[3];
	float robust_delta;		 /* [1.0] utility.hpp:766 */
	float quat_tran_ratio;	 /* [1000.0] utility.hpp:773 */
	int32_t reserved1;
	double t_limit;			 /* [2.0] mulls_slam.cpp:177 inter_submap_t_limit (the inner-submap loop passes 0.1, :179) */
	double r_limit;			 /* [0.05] mulls_slam.cpp:178 inter_submap_r_limit (inner-submap: 0.01, :180) */
	double function_tolerance; /* [1e-16] graph_optimizer.cpp:445 */
	float wrong_edge_translation_thre; /* [5.0] utility.hpp:776, mulls_slam.cpp:186 */
	float wrong_edge_rotation_thre;	   /* [25.0] degrees; mulls_slam.cpp:187 (utility.hpp:777 says 20) */
	float wrong_edge_ratio_thre;	   /* [0.1] utility.hpp:778 */
	uint32_t reserved2;
} mulls_pgo_params;
typedef struct mulls_pgo_result
{
	int32_t status;		 /* 1: solved (every stop); -1: too few edges; -2: the initial cost is not finite */
	int32_t termination; /* enum mulls_pgo_termination */
	int32_t iterations, successful_steps;
	uint32_t n_free, n_boxed, n_fixed, n_edges_used;
	double initial_cost, final_cost;
	int32_t wrong_edges, correct_reg_edges, edges_ok;
	int32_t reserved;
} mulls_pgo_result;
typedef struct mulls_pgo_problem
{
	const mulls_pgo_node *nodes;
	uint32_t n_nodes;
	const mulls_pgo_edge *edges;
	uint32_t n_edges;
	double *poses_out;	 /* 16 n_nodes, column-major */
	uint8_t *edge_wrong; /* n_edges, or NULL */
} mulls_pgo_problem;

void mulls_pgo_default_params(mulls_pgo_params *p);
/* One problem; a batch of one.  NULL ctx / params / result, NULL nodes with n_nodes > 0, NULL edges with n_edges > 0 or NULL poses_out with n_nodes > 0:
 * MULLS_E_INVALID with the result untouched.  MULLS_E_INVALID for a non-finite pose, T or info, an edge index outside the nodes, a == b, an edge type outside enum mulls_pgo_edge_type, num_iterations
 * outside 0 .. 1000, a negative or non-finite limit, tolerance, delta, ratio or threshold; MULLS_E_UNSUPPORTED above the capacity.  On either nothing is written to the
 * result, poses_out or edge_wrong.  n_nodes = 0: MULLS_OK, a zeroed result with status 1 and termination NO_FREE. */
int mulls_pgo_optimize(mulls_ctx *ctx, const mulls_pgo_node *nodes, uint32_t n_nodes, const mulls_pgo_edge *edges, uint32_t n_edges,
					   const mulls_pgo_params *params, double *poses_out, uint8_t *edge_wrong, mulls_pgo_result *result);
/* Many independent problems per call: the inner-submap loop of mulls_slam.cpp:876-926.  results[b], problems[b].poses_out and .edge_wrong are THE BITS THE
 * SINGLE CALL RETURNS for problem b, whatever its neighbours, its position and the sub-batches.  Every problem is checked before any device work; the first
 * offending problem's index is named in mulls_last_error and nothing is written for any problem.  The problems iterate in lock step, one launch set and
 * one 4-byte readback (the number of problems still running) per iteration; a stopped problem is skipped with its record frozen.
 * scratch_limit_bytes: the device memory one sub-batch may take; a problem larger than the limit runs alone.  0: MULLS_PGO_BATCH_DEFAULT_SCRATCH_BYTES.
 * n_problems = 0: MULLS_OK. */
int mulls_pgo_optimize_batch(mulls_ctx *ctx, const mulls_pgo_problem *problems, uint32_t n_problems, const mulls_pgo_params *params,
							 uint64_t scratch_limit_bytes, mulls_pgo_result *results);

/* ---- the submap archive: cloudblock_t submaps kept in device memory, their bounds, and loop closure's candidate edges ----
 * What test/mulls_slam.cpp does with cblock_submaps between judge_new_submap and the registration of a loop-closure edge: the deep copy of the local map
 * into a new submap (:454, utility.hpp:327-345), update_optimized_nodes (src/graph_optimizer.cpp:778-798) after a pose graph optimisation, and
 * Constraint_Finder::find_overlap_registration_constraint (src/build_pose_graph.cpp:123-209).  Lines marked [upstream] follow the reference's code, [LIB]
 * are this library's; PCL and FLANN are not available where this library is built and tested, and what is said of them is restated from memory and was
 * compared with neither.  tests/submaps_restated.py restates the bounds, the overlap search and the pairs in numpy; DESIGN.md section 7.7 has the reasons.
 *   storage    [LIB] one arena of capacity_points 48-byte records, allocated by mulls_submaps_create and never moved: a mulls_cloud handed out by
 *              mulls_submaps_cloud stays valid until mulls_submaps_clear or mulls_submaps_destroy.  A submap's records are contiguous, in the order of
 *              cloudblock_t::merge_feature_points(pc, false) (utility.hpp:471-482): ground, facade, pillar, beam, roof, vertex.  The six class clouds, the
 *              merged cloud and the merged cloud without ground are slices of that one range.
 *   capacity   [LIB] mulls_mapper_add's rule: a push that does not fit, in points or in submaps, returns MULLS_E_UNSUPPORTED, leaves the store as it was,
 *              and info reports n[], points_needed and submaps_needed (what the store would have held).
 *   bounds     [upstream utility.hpp:817-847] CloudUtility::get_cloud_bbx: min starts at DBL_MAX and is replaced when min > v, max starts at -DBL_MAX and
 *              is replaced when max < v, v the float coordinate widened to double.  So a NaN never wins, +inf never becomes a minimum, -inf never a
 *              maximum, and an axis nothing wins keeps (DBL_MAX, -DBL_MAX).  Both bounds are {min_x, min_y, min_z, max_x, max_y, max_z}.
 *              local_bound: over the submap's records as stored.  bound: over the same points moved by pose_lo as pcl::transformPointCloud with a
 *              Matrix4d does: (float)(((m00 x + m01 y) + m02 z) + m03) in double, no contraction, per row.  A minimum and a maximum are exact in any order:
 *              nothing depends on the job size or on which workgroup runs first, and a batched call returns the bits of single calls.
 *   vertex NMS [upstream mulls_slam.cpp:462] vertex_nms_radius > 0: the stored vertex cloud is, byte for byte, mulls_non_max_suppress's output for the given
 *              cloud at that radius on its default path (below its gate of 10 points: the cloud as given).  [LIB] that entry point runs inside the push
 *              and its refusals are the push's; its kept records pass through host memory on their way into the arena.  0: stored as given.
 *              A negative or non-finite radius: MULLS_E_INVALID.
 *   overlap    mulls_submaps_find_overlap, blocks = submaps 0 .. query_id, cur = query_id.
 *              [upstream :127] query_id + 1 < adjacent_id_thre + 2: no edges.
 *              [upstream :139-152] centres: pose_lo's translation cast to float; x, y (search_2d) or x, y, z.
 *              [LIB / FLANN L2_Simple from memory] d2 = 0.0f + dx dx + dy dy (+ dz dz), float, left to right, dx = query - history; a neighbour needs
 *              d2 < r2 strictly with r2 = (float)((double)r * (double)r) (mulls_non_max_suppress's rule); neighbours are ordered by (d2, id) ascending; the first max_neighbor are
 *              kept, max_neighbor <= 0 keeps all.  A NaN d2 is no neighbour.
 *              [upstream :571-590] iou = calculate_iou(bound of cur, bound of the neighbour), literally in double with max_(a, b) = a > b ? a : b and
 *              min_(a, b) = a < b ? a : b; an empty box gives NaN or 0 under IEEE rules and passes no threshold >= 0.
 *              [upstream :560-569] adjacent iff id_cur <= id_nb + thre && id_cur >= id_nb - thre on id_in_strip.
 *              [upstream :190] kept iff !adjacent && iou > (double)min_iou_thre.
 *              [upstream :204 / LIB] sorted by iou descending; ties keep the neighbour order (upstream's std::sort leaves them unspecified).
 *              [LIB] Trans1_2 = inverse(pose_tgt) * pose_src with the general 4 x 4 inverse of this library's host algebra (row-pivoted LU, hostmath.h) and
 *              its 4 x 4 product (each entry 0.0 + four products in ascending inner index); upstream's Eigen inverse cannot be pinned here.
 *   refused    [LIB] NULL arguments, a store of another context, a cloud with points and no address, a stride under 48 or not a multiple of 4, an id or
 *              `which` out of range, a non-finite search radius or IoU threshold: MULLS_E_INVALID, checked on the host before anything is launched.
 * A store belongs to its context: mulls_destroy(ctx) also destroys the stores still alive. */
#define MULLS_SUBMAP_CHUNK 1024u /* records of one submap per bounds job (one workgroup) */
#define MULLS_SUBMAP_MERGED 6	 /* `which` of mulls_submaps_cloud / _download: all six classes in merge order */
#define MULLS_SUBMAP_MERGED_NO_GROUND 7 /* ... facade, pillar, beam, roof, vertex */
typedef struct mulls_submaps mulls_submaps;
typedef struct mulls_submap_info
{
	uint32_t n[MULLS_NCLASS]; /* class sizes as stored, in the ABI's class order (enum mulls_class) */
	int32_t id_in_strip;
	uint32_t submaps_needed;  /* submaps the store holds after the push (or would have held) */
	uint64_t offset;		  /* the submap's first record in the arena */
	uint64_t points_needed;	  /* records the store holds after the push (or would have held) */
	double pose_lo[16];		  /* column-major */
	double local_bound[6];
	double bound[6];
} mulls_submap_info;
typedef struct mulls_overlap_params /* build_pose_graph.h:43-44 */
{
	float neighbor_search_dist; /* [50.0] */
	float min_iou_thre;			/* [0.25] */
	int32_t adjacent_id_thre;	/* [3] */
	int32_t search_2d;			/* [1] */
	int32_t max_neighbor;		/* [10] */
	int32_t reserved;
} mulls_overlap_params;
typedef struct mulls_submap_edge /* constraint_t as find_overlap_registration_constraint fills it; con_type is REGISTRATION */
{
	int32_t tgt_id; /* block1: the history submap */
	int32_t src_id; /* block2: the query submap */
	double overlapping_ratio;
	double Trans1_2[16]; /* column-major */
} mulls_submap_edge;

void mulls_overlap_default_params(mulls_overlap_params *p);
int mulls_submaps_create(mulls_ctx *ctx, uint32_t capacity_points /* <= 2^30 */, uint32_t capacity_submaps /* <= 2^16 */, mulls_submaps **out);
void mulls_submaps_destroy(mulls_ctx *ctx, mulls_submaps *store);
/* clouds: the six class clouds in the ABI's class order; each host memory or device memory (a cloud of the library's or any device allocation of the
 * caller's, told apart as mulls_scan_prepare does), at any stride that is a multiple of 4 and at least 48.  Returns MULLS_OK, the new submap's id being
 * info->submaps_needed - 1. */
int mulls_submaps_push(mulls_ctx *ctx, mulls_submaps *store, const mulls_cloud clouds[MULLS_NCLASS], const double pose_lo[16], int32_t id_in_strip,
					   float vertex_nms_radius, mulls_submap_info *info);
/* the local map's six clouds and pose_lo, device to device: the bytes mulls_map_download returns.  local_bound and bound are the last mulls_map_update's
 * report; a map that was set and never updated has none, and with vertex_nms_radius > 0 the report no longer describes what is stored: they are then taken
 * from the stored records. */
int mulls_submaps_push_map(mulls_ctx *ctx, mulls_submaps *store, const mulls_map *map, int32_t id_in_strip, float vertex_nms_radius, mulls_submap_info *info);
int mulls_submaps_count(mulls_ctx *ctx, const mulls_submaps *store, uint32_t *n_submaps, uint64_t *n_points);
int mulls_submaps_info(mulls_ctx *ctx, const mulls_submaps *store, uint32_t id, mulls_submap_info *info);
/* which: enum mulls_class, MULLS_SUBMAP_MERGED or MULLS_SUBMAP_MERGED_NO_GROUND; a device-resident cloud (stride 48) for every entry point that takes one */
int mulls_submaps_cloud(mulls_ctx *ctx, const mulls_submaps *store, uint32_t id, int which, mulls_cloud *out);
/* at most cap records to host memory; *n: the cloud's size (pts NULL with cap 0: the size query) */
int mulls_submaps_download(mulls_ctx *ctx, const mulls_submaps *store, uint32_t id, int which, void *pts, uint32_t cap, uint32_t *n);
int mulls_submaps_clear(mulls_ctx *ctx, mulls_submaps *store);
/* update_optimized_nodes (graph_optimizer.cpp:778-798): pose_lo of submaps first .. first + n - 1 becomes poses[16 k ..], column-major; with update_bbx
 * their `bound` is taken again.  One upload of the poses, one launch set over jobs of MULLS_SUBMAP_CHUNK records for all n submaps, one download of 6 n
 * doubles.  first + n beyond the count: MULLS_E_INVALID, nothing changed.  n = 0: MULLS_OK. */
int mulls_submaps_set_poses(mulls_ctx *ctx, mulls_submaps *store, uint32_t first, uint32_t n, const double *poses, int update_bbx);
/* edges: at most cap of them, in output order; *n_edges: the full count */
int mulls_submaps_find_overlap(mulls_ctx *ctx, const mulls_submaps *store, uint32_t query_id, const mulls_overlap_params *params, mulls_submap_edge *edges,
							   uint32_t cap, uint32_t *n_edges);
/* pairs[k] for mulls_icp_batch from edges[k]: tgt = the history submap's class clouds, src = the query's (use_more_points), src_down zero,
 * tgt_bound = the history submap's local_bound, init_guess = Trans1_2 */
int mulls_submaps_pairs(mulls_ctx *ctx, const mulls_submaps *store, const mulls_submap_edge *edges, uint32_t n, mulls_pair *pairs);

/* ---- NDT registration: CRegistration::omp_ndt (cregistration.hpp:945-1021) with base_align (:762-785), koide_reg::NormalDistributionsTransform
 * (baseline_reg/ndt_omp_impl.hpp), koide_reg::VoxelGridCovariance::applyFilter and getNeighborhoodAtPoint{1,7,} (voxel_grid_covariance_omp_impl.hpp:44-443)
 * and pcl::Registration::getFitnessScore.  The yardstick is a numpy restatement written from reading those files (tests/ndt_restated.py); NOTHING WAS
 * COMPARED WITH ndt_omp OR PCL THEMSELVES (PCL is not a dependency of this repository).  [upstream]: kept as upstream has it; [LIB]: defined here.
 *
 * Pre-steps [upstream, omp_ndt]  tgt = block1->pc_down, src = block2->pc_down.  The guess counts as identity when Eigen's isIdentity(1e-6) says so
 *   (|g_ii - 1| <= 1e-6 min(|g_ii|, 1), |g_ij| <= 1e-6).  Otherwise every source point becomes float(((g00 x + g01 y) + g02 z) + g03), .. in double
 *   (pcl::transformPointCloudWithNormals with a Matrix4d), src_bound is replaced by the box of the moved source, and T = T_ndt * guess at the end.
 *   box = {max(tgt_bound.min, src_bound.min) - 2, min(tgt_bound.max, src_bound.max) + 2} (get_intersection_bbx); with apply_intersection_filter both
 *   clouds keep, in order, the points with min < (double)coordinate < max on the three axes.  NDT itself starts from p = 0.
 *   [LIB] a cloud that is empty after the crop: no registration runs, T = guess (or identity), fitness = DBL_MAX, code = -3, converged = 0.
 * Grid [upstream]  inv = 1.0f / resolution (float); min_p, max_p: float minimum and maximum of the cropped target; min_b = (int)floorf(min_p * inv),
 *   max_b likewise, div_b = max_b - min_b + 1; cell of a point: (int)(floorf(x * inv) - (float)min_b.x), ..; index = i + j div_b.x + k div_b.x div_b.y.
 *   ((int64)((max_p.x - min_p.x) * inv) + 1) (..y) (..z) > INT32_MAX: MULLS_E_UNSUPPORTED (upstream warns and leaves an empty grid); [LIB] the same
 *   when div_b.x div_b.y div_b.z > INT32_MAX (upstream's int index overflows).  Per leaf, in double, points added in input order: n, the sum s of the
 *   points, the sum q of their outer products.  mean = s / n.  n >= min_points_per_voxel: the lower triangle of the covariance, element (b, a) =
 *   ((q_ab - 2 (s_b mean_a)) / n + mean_b mean_a) * ((n - 1.0) / n); eigenvalues e0 <= e1 <= e2 and vectors [LIB] by the cyclic Jacobi rotations of
 *   csrc/jacobi_rot.h (pairs (0,1) (0,2) (1,2), at most 60 sweeps, until the squared off-diagonal sum is below 1e-300); e0 < 0 or e1 < 0 or e2 <= 0:
 *   the leaf is disabled (n = -1).  e0 < m = min_covar_eigvalue_mult e2: e0 = m, then e1 = m if e1 < m, and the covariance becomes [LIB] V diag(e) V^T,
 *   element (a, b) = ((v_a0 e0) v_b0 + (v_a1 e1) v_b1) + (v_a2 e2) v_b2.  icov [LIB] by cofactors over the determinant ((c00 k00 + c01 k01) + c02 k02);
 *   an infinite element disables the leaf.  The leaves are found through a hash table keyed by the cell index; no dense table of the grid exists.
 * Score constants [upstream]  c1 = 10 (1 - outlier_ratio), c2 = outlier_ratio / pow(resolution, 3), d3 = -log(c2), d1 = -log(c1 + c2) - d3,
 *   d2 = -2 log((-log(c1 exp(-0.5) + c2) - d3) / d1), by the host's C library.
 * Neighbourhood [upstream] of a transformed point (a float): ijk = (int)floorf(x / resolution) (a division); the offsets in order — DIRECT1: (0,0,0);
 *   DIRECT7: (0,0,0) (1,0,0) (-1,0,0) (0,1,0) (0,-1,0) (0,0,1) (0,0,-1); DIRECT26: pcl::getAllNeighborCellIndices' 26 columns, i.e. the 13 of
 *   (i, j, -1) for i, j in -1 .. 1 (i outer), (i, -1, 0) for i in -1 .. 1, (-1, 0, 0), then their negatives in the same order (the centre is not among
 *   them).  An offset counts when min_b <= ijk + offset <= max_b on every axis and the cell has a leaf with n >= min_points_per_voxel.
 *   [LIB] a transformed coordinate that is not finite or beyond 2^30 cells has no neighbours.  MULLS_NDT_KDTREE (use_direct_search = false): MULLS_E_UNSUPPORTED.
 * One (point, leaf) term [LIB: in double throughout; upstream's float Matrix<float,4,6> intermediates and float exp are not reproduced]
 *   R, t of T(p) = Translation(p0 p1 p2) Rx(p3) Ry(p4) Rz(p5) in double with detmath.h's correctly rounded sin and cos; x' = float(((R_r0 x + R_r1 y)
 *   + R_r2 z) + t_r) (upstream stores the moved cloud in float), X = (double)x' - mean.  The vectors a .. h of equation 6.19 and a2 .. f3 of 6.21 as
 *   upstream writes them, with upstream's rule that an angle below 10e-5 counts as 0 there (not in T(p)).  Every 3-term dot product is (u0 v0 + u1 v1) + u2 v2.
 *   cX = C X, q = X . cX, e = exp_cr((-d2 q) / 2), score term -d1 e; E = d2 e; E > 1, E < 0 or NaN: the pair adds nothing; E = E d1.  J_k: the columns
 *   of the point Jacobian (unit vectors, then (0, x.a, x.b), (x.c, x.d, x.e), (x.f, x.g, x.h)); cJ_k = C J_k (column k of C for k < 3); g_k = X . cJ_k;
 *   gradient_k += E g_k; for i <= k: H_ik += E (((-d2 g_i) g_k + cX . h_ik) + J_k . cJ_i), the middle term only for i >= 3, J_k . cJ_i = (cJ_i)_k for k < 3.
 *   Only the upper triangle is accumulated; the Hessian is that triangle mirrored.
 * Sums [LIB]  a point's terms are added in offset order into 28 per-point sums starting from 0; the 28 sums over points: partial[l] = the sum over
 *   points l, l + MULLS_NDT_TREE, .. in that order, then for w = MULLS_NDT_TREE / 2 .. 1: partial[l] += partial[l + w], l < w.  The fitness sum likewise.
 * Newton loop [upstream :119-171]  with its quirks: converged when nr_iterations > max_iterations or (nr_iterations and |step| < transformation_epsilon);
 *   the return on a zero or NaN ||delta|| with converged = (norm == norm).  delta [LIB]: cyclic Jacobi eigen-decomposition of the Hessian in double
 *   (12 sweeps over the pairs (0,1) (0,2) .. (4,5); rotation as jacobi_rot.h's, the annihilated element set to 0), delta = -V diag(1/lambda) V^T g over
 *   the eigenvalues with |lambda| > 6 2^-52 max|lambda|; ||delta|| = sqrt of the squares added in order; direction = delta / ||delta||.
 * Line search [upstream :757-916, whole]  mu 1e-4, nu 0.9, at most max_step_iterations inner steps, step_max = step_size, step_min =
 *   transformation_epsilon / 2, the reversed direction, interval_converged = (step_max - step_min) > 0 as written (so with upstream's constants the inner
 *   loop never runs; it does with transformation_epsilon = 2 step_size), updateIntervalMT, trialValueSelectionMT, the extra Hessian only when the inner
 *   loop ran ([LIB] over the same direct neighbourhood: upstream's computeHessian searches its kd-tree of leaf centroids).
 * Results  T [LIB] = T(p) in double (upstream keeps a float matrix) times the guess; trans_probability = score / n_src [upstream]; fitness [upstream] =
 *   the mean over the cropped source of the float squared distance ((dx dx + dy dy) + dz dz) from x' under the final p to its nearest cropped target
 *   point; code = fitness > fitness_score_thre ? -3 : 1.  evaluations: evaluation passes, the Hessian-only ones included. */
enum mulls_ndt_search
{
	MULLS_NDT_KDTREE = 0, /* not built: MULLS_E_UNSUPPORTED */
	MULLS_NDT_DIRECT26 = 1,
	MULLS_NDT_DIRECT7 = 2,
	MULLS_NDT_DIRECT1 = 3
};
#define MULLS_NDT_TREE 4096u									/* width of the strided partial sums */
#define MULLS_NDT_BATCH_DEFAULT_SCRATCH_BYTES (1024ull << 20) /* a value chosen without a measurement */
#define MULLS_NDT_MAX_POINTS (1u << 24)						/* per cloud */
typedef struct mulls_ndt_params
{
	float resolution;				   /* 1.0 */
	int32_t search_method;			   /* MULLS_NDT_DIRECT7 */
	int32_t apply_intersection_filter; /* 1 */
	float fitness_score_thre;		   /* 10.0 */
	uint64_t scratch_limit_bytes;	   /* of one sub-batch of mulls_ndt_batch; 0: MULLS_NDT_BATCH_DEFAULT_SCRATCH_BYTES */
	/* upstream's constants */
	double step_size;				/* 0.1 */
	double transformation_epsilon; /* 0.1 */
	double outlier_ratio;			/* 0.55 */
	double min_covar_eigvalue_mult; /* 0.01 */
	int32_t max_iterations;			/* 35 */
	int32_t max_step_iterations;	/* 10 */
	int32_t min_points_per_voxel;	/* 6 */
	int32_t reserved;
} mulls_ndt_params;
typedef struct mulls_ndt_problem
{
	mulls_cloud tgt, src;	/* host or device memory, told apart as mulls_scan_prepare does; stride a multiple of 4, at least 12 */
	double tgt_bound[6];	/* block1->local_bound: min x y z, max x y z */
	double src_bound[6];	/* block2->local_bound (read only when the guess is identity) */
	double init_guess[16];	/* column-major */
} mulls_ndt_problem;
typedef struct mulls_ndt_result
{
	int32_t code; /* 1 or -3 */
	int32_t iterations, evaluations, converged;
	uint32_t n_leaves, n_leaves_used; /* cells with a point; leaves with n >= min_points_per_voxel that are not disabled */
	uint32_t n_src, n_tgt;			  /* after the crop */
	double T[16];					  /* column-major */
	double fitness, trans_probability;
	double gauss_d1, gauss_d2, gauss_d3;
	int32_t line_search_reversals, inner_steps; /* directions reversed; inner steps of all line searches */
} mulls_ndt_result;
void mulls_ndt_default_params(mulls_ndt_params *p);
/* MULLS_OK, or MULLS_E_INVALID (an empty cloud, a NULL pointer, a non-finite coordinate, bound or guess, a bad stride or parameter), MULLS_E_UNSUPPORTED
 * (MULLS_NDT_KDTREE, the grid refusals above, a cloud above MULLS_NDT_MAX_POINTS); the results are then not written. */
int mulls_ndt(mulls_ctx *ctx, const mulls_ndt_problem *problem, const mulls_ndt_params *params, mulls_ndt_result *result);
/* the bits of n_problems mulls_ndt calls.  The problems of a sub-batch run in lock step: a tick is one evaluation launch over the problems that still
 * run, one launch that advances every problem's Newton / line-search state, and one 4-byte readback; at most (max_iterations + 2) (max_step_iterations + 2)
 * + 1 ticks (the first evaluation, then per Newton iteration one trial, the inner steps and the Hessian pass).  Sub-batches are sized by params->scratch_limit_bytes; a problem larger than the limit runs alone.  n_problems = 0: MULLS_OK. */
int mulls_ndt_batch(mulls_ctx *ctx, const mulls_ndt_problem *problems, uint32_t n_problems, const mulls_ndt_params *params, mulls_ndt_result *results);

/* ---- Voxelised GICP registration: CRegistration::omp_gicp (cregistration.hpp:1024-1098) with using_voxel_gicp = true, the second base_align overload
 * (:788-815), koide_reg::FastVGICP (baseline_reg/fast_vgicp_impl.hpp, fast_vgicp_voxel.h, fast_gicp_utility.h) as upstream configures it
 * (k_correspondences 20, PLANE regularisation, ADDITIVE voxels, DIRECT1, the Sophus branch of computeTransformation) and
 * pcl::Registration::getFitnessScore.  The yardstick is a numpy restatement written from reading those files (tests/gicp_restated.py); NOTHING WAS
 * COMPARED WITH fast_gicp, Sophus, Eigen OR PCL THEMSELVES (none is a dependency of this repository).  [upstream]: kept as upstream has it; [LIB]:
 * defined here.  Every 3-term dot product is (u0 v0 + u1 v1) + u2 v2; sin and atan2 are detmath.h's correctly rounded ones; no contraction.
 *
 * Pre-steps [upstream, omp_gicp]  exactly mulls_ndt's (the same code runs): pc_down clouds, the isIdentity(1e-6) rule, the guess applied to the source
 *   in double and stored as float, get_intersection_bbx, the crop, T = T_gicp * guess at the end.  apply_intersection_filter defaults to 0 here (:1026).
 *   Quirk kept: with using_voxel_gicp = true upstream never reads max_iter_num and dis_thre_unit (:1071 is commented out, corr_dist_threshold_ is
 *   unused); the loop runs max_iterations = 64.  using_voxel_gicp = 0 (PCL's BFGS GICP): MULLS_E_UNSUPPORTED.
 *   [LIB] a cloud with fewer than k_correspondences points after the crop: no registration runs, T = guess (or identity), fitness = DBL_MAX,
 *   code = -3, converged = 0, stop = MULLS_GICP_STOP_NONE (upstream would read uninitialised columns of the neighbour matrix).
 * Neighbours [LIB order, upstream set]  of every point i of a cropped cloud: the k points of the same cloud, i itself among them, that are smallest by
 *   (float squared distance ((dx dx + dy dy) + dz dz), index) in lexicographic order.  FLANN's tie order is unknown and not claimed.
 * Point covariance [upstream shape, LIB arithmetic]  in double: m = the sum of the k neighbours in that order, divided by k; S = the sum, in that order,
 *   of the outer products of (p - m) (a scatter matrix: not divided); S is decomposed by the cyclic Jacobi rotations of csrc/jacobi_rot.h (pairs (0,1)
 *   (0,2) (1,2), at most 60 sweeps, until the squared off-diagonal sum is below 1e-300); eigenvalues descending, ties by column index ascending;
 *   C_ab = (v0_a v0_b + v1_a v1_b) + 0.01 (v2_a v2_b): PLANE, U diag(1, 1, 1e-2) V^T.  Upstream's JacobiSVD signs for a symmetric matrix are not
 *   reproduced.  Six doubles per point (xx xy xz yy yz zz).
 * Voxel map [upstream]  the coordinate of a float point is floorf(x / resolution - 0.5f) per axis, computed in float and cast to int (the -0.5 is
 *   upstream's and is kept).  [LIB] the key is three 21-bit fields of coordinate + 2^20; a coordinate outside [-2^20, 2^20), of a cropped target
 *   point in the voxel map or of a cropped point of either cloud in the neighbour search's cells of the same edge (floor(x (1 / edge)) in double):
 *   MULLS_E_UNSUPPORTED.  Per occupied voxel, in ascending point index and in
 *   double: n, the sum of the points, the sum of their C; mean = sum / n, cov = sum / n.  A voxel of one point is a voxel (upstream has no minimum).
 *   The map is an open-addressing hash table; no dense grid exists.
 * State and start [upstream]  x = (r, t), rotation vector and translation, from 0 (omp_gicp has applied the guess to the cloud).  Since |r| < 1e-2
 *   upstream sets r = Vector3f::Random().normalized() * 1e-2, an unseeded rand(); [LIB] r = params->start_rotvec.
 * Rotation [LIB]  in double.  exp(w): th = sqrt((w0^2 + w1^2) + w2^2); th == 0: I; else R_ij = (I_ij + a K_ij) + b K2_ij, K = skew(w), K2 = K K written
 *   out (diagonal -(w1 w1 + w2 w2), -(w0 w0 + w2 w2), -(w0 w0 + w1 w1); off-diagonal w_i w_j), a = sin_cr(th) / th, s = sin_cr(th / 2),
 *   b = ((2 s) s) / (th th).  log(R): w = ((R21 - R12) / 2, (R02 - R20) / 2, (R10 - R01) / 2), c = (((R00 + R11) + R22) - 1) / 2, n = |w| as above,
 *   th = atan2_cr(n, c); the result is w (th / n), or 0 when n == 0.  Rotations near pi are outside the definition.  csrc/gicp_math.h is this text.
 * One source point per iteration [upstream loss_ls, LIB double]  T = (exp(r), t); a'_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r, kept in double (upstream
 *   is float throughout; not reproduced).  The voxel of float(a') is looked up; with no voxel (or a coordinate out of range) the point adds nothing.
 *   RC = R C_A; the upper triangle of M = cov_B + RC R^T, mirrored; W = M^-1 by cofactors over the determinant ((m00 k00 + m01 k01) + m02 k02), as
 *   the NDT leaf's icov; d = mean_B - a', e = W d, J = [W skew(a'), -W] (3 x 6; column 0 of W skew(a') is W_i1 a'_2 - W_i2 a'_1, and cyclically).
 *   The point's 28 sums: the upper triangle of J^T J row by row (21), J^T e (6), e . e (1).  Over points: MULLS_NDT_TREE's strided-partial rule
 *   (lane l adds points l, l + MULLS_NDT_TREE, .. in order, then the halving tree).  n_corr = the points with a voxel.
 * Step [upstream GaussNewton::delta, LIB solve]  delta = (J^T J)^-1 J^T e by a 6 x 6 Cholesky in double, L by columns, every sum subtracted term by
 *   term in ascending index, then the two triangular solves.  [LIB] a pivot that is <= 0 or not finite, a non-finite delta or n_corr == 0 ends the
 *   loop: converged = 0, stop = MULLS_GICP_STOP_SINGULAR, the current x is kept (upstream takes a random step instead).  Update, a quirk kept:
 *   r = log(exp(-delta_r) exp(r)), t -= delta_t.  Converged, with iterations = i, when max(max|exp(delta_r) - I| / rotation_epsilon,
 *   max|delta_t| / transformation_epsilon) < 1.  After max_iterations steps without that: converged = 0, iterations = max_iterations - 1
 *   (upstream's nr_iterations_ = i), stop = MULLS_GICP_STOP_MAX_ITERATIONS.
 * Results  T = (exp(r), t) * guess in double.  fitness and code are mulls_ndt's fitness pass (the same kernels): the mean over the cropped source of
 *   the float squared distance from float(a') under the final x to the nearest cropped target point; code = fitness > fitness_score_thre ? -3 : 1.
 *   loss = the last evaluation's e . e sum, n_corr its count.
 * Not built: plain GICP (using_voxel_gicp = false); FastVGICP's DIRECT7 / DIRECT27, MULTIPLICATIVE / ADDITIVE_WEIGHTED voxels and the other
 *   regularisations (omp_gicp cannot select them); keeping a cloud's covariances between calls. */
enum mulls_gicp_stop
{
	MULLS_GICP_STOP_NONE = 0, /* no registration ran */
	MULLS_GICP_STOP_CONVERGED = 1,
	MULLS_GICP_STOP_MAX_ITERATIONS = 2,
	MULLS_GICP_STOP_SINGULAR = 3
};
#define MULLS_GICP_BATCH_DEFAULT_SCRATCH_BYTES (1024ull << 20) /* a value chosen without a measurement */
typedef struct mulls_gicp_params
{
	float voxel_resolution;			   /* 1.0 */
	int32_t k_correspondences;		   /* 20; 3 .. 32 */
	int32_t max_iterations;			   /* 64 */
	int32_t apply_intersection_filter; /* 0 */
	double rotation_epsilon;		   /* 2e-3 */
	double transformation_epsilon;	   /* 5e-4 */
	float fitness_score_thre;		   /* 10.0 */
	int32_t using_voxel_gicp;		   /* 1; 0: MULLS_E_UNSUPPORTED */
	float start_rotvec[3];			   /* 3 x 0.005773503f: the rotation vector the loop starts from */
	int32_t reserved;
	uint64_t scratch_limit_bytes; /* of one sub-batch of mulls_gicp_batch; 0: MULLS_GICP_BATCH_DEFAULT_SCRATCH_BYTES */
} mulls_gicp_params;
typedef mulls_ndt_problem mulls_gicp_problem; /* tgt, src, tgt_bound, src_bound, init_guess */
typedef struct mulls_gicp_result
{
	int32_t code; /* 1 or -3 */
	int32_t iterations, converged, stop; /* enum mulls_gicp_stop */
	uint32_t n_src, n_tgt; /* after the crop */
	uint32_t n_voxels, n_corr; /* occupied voxels; source points with a voxel at the last evaluation */
	double T[16];			   /* column-major */
	double fitness, loss;
} mulls_gicp_result;
void mulls_gicp_default_params(mulls_gicp_params *p);
/* MULLS_OK, or MULLS_E_INVALID (an empty cloud, a NULL pointer, a non-finite coordinate, bound or guess, a bad stride or parameter), MULLS_E_UNSUPPORTED
 * (using_voxel_gicp = 0, a coordinate beyond 2^20 voxels, a cloud above MULLS_NDT_MAX_POINTS); the results are then not written. */
int mulls_gicp(mulls_ctx *ctx, const mulls_gicp_problem *problem, const mulls_gicp_params *params, mulls_gicp_result *result);
/* the bits of n_problems mulls_gicp calls.  The covariances and voxel maps of a sub-batch are built in one launch set; then its problems run in lock
 * step: a tick is one evaluation launch over the problems that still run, one launch that solves and updates every problem, and one 4-byte readback;
 * at most max_iterations ticks.  Sub-batches are sized by params->scratch_limit_bytes; a problem larger than the limit runs alone.  n_problems = 0: MULLS_OK. */
int mulls_gicp_batch(mulls_ctx *ctx, const mulls_gicp_problem *problems, uint32_t n_problems, const mulls_gicp_params *params, mulls_gicp_result *results);

/* ---- Classical ICP registration: CRegistration::pcl_icp (cregistration.hpp:882-942) over icp_registration (:84-315), the part of it that is plain
 * ICP: pcl::IterativeClosestPoint / IterativeClosestPointWithNormals with nearest-neighbour correspondences within a distance, optionally reciprocal,
 * TransformationEstimationSVD or TransformationEstimationPointToPlaneLLS, DefaultConvergenceCriteria, get_pc_normal_pcar and
 * pcl::Registration::getFitnessScore.  NOTHING WAS COMPARED WITH PCL, FLANN OR EIGEN THEMSELVES (none is a dependency of this repository, and no PCL
 * source was at hand): the skeleton was read from cregistration.hpp and pca.hpp, and what PCL 1.8.1 does inside was restated FROM MEMORY; those
 * clauses say so.  The yardstick is a numpy restatement of this text (tests/pcl_icp_restated.py).  [upstream]: kept as upstream has it; [LIB]:
 * defined here.  Every 3-term dot product is (u0 v0 + u1 v1) + u2 v2; sin and cos are detmath.h's correctly rounded ones; no contraction.
 *
 * Pre-steps [upstream, pcl_icp]  exactly mulls_ndt's (the same code runs): pc_down clouds, the isIdentity(1e-6) rule, the guess applied to the source
 *   in double and stored as float, get_intersection_bbx, the crop, T = T_icp * guess at the end.  Quirk NOT kept: with an identity guess upstream never
 *   fills cloud_s_guess (:895-917), hands icp_registration an empty source and registers nothing (identity, fitness DBL_MAX, code -3); [LIB] with an
 *   identity guess the source is block2->pc_down itself.  [LIB] a cloud that is empty after the crop: no registration runs, T = guess (or identity),
 *   fitness = DBL_MAX, code = -3, converged = 0, stop = MULLS_PCL_ICP_STOP_NONE (mulls_ndt's rule).  max_iter_num and dis_thre_unit have no default
 *   upstream; [LIB] 20 and 1.5, mm_lls_icp's.  transformation_epsilon 1e-8 and euclidean_fitness_epsilon 1e-5 are the constants of :136-138.
 * d2 [upstream]  of two float points: dx = ax - bx, ..; ((dx dx + dy dy) + dz dz) in float.
 * Correspondences [upstream set, LIB tie order]  for the moved source point i, in ascending i: m = the cropped target point smallest by (d2, index);
 *   the pair is dropped when (double)d2 > (double)dis_thre_unit * (double)dis_thre_unit.  use_reciprocal_correspondence: i keeps its pair only if i
 *   is the smallest of all moved source points by (d2 to m, index).  No other rejector runs.  FLANN's tie order is unknown and not claimed.  Fewer
 *   than 3 pairs end the loop: converged = 0, stop = MULLS_PCL_ICP_STOP_NO_CORRESPONDENCES, the pose reached so far is kept.
 *   [LIB] the search walks hash tables of cubic cells (no dense grid) of edge dis_thre_unit (1 + 2^-20), cell = floor(x (1 / edge)) in double, and
 *   looks into the 27 cells around a point's own.  The margin makes the walk exact: a pair the float test accepts is apart by at most
 *   dis_thre_unit (1 + 2^-23) per axis, below one edge however the two products round.  The reciprocity test needs no unbounded search either: a
 *   source point that beats i at m lies within d(i, m) <= dis_thre_unit of m.  A coordinate of a cropped cloud outside [-2^20, 2^20) cells (of either
 *   edge, below): MULLS_E_UNSUPPORTED; a source point that leaves that range while it is moved takes no part in that iteration.
 * Sums [LIB]  over the pairs in ascending source index, in double: MULLS_NDT_TREE's strided-partial rule (lane l adds the pairs of the source points
 *   l, l + MULLS_NDT_TREE, .. in order, then the halving tree).
 * Point-to-point step [upstream shape: TransformationEstimationSVD, Umeyama without scale; from memory]  cs, ct = the sums of the paired moved source
 *   points and of their target points, each divided by the number of pairs; H_ab = the sum of (s_a - cs_a) (t_b - ct_b); R = the proper rotation that
 *   maximises trace(R H); t = ct - R cs.  [LIB] R by csrc/ransac_math.h's decomposition kept in double (Horn's symmetric 4 x 4, ten sweeps of cyclic
 *   Jacobi, the eigenvector of the largest diagonal entry as a unit quaternion); upstream's float JacobiSVD is not reproduced.
 * Point-to-plane step [upstream shape: TransformationEstimationPointToPlaneLLS; from memory]  per pair, with s the moved source point, t its target
 *   point and n the target point's normal as doubles: row = (s x n, n) with s x n = (s1 n2 - s2 n1, s2 n0 - s0 n2, s0 n1 - s1 n0), b = n . (t - s);
 *   the sums of row_i row_k for i <= k row by row (21) and of row_i b (6); x = (alpha, beta, gamma, tx, ty, tz) solves them.  [LIB] by
 *   csrc/gicp_math.h's 6 x 6 Cholesky; a pivot that is <= 0 or not finite or a non-finite x ends the loop: converged = 0, stop =
 *   MULLS_PCL_ICP_STOP_SINGULAR, the pose reached so far is kept.  R = Rz(gamma) Ry(beta) Rx(alpha), written out: R00 = cg cb, R01 = (-sg) ca +
 *   (cg sb) sa, R02 = sg sa + (cg sb) ca, R10 = sg cb, R11 = cg ca + (sg sb) sa, R12 = (-cg) sa + (sg sb) ca, R20 = -sb, R21 = cb sa, R22 = cb ca;
 *   the translation is (tx, ty, tz).  [LIB] a step of either kind with a non-finite element is SINGULAR as well.
 *   te selects nothing else: SVD or LLS under Point2Point both mean the first step, under Point2Plane both the second (upstream's default: branches).
 * Target normals (Point2Plane only) [upstream shape: get_pc_normal_pcar, NormalEstimationOMP with a radius, the viewpoint at the origin,
 *   check_normal; from memory]  the neighbourhood of a cropped target point p: every cropped target point q, p among them, with [LIB] (double)d2(q, p)
 *   <= (double)neighbor_radius * (double)neighbor_radius — a neighbour at exactly the radius counts; FLANN's rule there is not claimed.  Fewer than 3
 *   neighbours: the normal is (0.577f, 0.577f, 0.577f) (check_normal's value for PCL's NaN).  Otherwise [LIB] in double, the neighbours in ascending
 *   index, two passes as csrc/gicp_math.h's sum_add / mean_of / scatter_add: m = the sum / k, S = the sum of the outer products of (q - m); S by the
 *   cyclic Jacobi rotations of csrc/jacobi_rot.h (pairs (0,1) (0,2) (1,2), at most 60 sweeps, until the squared off-diagonal sum is below 1e-300);
 *   the column of the smallest diagonal entry, ties by the lower column index; divided by its norm; negated when n . (-p) < 0; stored as float
 *   ((0.577f, ..) if not finite).  The cells of this search have the edge neighbor_radius (1 + 2^-20).  Source normals are not computed: with
 *   ce = NN nothing reads them.
 * Loop [upstream: IterativeClosestPoint::computeTransformation and DefaultConvergenceCriteria; from memory]  an iteration takes the pairs of the moved
 *   source, estimates the step from them, moves the source in place, x <- float(((R_r0 x + R_r1 y) + R_r2 z) + t_r), composes final = step * final
 *   and counts the iteration.  Then, in this order: iterations >= max_iter_num: ITERATIONS; 0.5 (((R00 + R11) + R22) - 1) >= 1 -
 *   transformation_epsilon and (t0 t0 + t1 t1) + t2 t2 <= transformation_epsilon, of the step: TRANSFORM; with mse = the sum of the pairs' d2 (as
 *   recorded by the search, before the move) / the number of pairs: |mse - prev| < 1e-12: ABS_MSE; |mse - prev| / prev < euclidean_fitness_epsilon:
 *   REL_MSE; each of these with converged = 1.  prev starts at DBL_MAX and becomes mse when nothing fired.  [LIB] the step and the product are double
 *   (upstream's are float).  n_corr and mse are the last iteration's.
 * Fitness [upstream getFitnessScore(thre_dis), quirk kept]  the cropped source under the final pose, x' = float(((R_r0 x + R_r1 y) + R_r2 z) + t_r);
 *   d2 to the nearest cropped target point; a point counts when (double)d2 <= (double)dis_thre_unit — a squared distance against an unsquared range,
 *   as upstream has it; fitness = the sum over the counted points (the strided-partial rule) / n_fit, DBL_MAX when n_fit = 0; code = fitness >
 *   fitness_score_thre ? -3 : 1.
 * Not built (MULLS_E_UNSUPPORTED): use_trimmed_rejector (CorrespondenceRejectorVarTrimmed removes the distance bound: an unbounded search), te = LM,
 *   ce = NS (normal shooting), metrics = Plane2Plane (PCL's GICP). */
enum mulls_pcl_icp_metric
{
	MULLS_PCL_ICP_POINT2POINT = 0,
	MULLS_PCL_ICP_POINT2PLANE = 1,
	MULLS_PCL_ICP_PLANE2PLANE = 2 /* not built: MULLS_E_UNSUPPORTED */
};
enum mulls_pcl_icp_ce
{
	MULLS_PCL_ICP_NN = 0,
	MULLS_PCL_ICP_NS = 1 /* not built: MULLS_E_UNSUPPORTED */
};
enum mulls_pcl_icp_te
{
	MULLS_PCL_ICP_SVD = 0,
	MULLS_PCL_ICP_LM = 1, /* not built: MULLS_E_UNSUPPORTED */
	MULLS_PCL_ICP_LLS = 2
};
enum mulls_pcl_icp_stop
{
	MULLS_PCL_ICP_STOP_NONE = 0, /* no registration ran */
	MULLS_PCL_ICP_STOP_ITERATIONS = 1,
	MULLS_PCL_ICP_STOP_TRANSFORM = 2,
	MULLS_PCL_ICP_STOP_ABS_MSE = 3,
	MULLS_PCL_ICP_STOP_REL_MSE = 4,
	MULLS_PCL_ICP_STOP_NO_CORRESPONDENCES = 5,
	MULLS_PCL_ICP_STOP_SINGULAR = 6
};
#define MULLS_PCL_ICP_BATCH_DEFAULT_SCRATCH_BYTES (1024ull << 20) /* a value chosen without a measurement */
typedef struct mulls_pcl_icp_params
{
	int32_t max_iter_num;				   /* 20 [LIB] */
	float dis_thre_unit;				   /* 1.5 [LIB] */
	int32_t metrics;					   /* enum mulls_pcl_icp_metric; MULLS_PCL_ICP_POINT2POINT */
	int32_t ce;							   /* enum mulls_pcl_icp_ce; MULLS_PCL_ICP_NN */
	int32_t te;							   /* enum mulls_pcl_icp_te; MULLS_PCL_ICP_SVD */
	int32_t use_reciprocal_correspondence; /* 0 */
	int32_t use_trimmed_rejector;		   /* 0; 1: MULLS_E_UNSUPPORTED */
	float neighbor_radius;				   /* 2.0 */
	int32_t apply_intersection_filter;	   /* 1 */
	float fitness_score_thre;			   /* 10.0 */
	double transformation_epsilon;		   /* 1e-8 */
	double euclidean_fitness_epsilon;	   /* 1e-5 */
	uint64_t scratch_limit_bytes;		   /* of one sub-batch of mulls_pcl_icp_batch; 0: MULLS_PCL_ICP_BATCH_DEFAULT_SCRATCH_BYTES */
} mulls_pcl_icp_params;
typedef mulls_ndt_problem mulls_pcl_icp_problem; /* tgt, src, tgt_bound, src_bound, init_guess */
typedef struct mulls_pcl_icp_result
{
	int32_t code; /* 1 or -3 */
	int32_t iterations, converged, stop; /* enum mulls_pcl_icp_stop */
	uint32_t n_src, n_tgt; /* after the crop */
	uint32_t n_corr, n_fit; /* the last iteration's pairs; the source points the fitness counted */
	double mse;				/* of the last iteration's pairs */
	double T[16];			/* column-major */
	double fitness;
} mulls_pcl_icp_result;
void mulls_pcl_icp_default_params(mulls_pcl_icp_params *p);
/* MULLS_OK, or MULLS_E_INVALID (an empty cloud, a NULL pointer, a non-finite coordinate, bound or guess, a bad stride or parameter), MULLS_E_UNSUPPORTED
 * (the options above, a coordinate beyond 2^20 cells, a cloud above MULLS_NDT_MAX_POINTS); the results are then not written. */
int mulls_pcl_icp(mulls_ctx *ctx, const mulls_pcl_icp_problem *problem, const mulls_pcl_icp_params *params, mulls_pcl_icp_result *result);
/* the bits of n_problems mulls_pcl_icp calls.  The tables and normals of a sub-batch are built in one launch set; then its problems run in lock step:
 * a tick re-bins the moved sources (reciprocal only), searches, accumulates and decides for every problem that still runs, and reads 4 bytes back; at
 * most max_iter_num ticks.  Sub-batches are sized by params->scratch_limit_bytes; a problem larger than the limit runs alone.  n_problems = 0: MULLS_OK. */
int mulls_pcl_icp_batch(mulls_ctx *ctx, const mulls_pcl_icp_problem *problems, uint32_t n_problems, const mulls_pcl_icp_params *params,
						mulls_pcl_icp_result *results);

/* ---- FPFH descriptors and FPFH-based SAC-IA coarse registration: CRegistration::compute_fpfh_feature (cregistration.hpp:351-369) and
 * coarse_reg_fpfhsac (:372-406): pcl::FPFHEstimationOMP with a radius of 2.0 * search_radius over the records' own normals, and
 * pcl::SampleConsensusInitialAlignment with setCorrespondenceRandomness(15) and every other setting at its default.  NOTHING WAS COMPARED WITH PCL,
 * FLANN OR EIGEN THEMSELVES (none is a dependency of this repository, and no PCL source was at hand): the skeleton was read from cregistration.hpp,
 * and what PCL does inside (FPFHEstimation, computePairFeatures, SampleConsensusInitialAlignment::computeTransformation) was restated FROM MEMORY;
 * those clauses say so.  The yardstick is a numpy restatement of this text (tests/fpfh_restated.py).  [upstream shape, from memory]: kept as upstream
 * is remembered to have it; [LIB]: defined here.  Arithmetic is double on the float fields unless a clause says float; every 3-term product is
 * (u0 v0 + u1 v1) + u2 v2; u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0); atan2 is detmath.h's correctly rounded one; no contraction.
 *
 * Inputs  a cloud is host memory or device memory (a map's cloud, or any device pointer), told apart as mulls_scan_prepare does; the stride is a
 *   multiple of 4 and at least 28: the normals are the records' own, at bytes 16 .. 27, as upstream passes setInputNormals(input_cloud).  Nothing
 *   estimates normals here.
 * Neighbourhood [LIB]  r = 2.0f * search_radius.  The neighbourhood of p is every point q of the cloud, p included, with (double)d2(q, p) <= (double)r *
 *   (double)r, d2 the float ((dx dx + dy dy) + dz dz) — a neighbour at exactly the radius counts; FLANN's rule there is not claimed.  k = its size.
 *   The search walks the hash table of cubic cells of edge r (1 + 2^-20), cell = floor(x (1 / edge)) in double, and looks into the 27 cells around
 *   p's own; the margin makes the walk exact for the reason given for mulls_pcl_icp above.  A coordinate outside [-2^20, 2^20) cells:
 *   MULLS_E_UNSUPPORTED.  A cell that holds more than MULLS_FPFH_MAX_CELL_POINTS points: MULLS_E_UNSUPPORTED as well — the radius is then so large
 *   against the cloud that the work, quadratic in a cell's points, would hold the device for a long time.
 * Pair feature [upstream shape: computePairFeatures, from memory]  of p and a neighbour q that is not p itself (another record at p's position is a
 *   neighbour): dp = q - p, f4 = sqrt(dp . dp); f4 == 0: the pair adds nothing.  a1 = (n_p . dp) / f4, a2 = (n_q . dp) / f4.  PCL swaps the roles when
 *   acos|a1| > acos|a2|; [LIB] that is |a1| < |a2|.  Swapped: n1 = n_q, n2 = n_p, dp = -dp, f3 = -a2; else n1 = n_p, n2 = n_q, f3 = a1.  v = dp x n1;
 *   |v| = sqrt(v . v) == 0: the pair adds nothing; v = v / |v|, w = n1 x v, f2 = v . n2, f1 = atan2(w . n2, n1 . n2).
 * Bins [LIB: in double; upstream's float d_pi_ is not reproduced]  b1 = floor(11 ((f1 + pi) (1 / (2 pi)))), b2 = floor(11 ((f2 + 1) 0.5)), b3 =
 *   floor(11 ((f3 + 1) 0.5)), each clamped to 0 .. 10; pi = 0x1.921fb54442d18p+1.  A NaN feature: the pair adds nothing.
 * SPFH [LIB]  the pairs are counted per bin as integers, three times 11 counters a point, so the order of the neighbours cannot matter;
 *   spfh[b] = (float)(((double)count_b * 100.0) / (double)(k - 1)), all zero when k <= 1.  [upstream shape] the divisor is k - 1 even when pairs
 *   added nothing.
 * FPFH [upstream shape: weightPointSPFHSignature, from memory]  over the neighbours q of p with d2(q, p) != 0: acc[b] += (double)spfh_q[b] *
 *   (1.0 / (double)d2).  [LIB] the accumulators are double and the neighbours come in this order, which depends on the cloud and r alone: the 27
 *   cells around p's own, cell l = 9 (dz + 1) + 3 (dy + 1) + (dx + 1) for l = 0 .. 26, ascending index inside a cell.  Then per sub-histogram: s =
 *   the 11 accumulators added in bin order; hist[b] = (float)(acc[b] * (100.0 / s)) when s != 0, else 0.  A result that is not finite is stored as 0.
 *   hist is n x 33 floats: f1's 11 bins, then f2's, then f3's. */
#define MULLS_FPFH_MAX_CELL_POINTS 16384u /* points of one cell of edge r (1 + 2^-20) */
typedef struct mulls_fpfh_params
{
	float search_radius; /* 1.0 [LIB: upstream has no default]; the feature radius is 2.0 * search_radius, as upstream */
	int32_t reserved;
} mulls_fpfh_params;
void mulls_fpfh_default_params(mulls_fpfh_params *p);
/* hist: n x 33 floats, host or device memory; n_neighbours: n, host or device memory, may be NULL.  MULLS_OK, or MULLS_E_INVALID (an empty cloud, a
 * NULL pointer, a coordinate or normal that is not finite, a bad stride or radius), MULLS_E_UNSUPPORTED (a coordinate beyond 2^20 cells, a cell above MULLS_FPFH_MAX_CELL_POINTS, a cloud
 * above MULLS_NDT_MAX_POINTS); nothing is then written. */
int mulls_fpfh(mulls_ctx *ctx, const mulls_cloud *cloud, const mulls_fpfh_params *params, float *hist, uint32_t *n_neighbours);

/* SAC-IA [upstream shape: SampleConsensusInitialAlignment::computeTransformation, from memory]  both clouds' descriptors as above, then
 * max_iterations hypotheses, each from nr_samples = 3 source points and one similar target descriptor for each.
 * Draws [LIB; upstream uses rand()]  one std::mt19937(seed); index(n) = eng() % n.  Per iteration, the sample selection first: draw a source index
 *   index(n_src); reject it when it equals an already chosen one of this iteration or lies closer to one than min_sample_distance (the float
 *   sqrtf of d2); at the 3 n_src-th rejection in a row min_sample_distance is halved for the rest of the call and the count starts again; repeat
 *   until nr_samples are chosen.  Then one index(k_eff) per sample, k_eff = min(k_correspondences, n_tgt).  Nothing here depends on a device result:
 *   the host draws every iteration up front.
 * Similar features [LIB]  the k_eff nearest target descriptors of a sampled source descriptor by (d2, target index), d2 = the 33 float differences
 *   squared and added in bin order in float; the drawn rank picks one.  FLANN's order among equals is unknown and not claimed.
 * Model [LIB]  csrc/ransac_math.h's three-pair fit, as mulls_coarse_reg_ransac's hypotheses use it: a float 3 x 4.
 * Error of a hypothesis [upstream shape, quirk kept]  over all source points: x' = float(((R_r0 x + R_r1 y) + R_r2 z) + t_r) in double on the float
 *   model, e = the float d2 to the nearest target point; with thr = max_correspondence_distance, in double: MULLS_SACIA_TRUNCATED e <= thr ? e / thr
 *   : 1; MULLS_SACIA_HUBER e <= thr ? (0.5 e) e : (0.5 thr) (2 |e| - thr) — a squared distance against an unsquared range, as PCL has it.  The terms are
 *   summed by MULLS_NDT_TREE's strided-partial rule.  The lowest error wins, the first among equals; [LIB] an error that is NaN (e = inf under an infinite
 *   range gives inf / inf) comes after every number, NaNs among themselves by index.  UNDER THE DEFAULTS thr IS INFINITE, EVERY
 *   TERM IS e / inf = 0 AND HYPOTHESIS 0 WINS: upstream never sets a correspondence distance, and that is its call as remembered.  Set a finite
 *   max_correspondence_distance for a search that selects.
 * Fitness [upstream getFitnessScore()]  the mean float d2 of the source under T to its nearest target point, by the same summation rule.
 * Many clouds and many problems per call: mulls_compute_fpfh_batch and mulls_coarse_reg_fpfhsac_batch, below the single calls. */
enum mulls_sacia_error
{
	MULLS_SACIA_TRUNCATED = 0,
	MULLS_SACIA_HUBER = 1
};
typedef struct mulls_fpfhsac_params
{
	float search_radius;			   /* 1.0 [LIB]; as mulls_fpfh */
	int32_t nr_samples;				   /* 3 [PCL, from memory]; only 3 is built, anything else MULLS_E_UNSUPPORTED */
	int32_t k_correspondences;		   /* 15 [upstream: setCorrespondenceRandomness(15)]; 1 .. 64 */
	int32_t max_iterations;			   /* 10 [pcl::Registration's default, from memory]; at most 65536 */
	float min_sample_distance;		   /* 0 [PCL, from memory] */
	float max_correspondence_distance; /* +inf: upstream never sets it; see the quirk above.  Above 0 */
	int32_t error_function;			   /* enum mulls_sacia_error; MULLS_SACIA_TRUNCATED [PCL's default, from memory] */
	uint32_t seed;					   /* 0 [LIB] upstream uses rand() */
} mulls_fpfhsac_params;
typedef struct mulls_fpfhsac_result
{
	int32_t best_iteration, iterations;
	uint32_t n_src, n_tgt;
	double best_error, fitness;
	double T[16]; /* column-major; source to target */
} mulls_fpfhsac_result;
void mulls_fpfhsac_default_params(mulls_fpfhsac_params *p);
/* MULLS_OK, or MULLS_E_INVALID (n_src < 3, n_tgt = 0, a NULL pointer, a coordinate, normal or parameter that is not finite or out of its range, a
 * bad stride), MULLS_E_UNSUPPORTED (nr_samples other than 3, max_iterations above 65536, a coordinate beyond 2^20 cells, a cell above
 * MULLS_FPFH_MAX_CELL_POINTS, a cloud above MULLS_NDT_MAX_POINTS); the result is then not written.  Each cloud goes up once, as two packed copies
 * (coordinates, normals); both descriptor sets come from one launch set, during which the host draws the samples of a host source; the clouds'
 * refusals are read back before anything else is launched; then the similar features of all samples, all models, all hypotheses' errors, the
 * winner and its fitness, and one download of the result. */
int mulls_coarse_reg_fpfhsac(mulls_ctx *ctx, const mulls_cloud *tgt, const mulls_cloud *src, const mulls_fpfhsac_params *params, mulls_fpfhsac_result *result);

/* ---- many FPFH clouds and many SAC-IA problems per call: the candidate edges of one loop-closure event (test/mulls_slam.cpp:517-596 tries one query
 * submap against several candidates) by the way that needs nothing but points and normals, in front of mulls_icp_batch.
 * results[b] is THE BYTES THE SINGLE CALL RETURNS for (problems[b].tgt, problems[b].src, params) on the same context, and every cloud of the descriptor
 * batch gets the bits of its single descriptor call.  No arithmetic, order of summation, tie rule or draw is redefined; there is one params for the
 * whole call, seed included.  The device steps run for all problems of a sub-batch per launch: one launch set for the descriptors of all its distinct
 * clouds, one launch for the similar features of all samples (a wave per sample, which finds its problem in the sub-batch's table), one for all models,
 * then the hypotheses of all problems as one flat list in problem order, cut into consecutive stretches of at most MULLS_FPFH_HYP_CHUNK (1 024) slots
 * whose nearest-target distances fit the distance pool (a stretch may begin and end inside a problem; three launches a stretch), one pick launch with a
 * workgroup per problem, one nearest-target pass over the winners, and one download (addendum).  The draws run per problem on
 * the host, the problems side by side, while the descriptors run; a device source's packed coordinates come back with the heads and its draws follow.
 *   shared clouds  a cloud named by several problems of a sub-batch, as a source, a target or both (or by several entries of clouds[]), is staged once
 *                 and its descriptors are computed once per sub-batch.  Identity is (pts, n, stride), for host and device clouds alike.  No result
 *                 depends on it.
 *   whole call    checked before any device work and before anything is written: a NULL it needs, a problem or cloud the single call would refuse (by
 *                 the single call's own checks: n_src < 3, an empty cloud, a bad stride, a cloud above MULLS_NDT_MAX_POINTS, a refused parameter) make
 *                 the call return the single call's code and name the first such index in mulls_last_error ("problem 3: the source ...", "cloud 2
 *                 ..."; a refused parameter refuses problem 0).
 *   device refusals  a coordinate or normal that is not finite, a coordinate beyond 2^20 cells, a cell above MULLS_FPFH_MAX_CELL_POINTS: read from the
 *                 sub-batch's heads before anything else is launched for it; the call returns the single call's code and names the first problem (or
 *                 cloud) that uses the refused cloud.  NO OUTPUT OF THE CALL IS WRITTEN, earlier sub-batches' included: results are kept on the host
 *                 and copied out after the last sub-batch succeeded.  The descriptor batch, whose outputs may be device memory: when the limit
 *                 cuts it into several sub-batches, a first pass runs every sub-batch and reads its heads only, and when all are good a second pass
 *                 computes them again and copies out; a call of one sub-batch reads its heads and copies out of the arena.
 *   scratch_limit_bytes  bounds the device arena of a sub-batch.  Counted per cloud of n points: cloud(n) = 4 up256(12 n) + 2 up256(132 n) +
 *                 3 up256(4 n) + 20 slots(n) + 1024 (coordinates and normals as given and in cell order, SPFH and FPFH, neighbourhood sizes, slots and
 *                 lists, the cell table of slots(n) = the power of two >= max(2 n, 1024), its table entries; up256 rounds up to 256 bytes).  Per
 *                 problem: cloud(n_src) + cloud(n_tgt) + 140 max_iterations + 1280 + 2 up256(4 n_src) + 4096 (samples, ranks, correspondences,
 *                 frames and errors; the winner's distances and one hypothesis of the distance pool; its table entries), and 2 MiB per sub-batch for
 *                 the slots of a stretch.  A shared cloud is counted for every problem that names it, so the arena is never larger than counted.  The
 *                 batch is cut into consecutive sub-batches that fit, of at most MULLS_FPFH_HYP_CHUNK problems (4 096 clouds); a problem larger than
 *                 the limit runs alone.  The distance pool (4 n_src bytes per hypothesis) is what the limit leaves, at most the 256 MB the single call
 *                 allows itself and what all hypotheses need, and at least one hypothesis of the sub-batch's largest source.
 *                 0: MULLS_FPFHSAC_BATCH_DEFAULT_SCRATCH_BYTES, a value chosen without a measurement.
 * n_problems = 0, n_clouds = 0: MULLS_OK, nothing is touched. */
#define MULLS_FPFHSAC_BATCH_DEFAULT_SCRATCH_BYTES (1024ull << 20)
/* hist[c]: clouds[c].n x 33 floats; n_neighbours: NULL, or n_neighbours[c] NULL or clouds[c].n entries; host or device memory each */
int mulls_compute_fpfh_batch(mulls_ctx *ctx, const mulls_cloud *clouds, uint32_t n_clouds, const mulls_fpfh_params *params, float *const *hist,
							 uint32_t *const *n_neighbours, uint64_t scratch_limit_bytes);
typedef struct mulls_fpfhsac_problem
{
	mulls_cloud tgt, src; /* host or device-resident clouds, by the single call's rules */
} mulls_fpfhsac_problem;
int mulls_coarse_reg_fpfhsac_batch(mulls_ctx *ctx, const mulls_fpfhsac_problem *problems, uint32_t n_problems, const mulls_fpfhsac_params *params,
								   uint64_t scratch_limit_bytes, mulls_fpfhsac_result *results);

/* ---- stage-level entry points (used by the parity tests; same kernels the driver launches) ---- */

/* batch_transform_feature_points (cregistration.hpp:1685-1696): in place on a host cloud via the device kernel */
int mulls_stage_transform(mulls_ctx *ctx, void *pts, uint32_t n, uint32_t stride, const double T[16]);

/* determine_corres (cregistration.hpp:1701-1835) on already-transformed clouds.
 * Outputs, each sized n_src: match[s] = target index or -1, d2[s] = squared NN distance (float),
 * flags[s] bit0 = survives compaction (always 1 when n_src < 500), bit1 = final correspondence. */
int mulls_stage_correspond(mulls_ctx *ctx, const mulls_cloud *src, const mulls_cloud *tgt, float dis_thre,
						   int normal_check, float angle_thre_degree, int32_t *match, float *d2, uint8_t *flags);

/* one class' contribution to ATPA (21 packed upper/lower terms, row-major-upper enumeration) and ATPb (6):
 * metric 0 = pt2pl (:2066-2156), 1 = pt2li (:2160-2275), 2 = pt2pt (:1976-2063).  out27 = 21 + 6 doubles;
 * weight_out[k] (may be NULL) = value the reference leaves in pcl::Correspondence::weight. */
int mulls_stage_accumulate(mulls_ctx *ctx, int metric, const mulls_cloud *src, const mulls_cloud *tgt,
						   const int32_t *corr_src, const int32_t *corr_tgt, const float *corr_d2, uint32_t ncorr,
						   int iter_num, float class_weight, int dist_w, int resid_w, int inten_w, float window,
						   double *out27, float *weight_out);

#ifdef __cplusplus
}
#endif
#endif /* MULLS_HIP_H */
