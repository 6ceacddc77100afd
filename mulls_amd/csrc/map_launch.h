// map_launch.h — host-callable launchers of map_kernels.hip (the segmented compaction) and k_map_batch.hip (device-resident local map)
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

// one class cloud of 48-B records for the multi-cloud kernels (blockIdx.x = slot)
struct MapCloudArg
{
	const float4 *in; // 3 float4 per record
	float4 *out;
	const uint8_t *mask; // compaction by mask (mode 0); unused otherwise
	uint32_t n;
	uint32_t pad_;
};
struct MapCompactArgs
{
	MapCloudArg cloud[6];
	uint32_t *out_n; // [6]
	int mode;		 // 0 = keep where mask != 0; 1 = CFilter::dist_filter(cloud, radius) (cfilter.hpp:834-871)
	double radius;
};

// seg_scratch: device array of at least map_compact_segments(a) uint32 (one counter per 4096-record segment)
uint32_t map_compact_segments(const MapCompactArgs &a);
void launch_map_compact(hipStream_t st, const MapCompactArgs &a, uint32_t *seg_scratch);
// the same three steps for `count` sets of clouds in one launch each (mulls_extract_features_batch): a table in device memory, one entry per set (blockIdx.y),
// every set with its own segment scratch; tab_host: the table's host copy.  Returns the kernels launched.
struct MapCompactJob
{
	MapCompactArgs a;
	uint32_t *seg;
};
int launch_map_compact_batch(hipStream_t st, const MapCompactJob *tab_dev, const MapCompactJob *tab_host, uint32_t count);
#define MAP_NN_CHUNK 2048u // tree points per workgroup (a down-sampled frame against a 20 000-point map: 16384 made 8 workgroups of it, 284 us; 2048: ~40 workgroups)

// PCA refresh of a linear-feature cloud (MapManager::update_cloud_vectors): writes direction / linearity into the records of
// the points it keeps and keep[i] = 0/1 for every point; max_k <= 24.  An entry of launch_mapb_pca's table.
struct MapPcaArgs
{
	float4 *recs;
	uint32_t n;
	float radius;
	int max_k, min_k;
	float sin_low, sin_high, min_linearity;
	uint8_t *keep;
};

// ---- the local map's kernels (k_map_batch.hip), table-driven: one launch per step for every map of a lock-step group (mulls_map_update: a group of one) ----
// A launch reads an entry table (one entry per cloud taking part) and a flat job list (one job per workgroup: which entry, which block of it), both in device
// memory and both built on the host from the sizes it knows at every phase; the grid is the job list's length, whatever the largest cloud is.
struct MapbCopyEnt // byte range to copy; bytes a multiple of 4; job = 16 KiB block of it
{
	unsigned long long dst, src;
	uint32_t bytes, pad_;
};
struct MapbXformEnt // job = 256 records
{
	float4 *recs;
	uint32_t n, pad_;
	double T[12]; // rows of [R|t]
};
// one frame class cloud against its tree (dynamic removal); jobs: (frame block of 256, tree chunk of MAP_NN_CHUNK) and (frame block of 256).  best[i] = float
// bits of the smallest squared distance to a tree point (0x7f800000 if there is none); tree = map class cloud, with use_box restricted to the open box (strict
// inequalities, float vs double)
struct MapbRemEnt
{
	const float4 *frame, *tree;
	uint32_t *best;
	uint8_t *keep;
	uint32_t n_frame, n_tree;
	int use_box;
	float center_radius, dmin, dmax, near_;
	uint32_t pad_;
	double box[6];
};
struct MapbBoxEnt // job = MAPB_BOX_TILE records
{
	const float4 *recs;
	uint32_t *keys; // the map's 12-word block
	uint32_t n, pad_;
	double pose[12];
};
#define MAPB_BOX_TILE 2048u
#define MAPB_COPY_BLOCK 16384u
struct MapbJob
{
	uint32_t ent, block, chunk, pad_;
};
// every launcher: nothing is launched for an empty job list; returns the kernels launched
int launch_mapb_copy(hipStream_t st, const MapbCopyEnt *ent, const MapbJob *jobs, uint32_t n_jobs);
int launch_mapb_transform(hipStream_t st, const MapbXformEnt *ent, const MapbJob *jobs, uint32_t n_jobs);
int launch_mapb_fill_best(hipStream_t st, const MapbRemEnt *ent, const MapbJob *jobs, uint32_t n_jobs); // best[q] = 0x7f800000
int launch_mapb_nn(hipStream_t st, const MapbRemEnt *ent, const MapbJob *jobs, uint32_t n_jobs);
int launch_mapb_keep(hipStream_t st, const MapbRemEnt *ent, const MapbJob *jobs, uint32_t n_jobs);
int launch_mapb_bbox(hipStream_t st, const MapbBoxEnt *ent, const MapbJob *jobs, uint32_t n_jobs);
int launch_mapb_pca(hipStream_t st, const MapPcaArgs *ent, const MapbJob *jobs, uint32_t n_jobs); // job = tile of 256 points
