// k_nms.hip — CFilter::non_max_suppress (cfilter.hpp:1183-1312) of a key-point cloud for gfx950, the path for the sizes the real workload has (a few
// thousand key points): the whole suppression in ONE workgroup of 1024 lanes on one CU, with workgroup barriers where the multi-launch path
// (k_cl_nms_* in k_classify.hip) has launches and host polls.
//   k_nms_keys   normal[3] of every record of a device cloud, and the non-finite flag
//   k_nms_batch_keys, k_nms_batch_gather, k_nms_batch    mulls_non_max_suppress_batch: the keys of all device-resident clouds of a sub-batch, their
//                records in visiting order, and the suppression of every problem with one workgroup each (nms_suppress, the body k_nms_one runs), in
//                one launch each.  Alone one workgroup loses to the multi-launch path; B clouds on B CUs cost what one costs (profiles/nms_batch.txt)
//   k_nms_one    records in visiting order -> kept positions, kept records (nms_suppress):
//                  stage    x, y, z as three float arrays in LDS, a state byte per point (0 suppressed, 1 kept, 2 undecided)
//                  cells    a hashed grid in LDS, cell edge a hair above the radius: bucket of every point (the cell's three integer-valued doubles,
//                           hashed into H = the power of two >= n buckets), counts, their scan, the points' positions in bucket order (a counting sort)
//                  lists    lane t owns points t, t + 1024, ...: it walks the 27 buckets around each of its points and writes the first
//                           MULLS_NMS_LIST_CAP earlier neighbours within the radius into the point's list in LDS, [slot][point] as 16-bit positions.
//                           The owner is the only writer: no atomics.  Two of the 27 cells may share a bucket, and a bucket holds other cells' points too:
//                           the distance test sorts those out, and an entry that appears twice changes nothing in what follows.
//                  rounds   an undecided point with a kept earlier neighbour is suppressed, one whose earlier neighbours are all suppressed is kept,
//                           the others wait.  States only move from 2 to 0 or 1 and a decision taken on decided neighbours is final, so lanes may
//                           read states other lanes write in the same round: one barrier per round, which also counts who is left.  The first
//                           undecided point of the order always decides: at most n rounds, and the loop is bounded by n.
//                           A point with more earlier neighbours than the list holds (a dense cluster of key points) walks its 27 buckets again in
//                           each round it is still undecided in.
//                  compact  stable, 1024 positions at a time: ballot ranks within a wavefront, the wavefronts' counts through LDS
// Why lists in LDS, found through a grid in LDS: the rounds are a chain of dependent steps, as long as the deepest suppression chain of the cloud; each step
// should cost a barrier and a handful of LDS reads, not a trip to the L2.  And one CU cannot afford all pairs: the first version of this kernel walked every
// predecessor of every point (8 M distance tests at 4096 points) and took 0.9 - 1.8 ms.  With the grid it takes 0.52 - 0.73 ms (profiles/nms_kernel_stats.txt),
// which still loses to the multi-launch path's 0.20 - 0.25 ms per call: a walk is about 80 divergent trips of some 60 instructions, four wavefronts share a
// SIMD, and the demo clouds' dense clusters overflow the 8-slot list and walk again in every round (0.5 ms of rounds against 0.16 ms of lists at 2840
// points).  So nms.cpp's own choice (path 0) is the multi-launch path, and this kernel runs on request (path 1).
// The grid is exact: the cell is floor(x / edge) in double with edge = |r| (1 + 1e-5), so two points whose float d2 is below r2 (their true distance is then
// below |r| (1 + 1e-6)) are in cells that differ by at most one along each axis.  Where the quotient is beyond 2^53 neighbouring cells collapse into one
// value, and so do the coordinates themselves: a bucket is then walked more than once, no neighbour is missed.
// Every loop's trip count is bounded by a launch argument: n, the bucket count, or a bucket's size (<= n).  The distance is (dx dx + dy dy) + dz dz in
// float, built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>

#include "launch.h"
#include "nms_launch.h"

namespace
{
__global__ __launch_bounds__(256) void k_nms_keys(const float4 *__restrict__ recs, uint32_t n, float *__restrict__ keys, uint32_t *__restrict__ bad)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n)
		return;
	const float4 r0 = recs[(size_t)i * 3];
	keys[i] = recs[(size_t)i * 3 + 1].w;
	if (!(isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z)))
		atomicOr(bad, 1u);
}

// bucket of the cell (cx, cy, cz): integer-valued doubles (any magnitude), hashed
__device__ __forceinline__ uint32_t nms_axis(double c)
{
	const unsigned long long u = (unsigned long long)__double_as_longlong(c);
	return (uint32_t)(u ^ (u >> 32));
}
__device__ __forceinline__ uint32_t nms_bucket(uint32_t hx, uint32_t hy, uint32_t hz, uint32_t mask)
{
	uint32_t h = (hx * 0x9E3779B1u) ^ (hy * 0x85EBCA77u) ^ (hz * 0xC2B2AE3Du);
	h ^= h >> 15;
	h *= 0x2C1B3C6Du;
	h ^= h >> 12;
	return h & mask;
}
__device__ __forceinline__ double nms_cell(float x, double inv_edge)
{
	const double c = floor((double)x * inv_edge);
	return c == 0.0 ? 0.0 : c; // one zero: -0.0 and +0.0 have different bits
}

struct NmsLds // the dynamic LDS of k_nms_one, carved for n points and H buckets (nms_lds_bytes in nms_launch.h counts the same arrays)
{
	float *sx, *sy, *sz;
	uint32_t *start; // [H + 1] after the counting sort: start[b] = end of bucket b = beginning of bucket b + 1
	uint16_t *list;	 // [MULLS_NMS_LIST_CAP][n]; before the lists are written its first n entries hold the points' buckets
	uint16_t *sidx;	 // [n] positions in bucket order
	uint8_t *state, *fill;
};

// The earlier neighbours of point p: every q < p within the radius whose state is not `skip_state`, through visit(q); stops when visit returns false.
template <class Visit>
__device__ __forceinline__ void nms_walk(const NmsLds &L, uint32_t p, float r2, double inv_edge, uint32_t mask, const Visit &visit)
{
	const float x = L.sx[p], y = L.sy[p], z = L.sz[p];
	const double cx = nms_cell(x, inv_edge), cy = nms_cell(y, inv_edge), cz = nms_cell(z, inv_edge);
	uint32_t hx[3], hy[3], hz[3];
#pragma unroll
	for (int d = 0; d < 3; d++)
	{
		hx[d] = nms_axis(cx + (double)(d - 1));
		hy[d] = nms_axis(cy + (double)(d - 1));
		hz[d] = nms_axis(cz + (double)(d - 1));
	}
	// One loop over "the next entry of this bucket, or else the next bucket": a wavefront then runs as long as its busiest lane has entries and buckets
	// together, not 27 times as long as the fullest bucket any lane meets.  At most 27 + the 27 buckets' sizes trips: bounded by 27 (n + 1).
	uint32_t prev = 0xffffffffu, k = 0, k1 = 0;
	for (int c = -1;;)
	{
		if (k < k1)
		{
			const uint32_t q = L.sidx[k++];
			if (q >= p)
				continue;
			const float dx = x - L.sx[q], dy = y - L.sy[q], dz = z - L.sz[q];
			if (dx * dx + dy * dy + dz * dz < r2)
				if (!visit(q))
					return;
			continue;
		}
		if (++c >= 27)
			return;
		const uint32_t b = nms_bucket(hx[c % 3], hy[(c / 3) % 3], hz[c / 9], mask);
		if (b == prev)
			continue;
		prev = b;
		k = b ? L.start[b - 1] : 0u;
		k1 = L.start[b];
	}
}

// The whole suppression of one cloud by one workgroup of MULLS_NMS_BLOCK lanes: the one text of the staging, the cells, the lists, the rounds and the
// compaction, for k_nms_one (the single call's path 1) and k_nms_batch (one workgroup per problem).  nms_lds: nms_lds_bytes(n) bytes of LDS at least;
// wsum: MULLS_NMS_BLOCK / 64 words of LDS.  Returns the kept count (the same in every lane); *rounds_out: the rounds run.
__device__ __forceinline__ uint32_t nms_suppress(const float4 *__restrict__ recs, uint32_t n, uint32_t H, float r2, double inv_edge, uint32_t *__restrict__ kept_pos,
												  float4 *__restrict__ out, uint32_t out_cap, unsigned char *nms_lds, uint32_t *wsum, uint32_t *rounds_out)
{
	NmsLds L;
	L.sx = reinterpret_cast<float *>(nms_lds), L.sy = L.sx + n, L.sz = L.sy + n;
	L.start = reinterpret_cast<uint32_t *>(L.sz + n);
	L.list = reinterpret_cast<uint16_t *>(L.start + H + 1u);
	L.sidx = L.list + (size_t)MULLS_NMS_LIST_CAP * n;
	L.state = reinterpret_cast<uint8_t *>(L.sidx + n), L.fill = L.state + n;
	uint8_t *state = L.state;
	const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6, mask = H - 1u;

	for (uint32_t p = t; p < n; p += MULLS_NMS_BLOCK)
	{
		const float4 r0 = recs[(size_t)p * 3];
		L.sx[p] = r0.x, L.sy[p] = r0.y, L.sz[p] = r0.z;
		state[p] = 2;
		L.fill[p] = 0;
	}
	for (uint32_t b = t; b <= H; b += MULLS_NMS_BLOCK)
		L.start[b] = 0u;
	__syncthreads();

	if (r2 > 0.f) // (radius 0: nothing is within it, every point is kept in the first round)
	{
		// cells: the counting sort of the points by bucket
		uint16_t *bkt = L.list;
		for (uint32_t p = t; p < n; p += MULLS_NMS_BLOCK)
		{
			const uint32_t b = nms_bucket(nms_axis(nms_cell(L.sx[p], inv_edge)), nms_axis(nms_cell(L.sy[p], inv_edge)), nms_axis(nms_cell(L.sz[p], inv_edge)), mask);
			bkt[p] = (uint16_t)b;
			atomicAdd(&L.start[b], 1u);
		}
		__syncthreads();
		// exclusive scan of the H counts: `per` consecutive buckets per lane, the lanes' sums through the wavefronts
		const uint32_t per = (H + MULLS_NMS_BLOCK - 1u) / MULLS_NMS_BLOCK, b0 = t * per;
		uint32_t mine = 0;
		for (uint32_t i = 0; i < per; i++)
			mine += b0 + i < H ? L.start[b0 + i] : 0u;
		uint32_t inc = mine;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1)
		{
			const uint32_t o = __shfl_up(inc, d, 64);
			if (lane >= (uint32_t)d)
				inc += o;
		}
		if (lane == 63u)
			wsum[w] = inc;
		__syncthreads();
		uint32_t run = inc - mine;
		for (uint32_t v = 0; v < w; v++)
			run += wsum[v];
		for (uint32_t i = 0; i < per; i++)
			if (b0 + i < H)
			{
				const uint32_t c = L.start[b0 + i];
				L.start[b0 + i] = run;
				run += c;
			}
		__syncthreads();
		// scatter: the bucket's beginning is its cursor, and ends as its end
		for (uint32_t p = t; p < n; p += MULLS_NMS_BLOCK)
			L.sidx[atomicAdd(&L.start[bkt[p]], 1u)] = (uint16_t)p;
		__syncthreads();

		// lists: the earlier neighbours of the lane's own points
		for (uint32_t p = t; p < n; p += MULLS_NMS_BLOCK)
		{
			uint32_t cnt = 0;
			nms_walk(L, p, r2, inv_edge, mask, [&](uint32_t q) {
				if (cnt < MULLS_NMS_LIST_CAP)
					L.list[(size_t)cnt * n + p] = (uint16_t)q;
				cnt++;
				return cnt <= MULLS_NMS_LIST_CAP; // one past the list: it does not fit, the rounds will walk the buckets
			});
			L.fill[p] = (uint8_t)cnt;
		}
		__syncthreads();
	}

	// rounds
	uint32_t rounds = 0;
	for (uint32_t r = 0; r < n; r++)
	{
		int undecided = 0;
		for (uint32_t p = t; p < n; p += MULLS_NMS_BLOCK)
		{
			if (state[p] != 2)
				continue;
			const uint32_t cnt = L.fill[p];
			bool kept_near = false, wait = false;
			if (cnt <= MULLS_NMS_LIST_CAP)
				for (uint32_t k = 0; k < cnt; k++)
				{
					const uint8_t s = state[L.list[(size_t)k * n + p]];
					kept_near |= s == 1;
					wait |= s == 2;
				}
			else
				nms_walk(L, p, r2, inv_edge, mask, [&](uint32_t q) {
					const uint8_t s = state[q];
					kept_near |= s == 1;
					wait |= s == 2;
					return !kept_near;
				});
			if (kept_near)
				state[p] = 0;
			else if (!wait)
				state[p] = 1;
			else
				undecided = 1;
		}
		rounds = r + 1u;
		if (__syncthreads_count(undecided) == 0)
			break;
	}

	// stable compaction of the kept positions, and the kept records
	uint32_t n_kept = 0;
	for (uint32_t base = 0; base < n; base += MULLS_NMS_BLOCK)
	{
		const uint32_t p = base + t;
		const bool k = p < n && state[p] == 1;
		const unsigned long long b = __ballot(k);
		if (lane == 0)
			wsum[w] = (uint32_t)__popcll(b);
		__syncthreads();
		uint32_t before = 0, all = 0;
		for (uint32_t v = 0; v < MULLS_NMS_BLOCK / 64u; v++)
		{
			const uint32_t c = wsum[v];
			before += v < w ? c : 0u;
			all += c;
		}
		if (k)
		{
			const uint32_t at = n_kept + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
			kept_pos[at] = p;
			if (out && at < out_cap)
			{
				out[(size_t)at * 3] = recs[(size_t)p * 3];
				out[(size_t)at * 3 + 1] = recs[(size_t)p * 3 + 1];
				out[(size_t)at * 3 + 2] = recs[(size_t)p * 3 + 2];
			}
		}
		n_kept += all;
		__syncthreads();
	}
	*rounds_out = rounds;
	return n_kept;
}

__global__ __launch_bounds__(MULLS_NMS_BLOCK) void k_nms_one(const float4 *__restrict__ recs, uint32_t n, uint32_t H, float r2, double inv_edge,
															  NmsHeader *__restrict__ hdr, uint32_t *__restrict__ kept_pos, float4 *__restrict__ out, uint32_t out_cap)
{
	extern __shared__ unsigned char nms_lds[];
	__shared__ uint32_t wsum[MULLS_NMS_BLOCK / 64u];
	uint32_t rounds;
	const uint32_t n_kept = nms_suppress(recs, n, H, r2, inv_edge, kept_pos, out, out_cap, nms_lds, wsum, &rounds);
	if (threadIdx.x == 0)
	{
		hdr->n_kept = n_kept;
		hdr->rounds = rounds;
	}
}

// ---- mulls_non_max_suppress_batch (nms_batch.h has the arena's layout).  Every trip count below is bounded by a value of a record the host validated
// and wrote: a cloud's n (<= MULLS_NMS_MAX_POINTS; <= MULLS_NMS_LDS_MAX_POINTS where a workgroup holds it), the count of cloud records, the kept count (<= n).
template <class T>
__device__ __forceinline__ T *at(unsigned char *arena, uint64_t off)
{
	return reinterpret_cast<T *>(arena + off);
}
// the cloud whose blocks hold `block`: first[c] <= block < first[c + 1]; first[0] = 0, first[count] = the grid
__device__ __forceinline__ uint32_t nms_find_cloud(const uint32_t *__restrict__ first, uint32_t count, uint32_t block)
{
	uint32_t lo = 0, hi = count;
	while (hi - lo > 1u)
	{
		const uint32_t mid = (lo + hi) >> 1;
		if (first[mid] <= block)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// keys and non-finite flags of every device-resident cloud of a sub-batch: a block of 256 lanes belongs to one cloud
__global__ __launch_bounds__(256) void k_nms_batch_keys(unsigned char *__restrict__ arena, uint64_t o_src, uint64_t o_blk, uint32_t n_src, uint64_t o_bad)
{
	const uint32_t c = nms_find_cloud(at<uint32_t>(arena, o_blk), n_src, blockIdx.x);
	const NmsBatchSrc S = at<NmsBatchSrc>(arena, o_src)[c];
	const uint32_t i = (blockIdx.x - S.blk) * 256u + threadIdx.x;
	if (i >= S.n)
		return;
	const float4 *recs = reinterpret_cast<const float4 *>(S.src);
	const float4 r0 = recs[(size_t)i * 3];
	at<float>(arena, S.keys)[i] = recs[(size_t)i * 3 + 1].w;
	if (!(isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z)))
		atomicOr(at<uint32_t>(arena, o_bad) + c, 1u);
}

// the records of the first n_src device-resident clouds in visiting order: recs[i] = src[perm[i]] (perm: the host's permutation of 0 .. n - 1)
__global__ __launch_bounds__(256) void k_nms_batch_gather(unsigned char *__restrict__ arena, uint64_t o_src, uint64_t o_blk, uint32_t n_src)
{
	const uint32_t c = nms_find_cloud(at<uint32_t>(arena, o_blk), n_src, blockIdx.x);
	const NmsBatchSrc S = at<NmsBatchSrc>(arena, o_src)[c];
	const uint32_t i = (blockIdx.x - S.blk) * 256u + threadIdx.x;
	if (i >= S.n)
		return;
	const uint32_t j = at<uint32_t>(arena, S.perm)[i];
	if (j >= S.n) // (never: the host sorted 0 .. n - 1)
		return;
	const float4 *src = reinterpret_cast<const float4 *>(S.src);
	float4 *dst = at<float4>(arena, S.recs);
	dst[(size_t)i * 3] = src[(size_t)j * 3];
	dst[(size_t)i * 3 + 1] = src[(size_t)j * 3 + 1];
	dst[(size_t)i * 3 + 2] = src[(size_t)j * 3 + 2];
}

// one workgroup per problem: problem blockIdx.x of the sub-batch's records.  The kept records go to the sub-batch's one compact region: the
// workgroup reserves min(n_kept, out_cap) records at the cursor (the order of the ranges is the order of arrival; the header says where the range is).
__global__ __launch_bounds__(MULLS_NMS_BLOCK) void k_nms_batch(unsigned char *__restrict__ arena, uint64_t o_desc, float r2, double inv_edge, uint64_t o_cursor,
																uint64_t o_out)
{
	extern __shared__ unsigned char nms_lds[];
	__shared__ uint32_t wsum[MULLS_NMS_BLOCK / 64u];
	__shared__ uint32_t out_at;
	const NmsBatchDesc D = at<NmsBatchDesc>(arena, o_desc)[blockIdx.x];
	const float4 *recs = at<float4>(arena, D.recs);
	uint32_t *kept_pos = at<uint32_t>(arena, D.kept);
	uint32_t rounds;
	const uint32_t n_kept = nms_suppress(recs, D.n, D.H, r2, inv_edge, kept_pos, nullptr, 0u, nms_lds, wsum, &rounds);
	const uint32_t n_rec = n_kept < D.out_cap ? n_kept : D.out_cap;
	if (threadIdx.x == 0)
	{
		out_at = atomicAdd(at<uint32_t>(arena, o_cursor), n_rec);
		NmsBatchHeader *hdr = at<NmsBatchHeader>(arena, D.hdr);
		hdr->n_kept = n_kept, hdr->rounds = rounds, hdr->out_at = out_at, hdr->pad = 0u;
	}
	__syncthreads(); // (the kept positions were written before the compaction's last barrier)
	float4 *out = at<float4>(arena, o_out) + (size_t)out_at * 3;
	for (uint32_t k = threadIdx.x; k < n_rec * 3u; k += MULLS_NMS_BLOCK)
		out[k] = recs[(size_t)kept_pos[k / 3u] * 3 + k % 3u];
}
} // namespace

hipError_t launch_nms_keys(hipStream_t st, const void *recs, uint32_t n, float *keys, uint32_t *bad)
{
	if (n)
		hipLaunchKernelGGL(k_nms_keys, dim3((n + 255u) / 256u), dim3(256), 0, st, static_cast<const float4 *>(recs), n, keys, bad);
	return hipGetLastError();
}

namespace
{
// per device (launch.h: DevLaunch): the one-workgroup kernels may take the whole LDS of a CU
bool nms_dev_ready()
{
	const DevLaunch D = dev_launch<4>([](DevLaunch &) {
		return hipFuncSetAttribute(reinterpret_cast<const void *>(k_nms_one), hipFuncAttributeMaxDynamicSharedMemorySize,
								   (int)nms_lds_bytes(MULLS_NMS_LDS_MAX_POINTS)) == hipSuccess &&
			   hipFuncSetAttribute(reinterpret_cast<const void *>(k_nms_batch), hipFuncAttributeMaxDynamicSharedMemorySize,
								   (int)nms_lds_bytes(MULLS_NMS_LDS_MAX_POINTS)) == hipSuccess;
	});
	return D.ok;
}
// r2 and the reciprocal cell edge of a radius
void nms_radius_args(float radius, float *r2, double *inv_edge)
{
	*r2 = (float)((double)radius * (double)radius);
	const double edge = std::fabs((double)radius) * (1.0 + 1e-5);
	// the grid's exactness rests on d2's relative rounding error; an r2 near the subnormal range has none to speak of: one cell then (inv_edge 0), all pairs
	*inv_edge = *r2 >= 1e-30f ? 1.0 / edge : 0.0;
}
} // namespace

hipError_t launch_nms_one(hipStream_t st, const float4 *recs, uint32_t n, float radius, NmsHeader *hdr, uint32_t *kept_pos, float4 *out, uint32_t out_cap)
{
	if (n == 0 || n > MULLS_NMS_LDS_MAX_POINTS)
		return hipErrorInvalidValue;
	if (!nms_dev_ready())
		return hipErrorInvalidValue;
	float r2;
	double inv_edge;
	nms_radius_args(radius, &r2, &inv_edge);
	hipLaunchKernelGGL(k_nms_one, dim3(1), dim3(MULLS_NMS_BLOCK), nms_lds_bytes(n), st, recs, n, nms_buckets(n), r2, inv_edge, hdr, kept_pos, out, out_cap);
	return hipGetLastError();
}

hipError_t launch_nms_batch_keys(hipStream_t st, unsigned char *arena, const NmsBatchLayout &L)
{
	const uint32_t n_src = (uint32_t)L.src.size();
	if (n_src && L.blk[n_src])
		hipLaunchKernelGGL(k_nms_batch_keys, dim3(L.blk[n_src]), dim3(256), 0, st, arena, L.o_src, L.o_blk, n_src, L.o_bad);
	return hipGetLastError();
}

hipError_t launch_nms_batch_gather(hipStream_t st, unsigned char *arena, const NmsBatchLayout &L)
{
	if (L.n_gather && L.gather_blk)
		hipLaunchKernelGGL(k_nms_batch_gather, dim3(L.gather_blk), dim3(256), 0, st, arena, L.o_src, L.o_blk, L.n_gather);
	return hipGetLastError();
}

hipError_t launch_nms_batch(hipStream_t st, unsigned char *arena, const NmsBatchLayout &L, float radius)
{
	const uint32_t B = (uint32_t)L.desc.size();
	if (!B)
		return hipSuccess;
	if (L.n_max > MULLS_NMS_LDS_MAX_POINTS || B > MULLS_NMS_BATCH_MAX_PROBLEMS || !nms_dev_ready())
		return hipErrorInvalidValue;
	float r2;
	double inv_edge;
	nms_radius_args(radius, &r2, &inv_edge);
	// Dynamic LDS is one size per launch: the largest cloud's.  Measured against a launch per size class (the clouds that fit half a CU's LDS first, so that
	// two of their workgroups share a CU whatever else the batch holds; profiles/nms_batch.txt): 448 clouds of 1024 points with 64 of 4096 take 6.28 ms this
	// way and 6.50 ms as two launches, which run one after the other; a batch of small clouds alone has a small launch either way.
	hipLaunchKernelGGL(k_nms_batch, dim3(B), dim3(MULLS_NMS_BLOCK), nms_lds_bytes(L.n_max), st, arena, L.o_desc, r2, inv_edge, L.o_cursor, L.o_out);
	return hipGetLastError();
}
