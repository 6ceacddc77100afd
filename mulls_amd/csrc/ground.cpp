// ground.cpp — what the ground stage of the feature chain (extract_batch.cpp) decides on the host: parameter defaults and checks, PCL's sample table for
// normal method 3, which points of cloud_ground make cloud_ground_down (every ground_random_down_down_rate-th point, or the ABI's seeded fixed-number
// selection: cfilter.hpp:1955-1968); CFilter::voxel_downsample (mulls_voxel_downsample, and vox_run for the chain); the device-resident feature blocks.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/mulls_hip.h"
#include "ctx.h"
#include "device_types.h"
#include "map_launch.h"

#include "classify_launch.h"
#include "extract_batch.h"
#include "extract_internal.h"
#include "ground_launch.h"

using mulls_ex::GfArena;
using mulls_ex::gf_layout;

extern "C"
{
	void mulls_ground_default_params(mulls_ground_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		// extract_semantic_pts' defaults (cfilter.hpp:2296-2316) where it has them, the flag defaults of test/mulls_slam.cpp otherwise;
		// normal method 0 / distance-inverse sampling 0: the deterministic skeleton (see the header)
		p->min_grid_pt_num = 8;
		p->grid_resolution = 3.0f;
		p->max_height_difference = 0.3f;
		p->neighbor_height_diff = 1.5f;
		p->max_ground_height = 2.0f;
		p->ground_random_down_rate = 10;
		p->ground_random_down_down_rate = 2;
		p->nonground_random_down_rate = 3;
		p->reliable_neighbor_grid_num_thre = 0;
		p->estimate_ground_normal_method = 0;
		p->distance_weight_downsampling_method = 0;
		p->standard_distance = 15.0f;
		p->fixed_num_downsampling = 0;
		p->apply_grid_wise_outlier_filter = 0;
		p->down_ground_fixed_num = 500;
		p->intensity_thre = 3.402823466e+38f;
		p->outlier_std_scale = 3.0f;
		p->normal_estimation_radius = 2.0f;
		p->rng_seed = 0;
	}

	// ---- shared with extract_batch.cpp ------------------------------------------------------------------------------------------------------
	MULLS_HIDDEN int gf_check(mulls_ctx *ctx, const mulls_ground_params *P, uint32_t n)
	{
		if (P->estimate_ground_normal_method < 0 || P->estimate_ground_normal_method > 3)
		{
			ctx->err = "mulls_ground_filter: estimate_ground_normal_method must be 0 .. 3";
			return MULLS_E_INVALID;
		}
		if (P->estimate_ground_normal_method == 1 && !(P->normal_estimation_radius > 0.0f))
		{
			ctx->err = "mulls_ground_filter: normal method 1 needs a positive normal_estimation_radius";
			return MULLS_E_INVALID;
		}
		if (P->estimate_ground_normal_method == 2 && 2 * (long)P->min_grid_pt_num > 64)
		{
			ctx->err = "mulls_ground_filter: normal method 2 searches 2 * min_grid_pt_num neighbours, at most 64";
			return MULLS_E_UNSUPPORTED;
		}
		if (P->min_grid_pt_num < 1 || !(P->grid_resolution > 0.0f) || P->ground_random_down_rate < 1 || P->ground_random_down_down_rate < 1 ||
			P->nonground_random_down_rate < 1 || P->distance_weight_downsampling_method < 0 || P->distance_weight_downsampling_method > 2)
		{
			ctx->err = "mulls_ground_filter: min_grid_pt_num, grid_resolution and the down-sampling rates must be positive";
			return MULLS_E_INVALID;
		}
		if (n > 500000u)
		{
			ctx->err = "mulls_ground_filter: more than 500000 points in one scan";
			return MULLS_E_UNSUPPORTED;
		}
		return MULLS_OK;
	}
	// PCL's sample sequence for the plane RANSAC of normal method 3: SACSegmentation(random = false) seeds boost::mt19937 with 12345u for every
	// model and draws through boost::uniform_int<>(0, INT_MAX), i.e. output / 2 — the same draws for every grid cell, so one table serves all
	MULLS_HIDDEN int gf_rnd_table(mulls_ctx *ctx)
	{
		if (ctx->gf_rnd)
			return MULLS_OK;
		std::vector<uint32_t> t(MULLS_GF_RND);
		std::mt19937 eng(12345u);
		for (uint32_t &v : t)
			v = (uint32_t)(eng() >> 1);
		HIPCHK(ctx, hipMalloc(&ctx->gf_rnd, t.size() * sizeof(uint32_t)));
		HIPCHK(ctx, hipMemcpy(ctx->gf_rnd, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
		return MULLS_OK;
	}
	// CFilter::voxel_downsample (cfilter.hpp:83-160) on the n records at `in` (device): pc_down is gathered to `down` (device, room for n records),
	// *n_down = its size.  Bounding box and voxel indices come from the device; the order of the (voxel, index) pairs is std::sort's on the host,
	// as upstream's is: which point of a voxel comes first is decided by that sort (the comparison sees the voxel only, :42), and it depends on
	// nothing but the indices' values and their count, so the same sort over the same indices picks the same points.  The stream is idle afterwards.
	// base: the ground arena `a` lays out (its voxel keys and order are the scratch).
	MULLS_HIDDEN int vox_run(mulls_ctx *ctx, unsigned char *base, const GfArena &a, const float4 *in, uint32_t n, float voxel_size, float4 *down, uint32_t *n_down)
	{
		hipStream_t st = ctx->stream;
		unsigned long long *keys = reinterpret_cast<unsigned long long *>(base + a.o_keys);
		uint32_t *box = reinterpret_cast<uint32_t *>(base + a.o_keys + (size_t)n * 8);
		uint32_t *perm = reinterpret_cast<uint32_t *>(base + a.o_perm);
		*n_down = 0;
		if (n == 0)
			return MULLS_OK;
		uint32_t hb[7];
		if (launch_vox_bbox(st, in, n, box) != 0)
		{
			ctx->err = "mulls_voxel_downsample: launch failed";
			return MULLS_E_HIP;
		}
		HIPCHK(ctx, hipMemcpyAsync(hb, box, sizeof(hb), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		if (hb[6])
		{
			ctx->err = "mulls_voxel_downsample: non-finite coordinate";
			return MULLS_E_INVALID;
		}
		float min_p[3], max_p[3];
		for (int k = 0; k < 3; k++)
		{
			const uint32_t lo = hb[k], hi = hb[3 + k]; // ordered keys back to floats
			const uint32_t ul = (lo & 0x80000000u) ? (lo & 0x7fffffffu) : ~lo, uh = (hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi;
			std::memcpy(&min_p[k], &ul, 4);
			std::memcpy(&max_p[k], &uh, 4);
		}
		const float inverse_voxel_size = 1.0f / voxel_size;
		const float gap_p[3] = {max_p[0] - min_p[0], max_p[1] - min_p[1], max_p[2] - min_p[2]};
		for (int k = 0; k < 3; k++)
			if (!(std::ceil((double)(gap_p[k] * inverse_voxel_size)) + 1 < 2097152.0))
			{
				ctx->err = "mulls_voxel_downsample: more than 2^21 voxels along an axis";
				return MULLS_E_UNSUPPORTED;
			}
		const unsigned long long max_vy = (unsigned long long)(std::ceil(gap_p[1] * inverse_voxel_size) + 1);
		const unsigned long long max_vz = (unsigned long long)(std::ceil(gap_p[2] * inverse_voxel_size) + 1);
		launch_vox_keys(st, in, n, min_p, inverse_voxel_size, max_vy * max_vz, max_vz, keys);
		std::vector<unsigned long long> hk(n);
		HIPCHK(ctx, hipMemcpyAsync(hk.data(), keys, (size_t)n * 8, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		struct IdPair
		{
			unsigned long long voxel_idx;
			int idx;
			bool operator<(const IdPair &o) const { return voxel_idx < o.voxel_idx; }
		};
		std::vector<IdPair> id_pairs(n);
		for (uint32_t i = 0; i < n; i++)
			id_pairs[i].voxel_idx = hk[i], id_pairs[i].idx = (int)i;
		std::sort(id_pairs.begin(), id_pairs.end());
		std::vector<uint32_t> first;
		first.reserve(n);
		for (size_t b = 0; b < id_pairs.size();)
		{
			first.push_back((uint32_t)id_pairs[b].idx);
			size_t c = b + 1;
			while (c < id_pairs.size() && id_pairs[c].voxel_idx == id_pairs[b].voxel_idx)
				c++;
			b = c;
		}
		HIPCHK(ctx, hipMemcpyAsync(perm, first.data(), first.size() * 4, hipMemcpyHostToDevice, st));
		launch_cl_gather(st, in, perm, down, (uint32_t)first.size()); // whole 48-byte records
		HIPCHK(ctx, hipStreamSynchronize(st));
		*n_down = (uint32_t)first.size();
		return MULLS_OK;
	}
	// which points of cloud_ground make cloud_ground_down (cfilter.hpp:1955-1968): every ground_random_down_down_rate-th, or the seeded fixed-number selection
	MULLS_HIDDEN void gf_ground_down_indices(const mulls_ground_params *P, uint32_t n_ground, std::vector<uint32_t> &idx)
	{
		idx.clear();
		if (!P->fixed_num_downsampling)
		{
			for (uint32_t i = 0; i < n_ground; i++)
				if ((int)i % P->ground_random_down_down_rate == 0)
					idx.push_back(i);
		}
		else
		{
			std::vector<uint8_t> mask(std::max<uint32_t>(n_ground, 1));
			thin_mask(mask.data(), n_ground, P->down_ground_fixed_num, P->rng_seed, 12);
			for (uint32_t i = 0; i < n_ground; i++)
				if (mask[i])
					idx.push_back(i);
		}
	}
	void mulls_extract_default_params(mulls_extract_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		mulls_ground_default_params(&p->ground);
		mulls_classify_default_params(&p->classify);
		// extract_semantic_pts' scanner filter (cfilter.hpp:2338-2346) with approx_scanner_height 2.0, underground_thre -7.0
		p->apply_scanner_filter = 0;
		p->self_ring_radius = 1.75f;
		p->ghost_radius = 20.0f;
		p->z_min = -2.0f - 4.0f;
		p->z_min_min = -2.0f + -7.0f;
		// test/mulls_slam.cpp:51-53 (apply_dist_filter false, min_dist_used 1.0, max_dist_used 120.0), :40 (cloud_down_res 0.0)
		p->apply_dist_filter = 0;
		p->min_dist_used = 1.0;
		p->max_dist_used = 120.0;
		p->vf_downsample_resolution = 0.0f;
	}

	int mulls_voxel_downsample(mulls_ctx *ctx, const void *pts, uint32_t n, uint32_t stride, float voxel_size, void *out, uint32_t cap, uint32_t *n_out)
	try
	{
		if (!ctx || !n_out || (n && !pts) || (cap && !out) || stride < MULLS_POINT_BYTES)
			return MULLS_E_INVALID;
		*n_out = 0;
		if (voxel_size < 0.001) // `cloud_out = cloud_in` (:90-97)
		{
			*n_out = n;
			for (uint32_t i = 0; i < std::min(n, cap); i++)
				std::memcpy(static_cast<unsigned char *>(out) + (size_t)i * MULLS_POINT_BYTES, static_cast<const unsigned char *>(pts) + (size_t)i * stride, MULLS_POINT_BYTES);
			return MULLS_OK;
		}
		if (n == 0)
			return MULLS_OK;
		if (n > 500000u)
		{
			ctx->err = "mulls_voxel_downsample: more than 500000 points in one scan";
			return MULLS_E_UNSUPPORTED;
		}
		HIPCHK(ctx, hipSetDevice(ctx->device));
		hipStream_t st = ctx->stream;
		const mulls::StreamDrain drain{st};
		const GfArena a = gf_layout(n, false, true);
		if (ex_arena_reserve(ctx, a.total, MULLS_EXTRACT_BATCH_DEFAULT_SCRATCH_BYTES) != MULLS_OK)
			return MULLS_E_HIP;
		unsigned char *base = static_cast<unsigned char *>(ctx->exb_buf);
		if (stride == MULLS_POINT_BYTES)
			HIPCHK(ctx, hipMemcpyAsync(base + a.o_alt, pts, (size_t)n * MULLS_POINT_BYTES, hipMemcpyHostToDevice, st));
		else
			HIPCHK(ctx, hipMemcpy2DAsync(base + a.o_alt, MULLS_POINT_BYTES, pts, stride, MULLS_POINT_BYTES, n, hipMemcpyHostToDevice, st));
		uint32_t nd = 0;
		const int rc = vox_run(ctx, base, a, reinterpret_cast<const float4 *>(base + a.o_alt), n, voxel_size, reinterpret_cast<float4 *>(base), &nd);
		if (rc != MULLS_OK)
			return rc;
		*n_out = nd;
		if (std::min(nd, cap))
		{
			HIPCHK(ctx, hipMemcpyAsync(out, base, (size_t)std::min(nd, cap) * MULLS_POINT_BYTES, hipMemcpyDeviceToHost, st));
			HIPCHK(ctx, hipStreamSynchronize(st));
		}
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	// ---- device-resident feature blocks ------------------------------------------------------------------------------------------------
	int mulls_block_create(mulls_ctx *ctx, mulls_block **out)
	try
	{
		if (!ctx || !out)
			return MULLS_E_INVALID;
		*out = new mulls_block();
		ctx->blocks.push_back(*out);
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}
	void mulls_block_destroy(mulls_ctx *ctx, mulls_block *b)
	{
		if (!b)
			return;
		if (ctx)
		{
			(void)hipSetDevice(ctx->device);
			ctx->blocks.erase(std::remove(ctx->blocks.begin(), ctx->blocks.end(), b), ctx->blocks.end());
		}
		if (b->buf)
			(void)hipFree(b->buf);
		delete b;
	}
	int mulls_block_cloud(mulls_ctx *ctx, const mulls_block *b, int which, mulls_cloud *out)
	{
		if (!ctx || !b || !out || which < 0 || which >= MULLS_EX_COUNT || which == MULLS_EX_RAW || which == MULLS_EX_DOWN)
			return MULLS_E_INVALID;
		out->pts = b->n[which] ? b->buf + b->off[which] : nullptr;
		out->n = b->n[which];
		out->stride = MULLS_POINT_BYTES;
		return MULLS_OK;
	}
	int mulls_block_download(mulls_ctx *ctx, const mulls_block *b, int which, void *pts, uint32_t cap, uint32_t *n)
	try
	{
		if (!ctx || !b || !n || which < 0 || which >= MULLS_EX_COUNT || (cap && !pts))
			return MULLS_E_INVALID;
		*n = b->n[which];
		const uint32_t k = std::min(cap, b->n[which]);
		if (k)
		{
			HIPCHK(ctx, hipSetDevice(ctx->device));
			HIPCHK(ctx, hipMemcpy(pts, b->buf + b->off[which], (size_t)k * MULLS_POINT_BYTES, hipMemcpyDeviceToHost));
		}
		return MULLS_OK;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}
}
