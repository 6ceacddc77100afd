// classify.cpp — what the classification stage of the feature chain (extract_batch.cpp) decides on the host: CFilter::classify_nground_pts
// (cfilter.hpp:2058-2290) runs on the device (k_classify.hip; stable compactions: map_kernels.hip).  What the host does besides moving data is selection bookkeeping: the seeded
// fixed-number selections (upstream: pcl::RandomSample), the sector buckets of xy_normal_balanced_downsample on the few hundred points that
// reach it, and the one step upstream hands to this toolchain's std::sort — non_max_suppress's visiting order — for which the keys come
// back, are sorted by the same std::sort (so that equal keys fall as they fall upstream), and return as a permutation.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mulls_hip.h"
#include "classify_launch.h"
#include "ctx.h"
#include "extract_internal.h"

namespace
{
const size_t REC = MULLS_POINT_BYTES;
typedef std::vector<unsigned char> Bytes;

// random_downsample_pcl (cfilter.hpp:606-628) on raw records, with the ABI's seeded selection
void random_downsample(Bytes &c, int keep_number, uint64_t seed, int cloud_id)
{
	const uint32_t n = (uint32_t)(c.size() / REC);
	if (keep_number < 0 || (long)n <= (long)keep_number) // size_t comparison upstream (:608): a negative count keeps every point
		return;
	std::vector<uint8_t> mask(n);
	thin_mask(mask.data(), n, keep_number, seed, cloud_id);
	size_t w = 0;
	for (uint32_t i = 0; i < n; i++)
		if (mask[i])
		{
			if (w != i)
				std::memmove(c.data() + w * REC, c.data() + (size_t)i * REC, REC);
			w++;
		}
	c.resize(w * REC);
}
// xy_normal_balanced_downsample (cfilter.hpp:551-602): sectors by the normal's azimuth (std::atan2 of this platform's libm, as upstream)
void xy_normal_balanced_downsample(Bytes &c, int keep_number_per_sector, int sector_num, uint64_t seed, int cloud_id)
{
	const uint32_t n = (uint32_t)(c.size() / REC);
	if (keep_number_per_sector < 0 || (long)n <= (long)keep_number_per_sector) // size_t comparison upstream (:555)
		return;
	std::vector<Bytes> sectors(sector_num);
	const double angle_per_sector = 360.0 / sector_num;
	for (uint32_t i = 0; i < n; i++)
	{
		float nrm[2];
		std::memcpy(nrm, c.data() + (size_t)i * REC + 16, sizeof(nrm));
		double ang = std::atan2(nrm[1], nrm[0]);
		if (ang < 0)
			ang += 2 * M_PI;
		ang *= (180.0 / M_PI);
		int sector_id = (int)(ang / angle_per_sector);
		if (sector_id >= sector_num) // -tiny + 2 pi rounds to 2 pi: upstream indexes past the last sector
			sector_id = sector_num - 1;
		if (sector_id < 0)
			sector_id = 0;
		sectors[sector_id].insert(sectors[sector_id].end(), c.data() + (size_t)i * REC, c.data() + (size_t)(i + 1) * REC);
	}
	c.clear();
	for (int j = 0; j < sector_num; j++)
	{
		random_downsample(sectors[j], keep_number_per_sector, seed, cloud_id + j);
		c.insert(c.end(), sectors[j].begin(), sectors[j].end());
	}
}

} // namespace

extern "C"
{
	void mulls_classify_default_params(mulls_classify_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		// what extract_semantic_pts (cfilter.hpp:2301-2318) passes for test/mulls_reg.cpp with script/run_mulls_reg.sh's flags
		p->neighbor_searching_radius = 1.0f;
		p->neighbor_k = 50;
		p->neigh_k_min = 8;
		p->pca_down_rate = 1;
		p->edge_thre = 0.65f;
		p->planar_thre = 0.65f;
		p->edge_thre_down = 0.75f;
		p->planar_thre_down = 0.75f;
		p->extract_vertex_points_method = 2;
		p->curvature_thre = 0.10f;
		p->vertex_curvature_non_max_radius = 1.5f;
		p->linear_vertical_sin_high_thre = 0.94f;
		p->linear_vertical_sin_low_thre = 0.17f;
		p->planar_vertical_sin_high_thre = 0.98f;
		p->planar_vertical_sin_low_thre = 0.34f;
		p->sharpen_with_nms = 1;
		p->pillar_down_fixed_num = 200;
		p->facade_down_fixed_num = 800;
		p->beam_down_fixed_num = 200;
		p->roof_down_fixed_num = 200;
		p->unground_down_fixed_num = 20000;
		p->beam_height_max = FLT_MAX;
		p->roof_height_min = 0.0f;
		p->feature_pts_ratio_guess = 0.3f;
	}

	// the fixed-number thinning of the four *_down clouds (:2247-2257) on host records, host[MULLS_CL_*_DOWN]
	__attribute__((visibility("hidden"))) void mulls_classify_thin_down(std::vector<unsigned char> *host, const mulls_classify_params *P)
	{
		random_downsample(host[MULLS_CL_PILLAR_DOWN], P->pillar_down_fixed_num, P->rng_seed, 31);
		const int sector_num = 4;
		xy_normal_balanced_downsample(host[MULLS_CL_FACADE_DOWN], (int)(P->facade_down_fixed_num / sector_num), sector_num, P->rng_seed, 32);
		xy_normal_balanced_downsample(host[MULLS_CL_BEAM_DOWN], (int)(P->beam_down_fixed_num / sector_num), sector_num, P->rng_seed, 36);
		random_downsample(host[MULLS_CL_ROOF_DOWN], P->roof_down_fixed_num, P->rng_seed, 40);
	}
	// what the classification refuses before it looks at the cloud
	__attribute__((visibility("hidden"))) int mulls_classify_check(mulls_ctx *ctx, const mulls_classify_params *P)
	{
		if (P->pca_down_rate < 1 || P->neighbor_k < 1 || P->neighbor_k > (int)MULLS_CL_MAX_K || !(P->neighbor_searching_radius > 0.0f))
		{
			ctx->err = "mulls_classify_nground: pca_down_rate >= 1, 1 <= neighbor_k <= 64 and a positive radius are required";
			return MULLS_E_INVALID;
		}
		return MULLS_OK;
	}
	// the parameters as the kernels use them (n left 0)
	__attribute__((visibility("hidden"))) void mulls_classify_kernel_params(const mulls_classify_params *P, ClParams *out)
	{
		ClParams &Q = *out;
		std::memset(&Q, 0, sizeof(Q));
		Q.K = (uint32_t)P->neighbor_k;
		Q.down_rate = P->pca_down_rate, Q.k_min = P->neigh_k_min;
		Q.radius = P->neighbor_searching_radius;
		Q.adaptive = P->use_distance_adaptive_pca ? 1 : 0;
		Q.unit_distance = 30.0f; // :2098
		Q.edge_thre = P->edge_thre, Q.planar_thre = P->planar_thre, Q.edge_thre_down = P->edge_thre_down, Q.planar_thre_down = P->planar_thre_down;
		Q.lin_high = P->linear_vertical_sin_high_thre, Q.lin_low = P->linear_vertical_sin_low_thre;
		Q.pla_high = P->planar_vertical_sin_high_thre, Q.pla_low = P->planar_vertical_sin_low_thre;
		Q.beam_height_max = P->beam_height_max, Q.roof_height_min = P->roof_height_min;
		Q.nms = P->sharpen_with_nms ? 1 : 0;
		Q.vertex_method = (P->curvature_thre < 1e-8) ? 0 : P->extract_vertex_points_method; // :2161-2162
		Q.curvature_thre = P->curvature_thre;
		Q.vertex_ratio_thre = P->feature_pts_ratio_guess / P->pca_down_rate;									  // :2167
		Q.min_curvature = (float)(0.3 * P->curvature_thre);													  // :2210
		Q.min_neighbor_feature_pts = (int)(P->feature_pts_ratio_guess / P->pca_down_rate * P->neighbor_k) - 1; // :2206
	}
}
