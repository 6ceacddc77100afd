// cregistration_fpfh_hip.hpp — the part of the bridge that needs nothing of MULLS' utility.hpp: the library context of a host thread, borrow(), and
// CRegistration<PointT>::compute_fpfh_feature / coarse_reg_fpfhsac (include/common/cregistration.hpp:351-406) on libmulls_hip.so.
// cregistration_hip.hpp includes this header; a translation unit that has only PCL point types and Eigen visible may include it alone.
#ifndef MULLS_CREGISTRATION_FPFH_HIP_HPP
#define MULLS_CREGISTRATION_FPFH_HIP_HPP

#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "mulls_hip.h"

namespace lo
{
namespace hip
{

// One library context per host thread (the reference path is single-threaded and stateless, SURVEY §8b "Threading").
inline mulls_ctx *thread_context(int device = 0)
{
	struct Holder
	{
		mulls_ctx *ctx = nullptr;
		~Holder()
		{
			if (ctx)
				mulls_destroy(ctx);
		}
	};
	static thread_local Holder holder;
	if (!holder.ctx)
	{
		const int rc = mulls_create(device, &holder.ctx);
		if (rc != MULLS_OK)
			throw std::runtime_error("mulls_create failed (" + std::to_string(rc) + "): no usable gfx950 device; there is no CPU fallback");
		// constraint_t carries no per-class cloud sizes: stage only the clouds the registration reads (mulls_result.nsrc0 / ntgt0 of the others read 0)
		(void)mulls_set_option(holder.ctx, MULLS_OPT_LEAN_STAGING, 1.0);
	}
	return holder.ctx;
}

template <typename CloudPtr>
inline mulls_cloud borrow(const CloudPtr &cloud)
{
	typedef typename std::remove_reference<decltype(cloud->points[0])>::type PointT;
	static_assert(sizeof(PointT) >= MULLS_POINT_BYTES, "expects pcl::PointXYZINormal-compatible records (48 bytes)");
	mulls_cloud c;
	c.pts = cloud->points.empty() ? nullptr : static_cast<const void *>(cloud->points.data());
	c.n = static_cast<uint32_t>(cloud->points.size());
	c.stride = static_cast<uint32_t>(sizeof(PointT));
	return c;
}

// CRegistration<PointT>::compute_fpfh_feature (cregistration.hpp:351-369), verbatim signature: pcl::FPFHEstimationOMP over the records' own normals with
// a radius of 2.0 * search_radius, in one device call (mulls_fpfh).  The binding is one early return at the top of the member function:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::compute_fpfh_feature<PointT>(input_cloud, cloud_fpfh, search_radius);
//     #endif
// cloud_fpfh is upstream's fpfhPtr; it is a template parameter because this header names no histogram type: its points need a float histogram[33].
template <typename PointT, typename FpfhPtr>
inline void compute_fpfh_feature(const typename pcl::PointCloud<PointT>::Ptr &input_cloud, FpfhPtr &cloud_fpfh, float search_radius)
{
	const mulls_cloud c = borrow(input_cloud);
	cloud_fpfh->points.resize(c.n);
	if (!c.n)
		return;
	static_assert(sizeof(cloud_fpfh->points[0].histogram) == 33 * sizeof(float), "expects pcl::FPFHSignature33-compatible records");
	mulls_ctx *ctx = thread_context();
	mulls_fpfh_params P;
	mulls_fpfh_default_params(&P);
	P.search_radius = search_radius;
	std::vector<float> hist((size_t)33 * c.n);
	const int rc = mulls_fpfh(ctx, &c, &P, hist.data(), nullptr);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_fpfh failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (uint32_t i = 0; i < c.n; i++)
		std::memcpy(cloud_fpfh->points[i].histogram, &hist[(size_t)33 * i], 33 * sizeof(float));
}

// CRegistration<PointT>::coarse_reg_fpfhsac (cregistration.hpp:372-406), verbatim signature: both clouds' descriptors and
// pcl::SampleConsensusInitialAlignment with setCorrespondenceRandomness(15), in one device call (mulls_coarse_reg_fpfhsac).  The binding:
//     #ifdef MULLS_USE_HIP
//         return lo::hip::coarse_reg_fpfhsac<PointT>(source_cloud, target_cloud, traned_source, transformationS2T, search_radius);
//     #endif
// Returns the fitness score; transformationS2T receives the pose; traned_source the source with its positions under that pose, x' = float(((R_r0 x +
// R_r1 y) + R_r2 z) + t_r) in double, every other field copied (sac_ia.align's output).  Under upstream's settings hypothesis 0 wins
// (include/mulls_hip.h); fpfhsac_params() is where a caller sets a finite max_correspondence_distance, more iterations or a seed.
inline mulls_fpfhsac_params &fpfhsac_params()
{
	struct Holder
	{
		mulls_fpfhsac_params p;
		Holder() { mulls_fpfhsac_default_params(&p); }
	};
	static thread_local Holder holder;
	return holder.p;
}
template <typename PointT>
inline double coarse_reg_fpfhsac(const typename pcl::PointCloud<PointT>::Ptr &source_cloud, const typename pcl::PointCloud<PointT>::Ptr &target_cloud,
								 typename pcl::PointCloud<PointT>::Ptr &traned_source, Eigen::Matrix4d &transformationS2T, float search_radius)
{
	mulls_ctx *ctx = thread_context();
	mulls_fpfhsac_params P = fpfhsac_params();
	P.search_radius = search_radius;
	const mulls_cloud s = borrow(source_cloud), t = borrow(target_cloud);
	mulls_fpfhsac_result R;
	const int rc = mulls_coarse_reg_fpfhsac(ctx, &t, &s, &P, &R);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_coarse_reg_fpfhsac failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (int k = 0; k < 16; k++)
		transformationS2T.data()[k] = R.T[k];
	traned_source->points = source_cloud->points;
	for (auto &p : traned_source->points)
	{
		const double x = p.x, y = p.y, z = p.z;
		p.x = (float)(((R.T[0] * x + R.T[4] * y) + R.T[8] * z) + R.T[12]);
		p.y = (float)(((R.T[1] * x + R.T[5] * y) + R.T[9] * z) + R.T[13]);
		p.z = (float)(((R.T[2] * x + R.T[6] * y) + R.T[10] * z) + R.T[14]);
	}
	return R.fitness;
}

// The two calls for the candidate edges of one loop-closure event (test/mulls_slam.cpp:517-596 tries one query submap against several candidates): every
// cloud's descriptors, and every (source, target) pair's SAC-IA, in one device call each (mulls_compute_fpfh_batch, mulls_coarse_reg_fpfhsac_batch).  Each
// cloud and each pair gets the bits of its single bridge call.  A cloud pointer given several times, the query submap as every pair's target for instance,
// is one cloud to the library: staged once, its descriptors computed once.
template <typename PointT, typename FpfhPtr>
inline void compute_fpfh_feature_batch(const std::vector<typename pcl::PointCloud<PointT>::Ptr> &input_clouds, std::vector<FpfhPtr> &clouds_fpfh, float search_radius)
{
	if (clouds_fpfh.size() != input_clouds.size())
		throw std::runtime_error("compute_fpfh_feature_batch: as many descriptor clouds as input clouds are expected");
	std::vector<mulls_cloud> clouds;
	std::vector<size_t> which;
	for (size_t c = 0; c < input_clouds.size(); c++)
	{
		const mulls_cloud cl = borrow(input_clouds[c]);
		clouds_fpfh[c]->points.resize(cl.n);
		if (cl.n) // (the single bridge call returns an empty cloud's empty descriptors without a device call)
			clouds.push_back(cl), which.push_back(c);
	}
	if (clouds.empty())
		return;
	static_assert(sizeof(clouds_fpfh[0]->points[0].histogram) == 33 * sizeof(float), "expects pcl::FPFHSignature33-compatible records");
	mulls_ctx *ctx = thread_context();
	mulls_fpfh_params P;
	mulls_fpfh_default_params(&P);
	P.search_radius = search_radius;
	std::vector<std::vector<float>> hist(clouds.size());
	std::vector<float *> out(clouds.size());
	for (size_t k = 0; k < clouds.size(); k++)
		hist[k].resize((size_t)33 * clouds[k].n), out[k] = hist[k].data();
	const int rc = mulls_compute_fpfh_batch(ctx, clouds.data(), (uint32_t)clouds.size(), &P, out.data(), nullptr, 0);
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_compute_fpfh_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (size_t k = 0; k < clouds.size(); k++)
		for (uint32_t i = 0; i < clouds[k].n; i++)
			std::memcpy(clouds_fpfh[which[k]]->points[i].histogram, &hist[k][(size_t)33 * i], 33 * sizeof(float));
}

// Pair b is (source_clouds[b], target_clouds[b]); traned_sources[b] and transformationS2T[b] receive what the single bridge call gives them; the
// fitness scores are returned.  fpfhsac_params() applies as it does for the single bridge call: one set of parameters for the whole call.
template <typename PointT>
inline std::vector<double> coarse_reg_fpfhsac_batch(const std::vector<typename pcl::PointCloud<PointT>::Ptr> &source_clouds,
													 const std::vector<typename pcl::PointCloud<PointT>::Ptr> &target_clouds,
													 std::vector<typename pcl::PointCloud<PointT>::Ptr> &traned_sources, std::vector<Eigen::Matrix4d> &transformationS2T,
													 float search_radius)
{
	const size_t B = source_clouds.size();
	if (target_clouds.size() != B || traned_sources.size() != B)
		throw std::runtime_error("coarse_reg_fpfhsac_batch: as many targets and moved sources as sources are expected");
	transformationS2T.resize(B);
	std::vector<double> fitness(B, 0.0);
	if (!B)
		return fitness;
	mulls_ctx *ctx = thread_context();
	mulls_fpfhsac_params P = fpfhsac_params();
	P.search_radius = search_radius;
	std::vector<mulls_fpfhsac_problem> problems(B);
	for (size_t b = 0; b < B; b++)
		problems[b].src = borrow(source_clouds[b]), problems[b].tgt = borrow(target_clouds[b]);
	std::vector<mulls_fpfhsac_result> R(B);
	const int rc = mulls_coarse_reg_fpfhsac_batch(ctx, problems.data(), (uint32_t)B, &P, 0, R.data());
	if (rc != MULLS_OK)
		throw std::runtime_error(std::string("mulls_coarse_reg_fpfhsac_batch failed (") + std::to_string(rc) + "): " + mulls_last_error(ctx));
	for (size_t b = 0; b < B; b++)
	{
		const double *T = R[b].T;
		for (int k = 0; k < 16; k++)
			transformationS2T[b].data()[k] = T[k];
		traned_sources[b]->points = source_clouds[b]->points;
		for (auto &p : traned_sources[b]->points)
		{
			const double x = p.x, y = p.y, z = p.z;
			p.x = (float)(((T[0] * x + T[4] * y) + T[8] * z) + T[12]);
			p.y = (float)(((T[1] * x + T[5] * y) + T[9] * z) + T[13]);
			p.z = (float)(((T[2] * x + T[6] * y) + T[10] * z) + T[14]);
		}
		fitness[b] = R[b].fitness;
	}
	return fitness;
}

} // namespace hip
} // namespace lo

#endif // MULLS_CREGISTRATION_FPFH_HIP_HPP
