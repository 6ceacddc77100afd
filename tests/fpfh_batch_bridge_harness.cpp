// A stand-alone program over include/cregistration_fpfh_hip.hpp for tests/test_gpu_fpfh_batch.py, built against the stand-in PCL and Eigen types of
// oracle/ref_shim/shim.hpp and linked with libmulls_hip.so: lo::hip::compute_fpfh_feature_batch and lo::hip::coarse_reg_fpfhsac_batch on clouds read
// from a file.  A cloud that several problems name is one pointer here, as a query submap is in a loop-closure event.
//   argv: in out search_radius max_iterations k_correspondences max_correspondence_distance seed
//   in:   uint32 n_clouds; per cloud uint32 n and n records of 48 bytes; uint32 n_problems; per problem uint32 target cloud, source cloud
//   out:  per cloud n x 33 floats (its descriptors); per problem 16 doubles (the pose, column-major), 1 double (the fitness), n_src records (the moved source)
#include <cstdio>
#include <cstdlib>

#include "ref_shim/shim.hpp"

#include "cregistration_fpfh_hip.hpp"

typedef pcl::PointXYZINormal Point_T;
typedef pcl::PointCloud<Point_T>::Ptr CloudPtr;
struct Signature33
{
	float histogram[33];
};
typedef boost::shared_ptr<pcl::PointCloud<Signature33>> FpfhPtr;

int main(int argc, char **argv)
{
	if (argc != 8)
		return 2;
	FILE *in = fopen(argv[1], "rb");
	uint32_t n_clouds = 0, n_problems = 0;
	if (!in || fread(&n_clouds, 4, 1, in) != 1 || n_clouds > 64)
		return 2;
	std::vector<CloudPtr> clouds;
	std::vector<FpfhPtr> fpfh;
	for (uint32_t c = 0; c < n_clouds; c++)
	{
		uint32_t n = 0;
		if (fread(&n, 4, 1, in) != 1 || n > (1u << 20))
			return 2;
		clouds.push_back(CloudPtr(new pcl::PointCloud<Point_T>()));
		fpfh.push_back(FpfhPtr(new pcl::PointCloud<Signature33>()));
		clouds[c]->points.resize(n);
		if (fread(clouds[c]->points.data(), 48, n, in) != n)
			return 2;
	}
	if (fread(&n_problems, 4, 1, in) != 1 || n_problems > 64)
		return 2;
	std::vector<CloudPtr> sources, targets, moved;
	for (uint32_t b = 0; b < n_problems; b++)
	{
		uint32_t ts[2];
		if (fread(ts, 4, 2, in) != 2 || ts[0] >= n_clouds || ts[1] >= n_clouds)
			return 2;
		targets.push_back(clouds[ts[0]]), sources.push_back(clouds[ts[1]]), moved.push_back(CloudPtr(new pcl::PointCloud<Point_T>()));
	}
	fclose(in);
	const float search_radius = (float)atof(argv[3]);
	mulls_fpfhsac_params &P = lo::hip::fpfhsac_params();
	P.max_iterations = atoi(argv[4]), P.k_correspondences = atoi(argv[5]), P.max_correspondence_distance = (float)atof(argv[6]);
	P.seed = (uint32_t)strtoul(argv[7], nullptr, 10);
	std::vector<Eigen::Matrix4d> T;
	std::vector<double> fitness;
	try
	{
		lo::hip::compute_fpfh_feature_batch<Point_T>(clouds, fpfh, search_radius);
		fitness = lo::hip::coarse_reg_fpfhsac_batch<Point_T>(sources, targets, moved, T, search_radius);
	}
	catch (const std::exception &e)
	{
		fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	FILE *out = fopen(argv[2], "wb");
	if (!out || T.size() != n_problems || fitness.size() != n_problems)
		return 2;
	for (uint32_t c = 0; c < n_clouds; c++)
	{
		if (fpfh[c]->points.size() != clouds[c]->points.size())
			return 2;
		fwrite(fpfh[c]->points.data(), sizeof(Signature33), fpfh[c]->points.size(), out);
	}
	for (uint32_t b = 0; b < n_problems; b++)
	{
		if (moved[b]->points.size() != sources[b]->points.size())
			return 2;
		fwrite(T[b].data(), 8, 16, out);
		fwrite(&fitness[b], 8, 1, out);
		fwrite(moved[b]->points.data(), 48, moved[b]->points.size(), out);
	}
	fclose(out);
	return 0;
}
