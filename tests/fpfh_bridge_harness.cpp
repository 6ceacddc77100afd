// A stand-alone program over include/cregistration_fpfh_hip.hpp for tests/test_gpu_fpfh.py, built against the stand-in PCL and Eigen types of
// oracle/ref_shim/shim.hpp and linked with libmulls_hip.so: lo::hip::compute_fpfh_feature and lo::hip::coarse_reg_fpfhsac on clouds read from a file.
//   argv: in out search_radius max_iterations k_correspondences max_correspondence_distance seed
//   in:   uint32 n_tgt, n_src; n_tgt + n_src records of 48 bytes
//   out:  n_src x 33 floats (the source's descriptors); 16 doubles (the pose, column-major); 1 double (the fitness); n_src records (traned_source)
#include <cstdio>
#include <cstdlib>

#include "ref_shim/shim.hpp"

#include "cregistration_fpfh_hip.hpp"

typedef pcl::PointXYZINormal Point_T;
struct Signature33
{
	float histogram[33];
};

int main(int argc, char **argv)
{
	if (argc != 8)
		return 2;
	FILE *in = fopen(argv[1], "rb");
	uint32_t n[2];
	if (!in || fread(n, 4, 2, in) != 2)
		return 2;
	pcl::PointCloud<Point_T>::Ptr tgt(new pcl::PointCloud<Point_T>()), src(new pcl::PointCloud<Point_T>()), moved(new pcl::PointCloud<Point_T>());
	tgt->points.resize(n[0]), src->points.resize(n[1]);
	if (fread(tgt->points.data(), 48, n[0], in) != n[0] || fread(src->points.data(), 48, n[1], in) != n[1])
		return 2;
	fclose(in);
	const float search_radius = (float)atof(argv[3]);
	mulls_fpfhsac_params &P = lo::hip::fpfhsac_params();
	P.max_iterations = atoi(argv[4]), P.k_correspondences = atoi(argv[5]), P.max_correspondence_distance = (float)atof(argv[6]);
	P.seed = (uint32_t)strtoul(argv[7], nullptr, 10);
	boost::shared_ptr<pcl::PointCloud<Signature33>> fpfh(new pcl::PointCloud<Signature33>());
	Eigen::Matrix4d T;
	double fitness = 0.0;
	try
	{
		lo::hip::compute_fpfh_feature<Point_T>(src, fpfh, search_radius);
		fitness = lo::hip::coarse_reg_fpfhsac<Point_T>(src, tgt, moved, T, search_radius);
	}
	catch (const std::exception &e)
	{
		fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	FILE *out = fopen(argv[2], "wb");
	if (!out || fpfh->points.size() != n[1] || moved->points.size() != n[1])
		return 2;
	fwrite(fpfh->points.data(), sizeof(Signature33), n[1], out);
	fwrite(T.data(), 8, 16, out);
	fwrite(&fitness, 8, 1, out);
	fwrite(moved->points.data(), 48, n[1], out);
	fclose(out);
	return 0;
}
