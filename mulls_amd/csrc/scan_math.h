// scan_math.h — the per-point arithmetic of the raw-scan steps in front of extract_semantic_pts and of the merged-map export (test/mulls_slam.cpp:359-362,
// :404-412, :959-1015), shared by the device (k_scan.hip, k_setup.hip's k_motion_comp, k_ground.hip's k_raw_mask) and the host (scan.cpp's planning;
// tests/scanprep_harness.cpp runs all of it on the CPU).  include/mulls_hip.h has the definition these lines follow.  Trigonometry is detmath.h's: the
// same bits on the host and on the device, no math library of either.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/mulls_hip.h"
#include "detmath.h"

namespace mulls
{
namespace scan
{
// mulls_scan_prep_params as the kernels read it: the per-call constants upstream computes in front of its loops
struct Prep
{
	double ang_rad;		   // var_vertical_ang_d / 180.0 * M_PI (cfilter.hpp:266)
	double min_sq, max_sq; // xy_dist_min * xy_dist_min, xy_dist_max * xy_dist_max (:819)
	double begin_rad;	   // scan_begin_ang_anticlock_x_positive_deg / 180.0 * M_PI (:418)
	int32_t ratio;		   // >= 1
	int32_t ts_mode;	   // 0 off, 1 from time stamps, 2 from azimuth
	uint8_t calib;		   // 0: nothing, 1: the rotation of the vertical angle, 2: z negated
	uint8_t dist_on, calib_first, pad_;
};
inline Prep derive(const mulls_scan_prep_params &p)
{
	Prep d;
	d.ang_rad = p.vertical_ang_correction_deg / 180.0 * M_PI;
	d.min_sq = p.min_dist * p.min_dist;
	d.max_sq = p.max_dist * p.max_dist;
	d.begin_rad = p.scan_begin_ang_deg / 180.0 * M_PI;
	d.ratio = p.downsample_ratio > 1 ? p.downsample_ratio : 1;
	d.ts_mode = p.timestamp_mode;
	d.calib = !p.calib_on || p.vertical_ang_correction_deg == 0 ? 0 : (p.vertical_ang_correction_deg >= 180.0 ? 2 : 1); // :252-263
	d.dist_on = p.dist_filter_on != 0;
	d.calib_first = p.calib_first != 0;
	d.pad_ = 0;
	return d;
}

// CFilter::dist_filter(cloud, xy_dist_min, xy_dist_max) (cfilter.hpp:815-821): the float range expression widened to double, against the squared limits
MULLS_HD inline bool dist_keep(float x, float y, double min_sq, double max_sq)
{
	const float dis_square = x * x + y * y;
	return (double)dis_square < max_sq && (double)dis_square > min_sq;
}

// CFilter::vertical_intrinsic_calibration (cfilter.hpp:258-287) on one point
MULLS_HD inline void calibrate(float &x, float &y, float &z, const Prep &P)
{
	if (P.calib == 2)
	{
		z = -z; // z *= (-1.0)
		return;
	}
	if (P.calib != 1)
		return;
	const double dist = (double)sqrtf((x * x + y * y) + z * z); // std::sqrt of a float expression: the float root
	const double v_ang = det::asin_cr((double)z / dist);
	const double v_ang_c = v_ang + P.ang_rad;
	const double hor_scale = det::cos_cr(v_ang_c) / det::cos_cr(v_ang);
	x = (float)((double)x * hor_scale);
	y = (float)((double)y * hor_scale);
	z = (float)(dist * det::sin_cr(v_ang_c));
}

// the point's test in the flag pass: the dist filter on the coordinates it sees (calibrated ones when the calibration comes first)
MULLS_HD inline bool survives(float x, float y, float z, const Prep &P)
{
	if (!P.dist_on)
		return true;
	if (P.calib_first && P.calib == 1)
		calibrate(x, y, z, P);
	return dist_keep(x, y, P.min_sq, P.max_sq);
}

// CFilter::random_downsample(cloud, ratio) (cfilter.hpp:734-741) keeps the indices i with i % ratio == 0: of the ranks [base, base + count) these many ...
MULLS_HD inline uint32_t multiples_below(uint32_t a, uint32_t ratio) { return a / ratio + (a % ratio ? 1u : 0u); } // r in [0, a) with r % ratio == 0
MULLS_HD inline uint32_t thin_count(uint32_t base, uint32_t count, uint32_t ratio) { return multiples_below(base + count, ratio) - multiples_below(base, ratio); }
// ... and a kept rank r lands at multiples_below(r, ratio) = r / ratio
MULLS_HD inline uint32_t chunks_of(uint32_t n) { return n / MULLS_SCAN_CHUNK + (n % MULLS_SCAN_CHUNK ? 1u : 0u); }

// get_pts_timestamp_ratio_in_frame, time stamps (cfilter.hpp:428-439).  max_ / min_ are utility.hpp:31-32's macros: (a > b) ? a : b and (a < b) ? a : b —
// the later of two equal values wins, which is visible for +0 against -0; the folds below keep the cloud's order so that the same one wins here.
MULLS_HD inline double fold_last(double acc, double c) { return acc > c ? acc : c; }
MULLS_HD inline double fold_first(double acc, double c) { return acc < c ? acc : c; }
#define MULLS_SCAN_LAST_SEED (-1.7976931348623157e308) // -DBL_MAX (:420)
#define MULLS_SCAN_FIRST_SEED 1.7976931348623157e308   // DBL_MAX (:421)
MULLS_HD inline float stamp_duration(double first, double last, float scan_duration_ms)
{
	const double actual_scan_duration = last - first;
	return actual_scan_duration < scan_duration_ms * 0.75 ? (float)actual_scan_duration : scan_duration_ms;
}
MULLS_HD inline float stamp_ratio(float curvature, double last, float scan_duration_ms)
{
	const double s = (last - (double)curvature) / (double)scan_duration_ms;
	const double m = 0.0 > s ? 0.0 : s; // max_(0.0, s)
	return (float)(1.0 < m ? 1.0 : m);	// min_(1.0, .)
}
// ... azimuth (:447-463)
MULLS_HD inline float azimuth_ratio(float x, float y, double begin_rad)
{
	const double two_pi = 2 * M_PI;
	double ang = det::atan2_cr((double)y, (double)x);
	if (ang < 0)
		ang += two_pi;
	ang += begin_rad;
	if (ang >= two_pi)
		ang -= two_pi;
	return (float)((two_pi - ang) / two_pi);
}

// CFilter::apply_motion_compensation(pc_in_out, Tran, s_ambigous_thre) (cfilter.hpp:470-491): the point with time stamp t = curvature in [thre, 1 - thre]
// moves by the fraction t of Tran — slerp from the identity quaternion (Eigen's QuaternionBase::slerp), linear translation — in double, stored as float
struct MotionComp
{
	double q[4]; // Eigen::Quaterniond(Tran.block<3,3>(0,0)): w x y z
	double t[3]; // Tran.block<3,1>(0,3)
	double theta, sin_theta; // acos(|q.w|) — one value per transform, by the HOST's libm, the reference's own (motion_comp_of) — and its sine (detmath.h)
	float thre;
};
inline MotionComp motion_comp_of(const double q[4], const double t[3], float thre)
{
	MotionComp M;
	for (int k = 0; k < 4; k++)
		M.q[k] = q[k];
	for (int k = 0; k < 3; k++)
		M.t[k] = t[k];
	M.thre = thre;
	M.theta = std::acos(std::fabs(q[0]) < 1.0 ? std::fabs(q[0]) : 1.0);
	M.sin_theta = det::sin_cr(M.theta);
	return M;
}
MULLS_HD inline bool motion_comp_point(float &x, float &y, float &z, float sc /* curvature */, const MotionComp &M) // false: outside the window, nothing moved
{
	if (sc < M.thre || (double)sc > 1.0 - M.thre)
		return false;
	const double t = (double)sc, one = 1.0 - 2.220446049250313e-16;
	const double dq = M.q[0], absD = std::fabs(dq);
	double s0, s1;
	if (absD >= one)
	{
		s0 = 1.0 - t;
		s1 = t;
	}
	else
	{
		// (the two sines per point by detmath.h's correctly rounded sine: the same bits on every ROCm version and on the host, like the rest of the library's
		// trigonometry; the device library's acos / sin were the one place where a result depended on the toolchain — advisor, round 4)
		const double theta = M.theta, sinTheta = M.sin_theta;
		s0 = det::sin_cr((1.0 - t) * theta) / sinTheta;
		s1 = det::sin_cr((t * theta)) / sinTheta;
	}
	if (dq < 0)
		s1 = -s1;
	const double qw = s0 + s1 * M.q[0], qx = s1 * M.q[1], qy = s1 * M.q[2], qz = s1 * M.q[3];
	const double vx = x, vy = y, vz = z;
	const double uvx = 2.0 * (qy * vz - qz * vy), uvy = 2.0 * (qz * vx - qx * vz), uvz = 2.0 * (qx * vy - qy * vx);
	const double rx = vx + qw * uvx + (qy * uvz - qz * uvy);
	const double ry = vy + qw * uvy + (qz * uvx - qx * uvz);
	const double rz = vz + qw * uvz + (qx * uvy - qy * uvx);
	x = (float)(rx + t * M.t[0]);
	y = (float)(ry + t * M.t[1]);
	z = (float)(rz + t * M.t[2]);
	return true;
}

// pcl::transformPointCloud by a pose (12 values, row-major 3 x 4): positions in double, stored as float; every other field stays (map_kernels.hip's rule)
MULLS_HD inline void pose_point(float &x, float &y, float &z, const double *T)
{
	const double dx = x, dy = y, dz = z;
	x = (float)(T[0] * dx + T[1] * dy + T[2] * dz + T[3]);
	y = (float)(T[4] * dx + T[5] * dy + T[6] * dz + T[7]);
	z = (float)(T[8] * dx + T[9] * dy + T[10] * dz + T[11]);
}

// everything after the selection on one kept record's words 0 and 2, in upstream's order: whichever of calibration and dist filter comes second has run on
// the coordinates by now (the dist test decided the selection already), then the time ratio, [the mapper:] compensation and pose
struct FrameMove
{
	MotionComp comp;
	double pose[12];
	double last;	// the frame's last time stamp (mode 1)
	float duration; // the duration its ratios divide by (mode 1)
	uint8_t compensate, has_pose, pad_[2];
};
MULLS_HD inline void finish_point(float &x, float &y, float &z, float &curvature, const Prep &P, const FrameMove &F)
{
	calibrate(x, y, z, P);
	if (P.ts_mode == 1)
		curvature = stamp_ratio(curvature, F.last, F.duration);
	else if (P.ts_mode == 2)
		curvature = azimuth_ratio(x, y, P.begin_rad);
	if (F.compensate)
		motion_comp_point(x, y, z, curvature, F.comp);
	if (F.has_pose)
		pose_point(x, y, z, F.pose);
}
} // namespace scan
} // namespace mulls
