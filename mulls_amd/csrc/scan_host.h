// scan_host.h — the host's share of mulls_scan_prepare / mulls_mapper_add that is arithmetic: the argument check, a frame's transforms as the kernels read
// them, the output offsets.  scan.cpp runs these lines in front of the launches; tests/scanprep_harness.cpp runs them on the CPU.
#pragma once
#include <cmath>
#include <cstring>

#include "hostmath.h"
#include "scan_math.h"

namespace mulls
{
namespace scan
{
// NULL, or why the parameters are refused
inline const char *refusal(const mulls_scan_prep_params &p)
{
	if (!std::isfinite(p.min_dist) || !std::isfinite(p.max_dist))
		return "min_dist / max_dist is not finite";
	if (!std::isfinite(p.vertical_ang_correction_deg) || !std::isfinite(p.scan_begin_ang_deg))
		return "an angle is not finite";
	if (!std::isfinite(p.scan_duration_ms))
		return "scan_duration_ms is not finite";
	if (p.timestamp_mode < 0 || p.timestamp_mode > 2)
		return "timestamp_mode outside 0 .. 2";
	return nullptr;
}

// the mapper's steps are the export's: calib_first is taken as 1 (test/mulls_slam.cpp:966-969)
inline mulls_scan_prep_params mapper_params(const mulls_scan_prep_params &prep)
{
	mulls_scan_prep_params p = prep;
	p.calib_first = 1;
	return p;
}

// pose (column-major 4 x 4; NULL: none) and adjacent_tran (read when compensate) of one frame
inline FrameMove frame_move_of(const double *pose, const double *adjacent_tran, bool compensate)
{
	FrameMove F;
	std::memset(&F, 0, sizeof(F));
	F.last = MULLS_SCAN_LAST_SEED;
	F.compensate = compensate;
	if (compensate)
	{
		Mat4 T;
		std::memcpy(T.v, adjacent_tran, sizeof(T.v));
		double q[4];
		rotation_quaternion(T, q); // Eigen::Quaterniond(Tran.block<3, 3>(0, 0)), cfilter.hpp:475
		const double t[3] = {T.at(0, 3), T.at(1, 3), T.at(2, 3)};
		F.comp = motion_comp_of(q, t, 0.0f);
	}
	F.has_pose = pose != nullptr;
	if (pose)
		for (int r = 0; r < 3; r++)
			for (int c = 0; c < 4; c++)
				F.pose[4 * r + c] = pose[r + 4 * c];
	return F;
}

// frames are appended while they fit (include/mulls_hip.h, capacity): place() gives a frame of n_out records its offset behind the frames before it and says
// whether it is appended; after the first frame that is not, none is.  at: the records all frames placed so far have.
struct Appender
{
	uint64_t at, room;
	bool open;
	uint64_t place(uint32_t n_out, bool *fits)
	{
		const uint64_t o = at;
		at += n_out;
		open = open && at <= room;
		*fits = open;
		return o;
	}
};
} // namespace scan
} // namespace mulls
