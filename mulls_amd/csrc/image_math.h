// image_math.h — the per-point and per-pixel arithmetic of the pictures of a cloud: CloudUtility::get_cloud_cpt (utility.hpp:800-814), CFilter::generate_2d_map
// (cfilter.hpp:2751-2790) and CFilter::pointcloud_to_rangeimage (:2714-2746), shared by the device (k_image.hip) and the host (image.cpp's checks;
// tests/images_harness.cpp runs all of it on the CPU).  include/mulls_hip.h has the definition these lines follow.  Trigonometry is detmath.h's.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/mulls_hip.h"
#include "detmath.h"

namespace mulls
{
namespace image
{
// ---- centre point ----
// the term of one coordinate of one point: a float divided by the int count converted to float, widened (utility.hpp:807)
MULLS_HD inline double centre_term(float v, uint32_t n) { return (double)(v / (float)n); }

// ---- 2-D map image ----
// mulls_image2d_params as the kernels read it
struct Map2d
{
	double m2pix, half_w, half_h; // (double)(map_width / 2), (double)(map_height / 2): the integer divisions
	double min_height, max_height;
	int32_t width, height, min_points;
	float a; // (float)(-255.0 / (double)(max - min))
	int32_t shift, form;
};
inline Map2d derive(const mulls_image2d_params &p)
{
	Map2d d;
	d.m2pix = p.m2pix;
	d.half_w = (double)(p.map_width / 2), d.half_h = (double)(p.map_height / 2);
	d.min_height = p.min_height, d.max_height = p.max_height;
	d.width = p.map_width, d.height = p.map_height, d.min_points = p.min_points_in_pix;
	d.a = (float)(-255.0 / (double)((int64_t)p.max_points_in_pix - (int64_t)p.min_points_in_pix));
	d.shift = p.shift != 0, d.form = p.count_form;
	return d;
}
// NULL, or why the parameters are refused
inline const char *refusal(const mulls_image2d_params &p)
{
	if (p.max_points_in_pix == p.min_points_in_pix)
		return "max_points_in_pix == min_points_in_pix";
	if (p.map_width < 1 || p.map_height < 1 || (uint64_t)p.map_width * (uint64_t)p.map_height > MULLS_IMAGE_MAX_PIXELS)
		return "map_width / map_height (at least 1, at most 2^26 pixels)";
	if (p.m2pix != p.m2pix || p.min_height != p.min_height || p.max_height != p.max_height)
		return "m2pix or a height limit is NaN";
	if (p.count_form < 0 || p.count_form > 2)
		return "count_form outside 0 .. 2";
	return nullptr;
}

enum : uint32_t
{
	MAP_COUNTED = 0,
	MAP_SKIPPED_HEIGHT = 1,
	MAP_SKIPPED_FRAME = 2
};
// trunc(d) as a pixel coordinate below `size`: false when it is none (non-finite values included: every comparison with NaN is false)
MULLS_HD inline bool pixel_of(double d, int32_t size, uint32_t *out)
{
	const double t = trunc(d);
	if (!(t >= 0.0 && t < (double)size))
		return false;
	*out = (uint32_t)t;
	return true;
}
// one point of generate_2d_map's loop (cfilter.hpp:2773-2784): MAP_COUNTED and its pixel y * width + x, or why it is skipped
MULLS_HD inline uint32_t map_point(float x, float y, float z, float shift_x, float shift_y, const Map2d &M, uint32_t *pixel)
{
	if ((double)z < M.min_height || (double)z > M.max_height)
		return MAP_SKIPPED_HEIGHT;
	const double dx = (double)(x - shift_x) * M.m2pix + M.half_w;
	const double dy = (double)(-(y - shift_y)) * M.m2pix + M.half_h;
	uint32_t px, py;
	if (!pixel_of(dx, M.width, &px) || !pixel_of(dy, M.height, &py))
		return MAP_SKIPPED_FRAME;
	*pixel = py * (uint32_t)M.width + px;
	return MAP_COUNTED;
}
// round half to even of a float in [0, 255] (exact: every step is exact for such a value)
MULLS_HD inline float round_half_even(float v)
{
	const float f = floorf(v), r = v - f;
	if (r > 0.5f)
		return f + 1.0f;
	if (r < 0.5f)
		return f;
	return ((uint32_t)f & 1u) ? f + 1.0f : f;
}
// map -= min; map.convertTo(CV_8UC1, a, 255) on one pixel, as include/mulls_hip.h restates it
MULLS_HD inline uint8_t map_value(int32_t count, int32_t min_points, float a)
{
	const float prod = (float)((int64_t)count - (int64_t)min_points) * a; // (the difference in 64 bits: no overflow for any min_points_in_pix)
	const float v = prod + 255.0f;
	if (!(v > 0.0f)) // (NaN cannot arise: a is finite or the parameters were refused)
		return 0;
	if (v >= 255.0f)
		return 255;
	return (uint8_t)round_half_even(v);
}

// ---- range image ----
struct Range
{
	int32_t width, height;
	float f_up, f_down, max_distance;
};
inline Range derive(const mulls_range_image_params &p)
{
	Range r;
	r.width = p.width, r.height = p.height;
	r.f_up = p.f_up_deg, r.f_down = p.f_down_deg, r.max_distance = p.max_distance;
	return r;
}
inline const char *refusal(const mulls_range_image_params &p)
{
	if (p.width < 1 || p.height < 1 || (uint64_t)p.width * (uint64_t)p.height > MULLS_IMAGE_MAX_PIXELS)
		return "width / height (at least 1, at most 2^26 pixels)";
	if (!std::isfinite(p.f_up_deg) || !std::isfinite(p.f_down_deg) || !std::isfinite(p.max_distance))
		return "f_up_deg, f_down_deg or max_distance is not finite";
	if (!(p.max_distance > 0.0f))
		return "max_distance <= 0";
	return nullptr;
}
// the truncated float clamped to [0, size - 1], then converted (the limits in double: size - 1 need not be a float)
MULLS_HD inline uint32_t clamp_trunc(float f, int32_t size)
{
	const double t = (double)truncf(f), hi = (double)(size - 1);
	return (uint32_t)(t < 0.0 ? 0.0 : (t > hi ? hi : t));
}
// one point of pointcloud_to_rangeimage's loop (cfilter.hpp:2729-2743): false when it is skipped; else its pixel (row * width + column) and its value
MULLS_HD inline bool range_point(float x, float y, float z, const Range &R, uint32_t *pixel, uint32_t *value)
{
	const float d = sqrtf((x * x + y * y) + z * z);
	const float hor = (float)det::atan2_cr((double)y, (double)x);
	const float a = (float)det::asin_cr((double)(z / d));
	const float ver = (float)(((double)a / M_PI) * 180.0);
	const float u = (float)((0.5 * (1 - (double)hor / M_PI)) * R.width);
	const float one = 1.0f;
	const float v = (one - (R.f_up - ver) / (R.f_up + R.f_down)) * (float)R.height;
	if (!(fabsf(u) <= 3.4028234663852886e38f) || !(fabsf(v) <= 3.4028234663852886e38f)) // not finite
		return false;
	const uint32_t c = clamp_trunc(u, R.width), r = clamp_trunc(v, R.height);
	const double q = (double)(d / R.max_distance);
	const double m = 1.0 < q ? 1.0 : q; // min_(1.0, q); q is not NaN here (d is finite or +inf: a NaN d gave a NaN v) and not negative
	*value = (uint32_t)(255.0 * m);
	*pixel = ((uint32_t)R.height - 1u - r) * (uint32_t)R.width + c;
	return true;
}
} // namespace image
} // namespace mulls
