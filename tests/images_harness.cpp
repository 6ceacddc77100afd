// images_harness.cpp — mulls_amd/csrc/image_math.h on the CPU: the text the kernels of k_image.hip compile, run over a cloud by plain loops (the centre by
// MULLS_NDT_TREE's strided-partial rule, the counts by one increment per point, the range image by one overwrite per point in index order), for
// tests/test_images.py to hold against tests/images_restated.py.  Built with -fsanitize=address,undefined.
//   images_harness run <in> <out>
//     in : uint32 n, uint32 pad, mulls_image2d_params, mulls_range_image_params, n 48-byte records
//     out: int32 rc of the 2-D map parameters, int32 rc of the range parameters, double centre[3], uint32 counted, skipped_height, skipped_frame, pad,
//          [rc 0: int32 counts[h * w], uint8 image[h * w]], [rc 0: uint8 range image[height * width]]
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mulls_amd/csrc/image_math.h"

using namespace mulls::image;

static std::vector<unsigned char> slurp(const char *path)
{
	std::vector<unsigned char> b;
	FILE *f = std::fopen(path, "rb");
	if (!f)
		return b;
	unsigned char buf[1 << 16];
	size_t k;
	while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0)
		b.insert(b.end(), buf, buf + k);
	std::fclose(f);
	return b;
}

static float coord(const unsigned char *rec, int k)
{
	float v;
	std::memcpy(&v, rec + 4 * k, 4);
	return v;
}

int main(int argc, char **argv)
{
	if (argc != 4 || std::strcmp(argv[1], "run"))
		return 2;
	const std::vector<unsigned char> in = slurp(argv[2]);
	mulls_image2d_params bp;
	mulls_range_image_params rp;
	const size_t head = 8 + sizeof(bp) + sizeof(rp);
	if (in.size() < head)
		return 3;
	uint32_t n;
	std::memcpy(&n, in.data(), 4);
	std::memcpy(&bp, in.data() + 8, sizeof(bp));
	std::memcpy(&rp, in.data() + 8 + sizeof(bp), sizeof(rp));
	if (in.size() != head + (size_t)n * MULLS_POINT_BYTES)
		return 3;
	const unsigned char *recs = in.data() + head;
	const int32_t rc_map = refusal(bp) ? MULLS_E_INVALID : MULLS_OK, rc_range = refusal(rp) ? MULLS_E_INVALID : MULLS_OK;

	// the centre: lane l adds the points l, l + MULLS_NDT_TREE, .. in order, then the halving tree
	double centre[3];
	for (int k = 0; k < 3; k++)
	{
		std::vector<double> partial(MULLS_NDT_TREE, 0.0);
		for (uint32_t l = 0; l < MULLS_NDT_TREE; l++)
			for (uint64_t i = l; i < n; i += MULLS_NDT_TREE)
				partial[l] += centre_term(coord(recs + i * MULLS_POINT_BYTES, k), n);
		for (uint32_t w = MULLS_NDT_TREE / 2; w >= 1; w >>= 1)
			for (uint32_t l = 0; l < w; l++)
				partial[l] += partial[l + w];
		centre[k] = partial[0];
	}

	FILE *out = std::fopen(argv[3], "wb");
	if (!out)
		return 4;
	uint32_t counters[4] = {0, 0, 0, 0};
	std::vector<int32_t> counts;
	std::vector<uint8_t> bev, range;
	if (rc_map == MULLS_OK)
	{
		const Map2d M = derive(bp);
		counts.assign((size_t)bp.map_width * bp.map_height, 0);
		const float sx = M.shift ? (float)centre[0] : 0.0f, sy = M.shift ? (float)centre[1] : 0.0f;
		for (uint32_t i = 0; i < n; i++)
		{
			const unsigned char *r = recs + (size_t)i * MULLS_POINT_BYTES;
			uint32_t pixel = 0;
			const uint32_t kind = map_point(coord(r, 0), coord(r, 1), coord(r, 2), sx, sy, M, &pixel);
			counters[kind]++;
			if (kind == MAP_COUNTED)
				counts.at(pixel)++;
		}
		for (int32_t c : counts)
			bev.push_back(map_value(c, M.min_points, M.a));
	}
	if (rc_range == MULLS_OK)
	{
		const Range R = derive(rp);
		range.assign((size_t)rp.width * rp.height, 0);
		for (uint32_t i = 0; i < n; i++)
		{
			const unsigned char *r = recs + (size_t)i * MULLS_POINT_BYTES;
			uint32_t pixel, value;
			if (range_point(coord(r, 0), coord(r, 1), coord(r, 2), R, &pixel, &value))
				range.at(pixel) = (uint8_t)value;
		}
	}
	std::fwrite(&rc_map, 4, 1, out);
	std::fwrite(&rc_range, 4, 1, out);
	std::fwrite(centre, 8, 3, out);
	std::fwrite(counters, 4, 4, out);
	if (!counts.empty())
	{
		std::fwrite(counts.data(), 4, counts.size(), out);
		std::fwrite(bev.data(), 1, bev.size(), out);
	}
	if (!range.empty())
		std::fwrite(range.data(), 1, range.size(), out);
	return std::fclose(out) ? 4 : 0;
}
