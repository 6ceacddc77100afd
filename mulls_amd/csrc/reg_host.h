// reg_host.h — the host part that mulls_ndt, mulls_gicp and mulls_pcl_icp have in common (reg_host.cpp; fpfh.cpp uses its arena, uploads and staging): the pre-steps of omp_ndt, omp_gicp and pcl_icp
// are the same text upstream, and a sub-batch of any of them is the same sequence around its own launches.  Plain functions that ndt.cpp, gicp.cpp and
// pcl_icp.cpp call in the order they need: the checks of a call, a problem's crop descriptor, the sub-batch's memory, the uploads, the staging of
// descriptors, the tick loop, the download of records, and the output pose.
#pragma once
#include <initializer_list>
#include <string>
#include <vector>

#include "ctx.h"
#include "ndt_launch.h"
#include "subbatch.h"

namespace reg_host
{
constexpr uint32_t MAX_SUB_BATCH = 4096u; // problems of one sub-batch (at most three tables each in one grid dimension of the per-point launches)

// hands out the arena: offsets in steps of 256 bytes
struct Arena
{
	size_t off = 0;
	uint64_t operator()(size_t bytes)
	{
		const size_t at = off;
		off += up256(bytes);
		return (uint64_t)at;
	}
};

// ---- a call ----
// who + "problem N: " (nothing after who for a single call)
std::string refusal_prefix(const std::string &who, bool single, uint32_t index);
// the argument checks of every problem before any device work; a refusal is left in ctx->err
int check_problems(mulls_ctx *ctx, const mulls_ndt_problem *problems, uint32_t n_problems, const std::string &who, bool single);
// the guess and the bounds of a problem into the crop's descriptor; -> is the guess applied (it is not the identity)?
bool crop_desc(const mulls_ndt_problem &P, bool crop, NdtDesc &N);
// the cuts of a call into sub-batches by the problems' arena bytes (subbatch.h): sub-batch c is cuts[c] .. cuts[c + 1]
std::vector<uint32_t> cuts_of(const std::vector<uint64_t> &bytes, uint64_t limit);

// ---- a sub-batch ----
// the context's device arena and pinned buffer, grown to hold this many bytes
int reserve(mulls_ctx *ctx, size_t dev_bytes, size_t pinned_bytes, unsigned char **dev, unsigned char **pinned);
// a problem's two clouds, packed to 12 bytes a point, to N.o_src_in and N.o_tgt_in (a host cloud through the pinned buffer, a device cloud by a strided copy)
int upload_problem(mulls_ctx *ctx, const mulls_ndt_problem &P, const NdtDesc &N, unsigned char *dev, unsigned char *pinned);
// is a cloud's memory the device's (a map's, or what the runtime calls device memory)?
bool on_device(mulls_ctx *ctx, const mulls_cloud &c);
// the three floats at byte `offset` of every record (0: the coordinates, 16: the normal), packed to 12 bytes a point, to dst
int upload_xyz(mulls_ctx *ctx, const mulls_cloud &c, uint32_t offset, unsigned char *dst, unsigned char *pinned);
// blocks between the host and the arena through the pinned buffer, each at the next multiple of 256 bytes of it.  stage() queues the copies up: the
// pinned buffer is free again after the next wait on the stream.  download() waits, then fills the hosts' blocks.
struct Block
{
	void *dev;
	void *host;
	size_t bytes;
};
inline size_t pinned_bytes(std::initializer_list<size_t> blocks)
{
	size_t sum = 0;
	for (size_t b : blocks)
		sum += up256(b);
	return sum;
}
int stage(mulls_ctx *ctx, unsigned char *pinned, std::initializer_list<Block> blocks);
int download(mulls_ctx *ctx, unsigned char *pinned, std::initializer_list<Block> blocks);
// Ticks 0 .. max_ticks - 1 in lock step: tick(running, next) launches one, whose decide kernel adds the problems still running to *running and sets
// *next to 0; after each the word is read back (through pinned), and the loop ends when it reads 0.  words: two zeroed uint32 on the device.
template <typename Tick>
int tick_loop(mulls_ctx *ctx, uint32_t *words, unsigned char *pinned, uint32_t max_ticks, Tick tick)
{
	uint32_t *h_word = reinterpret_cast<uint32_t *>(pinned);
	for (uint32_t t = 0; t < max_ticks; t++)
	{
		if (int rc = tick(words + (t & 1u), words + ((t + 1u) & 1u)))
			return rc;
		HIPCHK(ctx, hipMemcpyAsync(h_word, words + (t & 1u), 4, hipMemcpyDeviceToHost, ctx->stream));
		HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
		if (*h_word == 0)
			break;
	}
	return MULLS_OK;
}

// ---- the output pose ----
// T = [R | t] * guess (column-major 4 x 4; R row-major; the guess only where it was applied)
void pose_of(const double *R, const double *t, const mulls_ndt_problem &P, bool apply_guess, double *T);
// the pose of a problem that did not run: the guess where it was applied, else the identity
void idle_pose(const mulls_ndt_problem &P, bool apply_guess, double *T);
} // namespace reg_host
