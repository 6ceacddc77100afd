// reg_host.cpp — the host part that mulls_ndt, mulls_gicp and mulls_pcl_icp have in common (reg_host.h)
#include "reg_host.h"

#include <cmath>
#include <cstring>

// a context's scratch of the three entry points: one device arena, one pinned host buffer; grow-only
struct mulls_reg_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr;
	size_t dev_cap = 0, pin_cap = 0;
};

void mulls_reg_release(mulls_ctx *ctx)
{
	if (!ctx->reg)
		return;
	staggered_free(ctx->reg->dev);
	if (ctx->reg->pin)
		(void)hipHostFree(ctx->reg->pin);
	delete ctx->reg;
	ctx->reg = nullptr;
}

namespace
{
// Eigen's isIdentity(prec) of a column-major 4 x 4
bool is_identity(const double *G, double prec)
{
	for (int c = 0; c < 4; c++)
		for (int r = 0; r < 4; r++)
		{
			const double v = G[r + 4 * c];
			if (r == c)
			{
				if (!(std::fabs(v - 1.0) <= std::min(std::fabs(v), 1.0) * prec))
					return false;
			}
			else if (!(std::fabs(v) <= prec))
				return false;
		}
	return true;
}

int check_problem(const mulls_ndt_problem &P, std::string &msg)
{
	const mulls_cloud *cl[2] = {&P.tgt, &P.src};
	for (int k = 0; k < 2; k++)
	{
		const char *name = k ? "the source" : "the target";
		if (cl[k]->n == 0)
		{
			msg = std::string(name) + " is empty";
			return MULLS_E_INVALID;
		}
		if (!cl[k]->pts)
		{
			msg = std::string(name) + " is NULL";
			return MULLS_E_INVALID;
		}
		if (cl[k]->stride < 12 || cl[k]->stride % 4)
		{
			msg = std::string(name) + " has a stride below 12 or not a multiple of 4";
			return MULLS_E_INVALID;
		}
		if (cl[k]->n > MULLS_NDT_MAX_POINTS)
		{
			msg = std::string(name) + " has more than 2^24 points";
			return MULLS_E_UNSUPPORTED;
		}
	}
	for (int k = 0; k < 16; k++)
		if (!std::isfinite(P.init_guess[k]))
		{
			msg = "init_guess is not finite";
			return MULLS_E_INVALID;
		}
	for (int k = 0; k < 6; k++)
		if (!std::isfinite(P.tgt_bound[k]) || !std::isfinite(P.src_bound[k]))
		{
			msg = "a bound is not finite";
			return MULLS_E_INVALID;
		}
	return MULLS_OK;
}

} // namespace

namespace reg_host
{
bool on_device(mulls_ctx *ctx, const mulls_cloud &c)
{
	if (mulls_is_map_memory(ctx, c.pts, (size_t)c.n * c.stride))
		return true;
	hipPointerAttribute_t at;
	std::memset(&at, 0, sizeof(at));
	if (hipPointerGetAttributes(&at, c.pts) == hipSuccess)
		return at.type == hipMemoryTypeDevice;
	(void)hipGetLastError(); // (an ordinary host pointer: the query reports an error on some runtimes — cleared)
	return false;
}

int upload_xyz(mulls_ctx *ctx, const mulls_cloud &c, uint32_t offset, unsigned char *dst, unsigned char *pinned)
{
	hipStream_t st = ctx->stream;
	if (on_device(ctx, c))
		HIPCHK(ctx, hipMemcpy2DAsync(dst, 12, static_cast<const unsigned char *>(c.pts) + offset, c.stride, 12, c.n, hipMemcpyDeviceToDevice, st));
	else
	{
		const unsigned char *src = static_cast<const unsigned char *>(c.pts) + offset;
		for (uint32_t i = 0; i < c.n; i++)
			std::memcpy(pinned + 12ull * i, src + (size_t)i * c.stride, 12);
		HIPCHK(ctx, hipMemcpyAsync(dst, pinned, 12ull * c.n, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, hipStreamSynchronize(st)); // (the pinned buffer is reused)
	}
	return MULLS_OK;
}
std::string refusal_prefix(const std::string &who, bool single, uint32_t index)
{
	return who + (single ? std::string() : "problem " + std::to_string(index) + ": ");
}

int check_problems(mulls_ctx *ctx, const mulls_ndt_problem *problems, uint32_t n_problems, const std::string &who, bool single)
{
	for (uint32_t b = 0; b < n_problems; b++)
	{
		std::string msg;
		if (int rc = check_problem(problems[b], msg))
		{
			ctx->err = refusal_prefix(who, single, b) + msg;
			return rc;
		}
	}
	return MULLS_OK;
}

bool crop_desc(const mulls_ndt_problem &P, bool crop, NdtDesc &N)
{
	const bool apply_guess = !is_identity(P.init_guess, 1e-6);
	N.apply_guess = apply_guess ? 1 : 0, N.crop = crop ? 1 : 0;
	for (int r = 0; r < 3; r++)
	{
		for (int c = 0; c < 3; c++)
			N.G[3 * r + c] = P.init_guess[r + 4 * c];
		N.G[9 + r] = P.init_guess[12 + r];
	}
	std::memcpy(N.tgt_bound, P.tgt_bound, sizeof(N.tgt_bound)), std::memcpy(N.src_bound, P.src_bound, sizeof(N.src_bound));
	return apply_guess;
}

std::vector<uint32_t> cuts_of(const std::vector<uint64_t> &bytes, uint64_t limit)
{
	std::vector<uint32_t> cuts;
	sub_batch_cuts(bytes.data(), (uint32_t)bytes.size(), limit, MAX_SUB_BATCH, &cuts);
	return cuts;
}

int reserve(mulls_ctx *ctx, size_t dev_bytes, size_t pinned_bytes, unsigned char **dev, unsigned char **pinned)
{
	if (!ctx->reg)
		ctx->reg = new mulls_reg_scratch();
	mulls_reg_scratch &sc = *ctx->reg;
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, dev_bytes))
		return rc;
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, pinned_bytes, hipHostMallocDefault))
		return rc;
	*dev = sc.dev, *pinned = sc.pin;
	return MULLS_OK;
}

int upload_problem(mulls_ctx *ctx, const mulls_ndt_problem &P, const NdtDesc &N, unsigned char *dev, unsigned char *pinned)
{
	if (int rc = upload_xyz(ctx, P.src, 0, dev + N.o_src_in, pinned))
		return rc;
	return upload_xyz(ctx, P.tgt, 0, dev + N.o_tgt_in, pinned);
}

int stage(mulls_ctx *ctx, unsigned char *pinned, std::initializer_list<Block> blocks)
{
	size_t at = 0;
	for (const Block &b : blocks)
	{
		std::memcpy(pinned + at, b.host, b.bytes);
		HIPCHK(ctx, hipMemcpyAsync(b.dev, pinned + at, b.bytes, hipMemcpyHostToDevice, ctx->stream));
		at += up256(b.bytes);
	}
	return MULLS_OK;
}

int download(mulls_ctx *ctx, unsigned char *pinned, std::initializer_list<Block> blocks)
{
	size_t at = 0;
	for (const Block &b : blocks)
	{
		HIPCHK(ctx, hipMemcpyAsync(pinned + at, b.dev, b.bytes, hipMemcpyDeviceToHost, ctx->stream));
		at += up256(b.bytes);
	}
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	at = 0;
	for (const Block &b : blocks)
	{
		std::memcpy(b.host, pinned + at, b.bytes);
		at += up256(b.bytes);
	}
	return MULLS_OK;
}

void pose_of(const double *R, const double *t, const mulls_ndt_problem &P, bool apply_guess, double *T)
{
	double Tn[16] = {0};
	for (int r = 0; r < 3; r++)
	{
		for (int c = 0; c < 3; c++)
			Tn[r + 4 * c] = R[3 * r + c];
		Tn[r + 12] = t[r];
	}
	Tn[15] = 1.0;
	if (!apply_guess)
	{
		std::memcpy(T, Tn, 16 * sizeof(double));
		return;
	}
	const double *G = P.init_guess;
	for (int r = 0; r < 4; r++)
		for (int c = 0; c < 4; c++)
			T[r + 4 * c] = ((Tn[r] * G[4 * c] + Tn[r + 4] * G[1 + 4 * c]) + Tn[r + 8] * G[2 + 4 * c]) + Tn[r + 12] * G[3 + 4 * c];
}

void idle_pose(const mulls_ndt_problem &P, bool apply_guess, double *T)
{
	for (int k = 0; k < 16; k++)
		T[k] = apply_guess ? P.init_guess[k] : (k % 5 == 0 ? 1.0 : 0.0);
}
} // namespace reg_host
