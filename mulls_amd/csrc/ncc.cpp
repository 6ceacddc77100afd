// ncc.cpp — mulls_ncc_correspond: CRegistration<PointT>::find_feature_correspondence_ncc (cregistration.hpp:409-601), the correspondence stage of the
// reference's global (coarse) registration, on the device, and mulls_ncc_correspond_batch, the same for many problems per call.  Host side: argument
// checks, staging of host clouds (the five live floats per key point), the launch sequence, one download, and — fixed-number mode — the ordering of the
// at most 65 536 selected entries and upstream's serial walk.  The device steps run once per sub-batch (ncc_batch.h plans it, k_ncc_batch.hip runs it),
// the ordering and the walk per problem.  The single call is a batch of one.
#include <cfloat>

#include "ctx.h"
#include "ncc_batch.h"
#include "ncc_launch.h"

// a context's scratch of this entry point: one device arena and one pinned host buffer, grow-only, reused between calls
struct mulls_ncc_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr;
	size_t dev_cap = 0, pin_cap = 0;
};

void mulls_ncc_release(mulls_ctx *ctx)
{
	if (!ctx->ncc)
		return;
	staggered_free(ctx->ncc->dev);
	if (ctx->ncc->pin)
		(void)hipHostFree(ctx->ncc->pin);
	delete ctx->ncc;
	ctx->ncc = nullptr;
}

namespace
{
// device-resident cloud (the library's own block / map memory, or any device allocation of the caller's) or host memory — as mulls_motion_compensate tells them apart
bool cloud_on_device(mulls_ctx *ctx, const mulls_cloud &c)
{
	if (mulls_is_map_memory(ctx, c.pts, (size_t)c.n * MULLS_POINT_BYTES))
		return true;
	hipPointerAttribute_t at;
	std::memset(&at, 0, sizeof(at));
	if (hipPointerGetAttributes(&at, c.pts) == hipSuccess)
		return at.type == hipMemoryTypeDevice;
	(void)hipGetLastError(); // (an ordinary host pointer: the query reports an error on some runtimes — cleared)
	return false;
}

void pack_live(const mulls_cloud &c, float *out)
{
	const unsigned char *p = static_cast<const unsigned char *>(c.pts);
	for (uint32_t i = 0; i < c.n; i++, p += c.stride, out += MULLS_NCC_LIVE)
	{
		std::memcpy(out, p + 12, 12);	  // data[3], normal[0], normal[1]
		std::memcpy(out + 3, p + 28, 8); // normal[3], intensity
	}
}

// the nearest-neighbour modes' download (k_nb_recip's out) -> the caller's lists; returns the full count
uint32_t finish_pairs(const uint32_t *h, uint32_t n_t, int32_t *tgt_idx, int32_t *src_idx, uint32_t cap)
{
	const uint32_t n = std::min(h[0], n_t), w = std::min(n, cap);
	if (w)
	{
		std::memcpy(tgt_idx, h + 2, (size_t)w * 4u);
		std::memcpy(src_idx, h + 2 + n_t, (size_t)w * 4u);
	}
	return n;
}

// the fixed-number mode's download (cand: the count, then the keys up to the rank-K key, unordered) -> the caller's lists; returns the full count
uint32_t finish_fixed(unsigned long long *keys, uint32_t K, uint32_t n_t, uint32_t n_s, int32_t *tgt_idx, int32_t *src_idx, uint32_t cap)
{
	const uint32_t got = (uint32_t)std::min<unsigned long long>(keys[0] & 0xffffffffull, K);
	// ascending distance, equal distances by ascending flat index: the order this library defines where upstream's unstable std::sort leaves it open
	std::sort(keys + 1, keys + 1 + got);
	// :567-586 — a point may take part while its count is not above 6, i.e. seven times
	std::vector<int32_t> count_t(n_t, 0), count_s(n_s, 0);
	uint32_t n = 0;
	for (uint32_t k = 0; k < got; k++)
	{
		const uint32_t index = (uint32_t)keys[1 + k], i = index / n_s, j = index % n_s;
		if (count_t[i] > 6 || count_s[j] > 6)
			continue;
		count_t[i]++;
		count_s[j]++;
		if (n < cap)
		{
			tgt_idx[n] = (int32_t)i;
			src_idx[n] = (int32_t)j;
		}
		n++;
	}
	return n;
}

// ---- both entry points: the single call is a batch of one
const char *const SINGLE = "mulls_ncc_correspond", *const BATCH = "mulls_ncc_correspond_batch";

// a refusal's message: `<entry point>: [problem <b>: ]<why>`
struct Refusal
{
	mulls_ctx *ctx;
	const char *who;
	int64_t problem; // -1: the single call

	int operator()(int code, const char *why) const
	{
		ctx->err = std::string(who) + (problem >= 0 ? ": problem " + std::to_string(problem) : std::string()) + ": " + why;
		return code;
	}
};

struct BatchProblem // a problem that reaches the device
{
	uint32_t index, K;
	bool t_dev, s_dev;
};

// A problem as it was handed in: the refusals, in the order the single call has always had (it never named the first two, and still does not), and the
// reference's answers without a table.  *ret: 0 ("Too few key points"), 1 (fixed-number mode with corr_num <= 0: `true` without a pair), or -1 for a
// problem that goes to the device, with K and the two residences in *A.  The device is selected ahead of the first residence query of a call.
int check_problem(const Refusal &refuse, const mulls_ncc_problem &P, const mulls_ncc_params &params, bool *device_set, BatchProblem *A, int32_t *ret)
{
	mulls_ctx *ctx = refuse.ctx;
	const bool batch = refuse.problem >= 0;
	const mulls_cloud &T = P.tgt, &S = P.src;
	if ((P.cap && (!P.tgt_idx || !P.src_idx)) || (T.n && !T.pts) || (S.n && !S.pts))
		return batch ? refuse(MULLS_E_INVALID, "a NULL cloud or index buffer") : MULLS_E_INVALID;
	if (T.n > (uint32_t)INT32_MAX || S.n > (uint32_t)INT32_MAX) // upstream's sizes are ints
		return batch ? refuse(MULLS_E_UNSUPPORTED, "more than 2^31 - 1 key points") : MULLS_E_UNSUPPORTED;
	*ret = 0;
	if (T.n < 10u || S.n < 10u) // "Too few key points" (:421-425)
		return MULLS_OK;
	A->K = 0;
	if (params.fixed_num_corr)
	{
		if ((uint64_t)T.n * S.n > (uint64_t)INT32_MAX || params.corr_num > (int32_t)MULLS_NCC_MAX_CORR)
			return refuse(MULLS_E_UNSUPPORTED, "fixed-number mode takes at most 2^31 - 1 table entries and corr_num <= 65536");
		*ret = 1;
		if (params.corr_num <= 0)
			return MULLS_OK;
		A->K = (uint32_t)std::min<uint64_t>((uint64_t)params.corr_num, (uint64_t)T.n * S.n); // :565
	}
	if (!*device_set)
	{
		HIPCHK(ctx, hipSetDevice(ctx->device));
		*device_set = true;
	}
	A->t_dev = cloud_on_device(ctx, T), A->s_dev = cloud_on_device(ctx, S);
	if ((A->t_dev && T.stride != MULLS_POINT_BYTES) || (A->s_dev && S.stride != MULLS_POINT_BYTES) || (!A->t_dev && (T.stride < 36u || T.stride % 4u)) ||
		(!A->s_dev && (S.stride < 36u || S.stride % 4u)))
		return refuse(MULLS_E_INVALID, "stride (device clouds: 48; host clouds: a multiple of 4, at least 36)");
	*ret = -1;
	return MULLS_OK;
}

void reset_results(mulls_ncc_result *results, uint32_t n)
{
	for (uint32_t b = 0; b < n; b++)
		results[b].ret = 0, results[b].n_corr = 0;
}

// one sub-batch: `count` problems whose arena fits the limit (or one that does not)
int ncc_sub_batch(mulls_ctx *ctx, const mulls_ncc_problem *problems, const BatchProblem *act, uint32_t count, const mulls_ncc_params *params,
				  mulls_ncc_result *results)
{
	mulls_ncc_scratch &sc = *ctx->ncc;
	const bool fixed = params->fixed_num_corr != 0;
	std::vector<NccBatchShape> shape(count);
	for (uint32_t k = 0; k < count; k++)
	{
		const mulls_ncc_problem &P = problems[act[k].index];
		shape[k] = NccBatchShape{P.tgt.n, P.src.n, act[k].K, act[k].t_dev ? nullptr : P.tgt.pts, act[k].s_dev ? nullptr : P.src.pts, P.tgt.stride, P.src.stride, ~0u, ~0u};
	}
	NccBatchLayout L;
	ncc_batch_layout(shape.data(), count, fixed, &L);
	for (uint32_t k = 0; k < count; k++) // device-resident clouds are read where they are
	{
		const mulls_ncc_problem &P = problems[act[k].index];
		if (act[k].t_dev)
			L.desc[k].in_t = (uint64_t)(uintptr_t)P.tgt.pts;
		if (act[k].s_dev)
			L.desc[k].in_s = (uint64_t)(uintptr_t)P.src.pts;
	}
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, (size_t)L.dev_bytes))
		return rc;
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, (size_t)(L.up_bytes + L.out_bytes), hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin, *h_out = sc.pin + L.up_bytes;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};

	// one upload: the records, the prefix tables and the live floats of every distinct host cloud
	std::memcpy(h + L.o_desc, L.desc.data(), sizeof(NccBatchDesc) * count);
	std::memcpy(h + L.o_wg, L.wg.data(), 4u * (count + 1u));
	std::memcpy(h + L.o_wg_swap, L.wg_swap.data(), 4u * (count + 1u));
	std::memcpy(h + L.o_blk, L.blk.data(), 4u * (count + 1u));
	for (size_t c = 0; c < L.staged_at.size(); c++)
	{
		const mulls_ncc_problem &P = problems[act[L.staged_owner[c] >> 1].index];
		pack_live((L.staged_owner[c] & 1u) ? P.src : P.tgt, reinterpret_cast<float *>(h + L.staged_at[c]));
	}
	HIPCHK(ctx, hipMemcpyAsync(d, h, (size_t)L.up_bytes, hipMemcpyHostToDevice, st));
	HIPCHK(ctx, launch_ncc_batch_describe(st, d, L, count, fixed));
	if (!fixed)
	{
		HIPCHK(ctx, launch_ncc_batch_rowmin(st, d, L, count, 0));
		if (params->reciprocal_on)
			HIPCHK(ctx, launch_ncc_batch_rowmin(st, d, L, count, 1)); // the roles swapped: column minima
		HIPCHK(ctx, launch_ncc_batch_recip(st, d, L, count, params->reciprocal_on != 0));
	}
	else
	{
		HIPCHK(ctx, hipMemsetAsync(d + L.o_sel, 0, (size_t)L.sel_bytes, st));
		HIPCHK(ctx, launch_ncc_batch_select(st, d, L, count));
	}
	HIPCHK(ctx, hipMemcpyAsync(h_out, d + L.o_out, (size_t)L.out_bytes, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	for (uint32_t k = 0; k < count; k++)
	{
		const mulls_ncc_problem &P = problems[act[k].index];
		mulls_ncc_result &R = results[act[k].index];
		unsigned char *o = h_out + (L.desc[k].out - L.o_out);
		R.n_corr = fixed ? finish_fixed(reinterpret_cast<unsigned long long *>(o), act[k].K, P.tgt.n, P.src.n, P.tgt_idx, P.src_idx, P.cap)
						 : finish_pairs(reinterpret_cast<const uint32_t *>(o), P.tgt.n, P.tgt_idx, P.src_idx, P.cap);
		R.ret = 1;
	}
	return MULLS_OK;
}

// who: SINGLE (one problem, named by no number) or BATCH
int ncc_run(mulls_ctx *ctx, const char *who, const mulls_ncc_problem *problems, uint32_t n_problems, const mulls_ncc_params *params, uint64_t limit,
			mulls_ncc_result *results)
{
	if (!ctx || (n_problems && (!problems || !results)))
		return MULLS_E_INVALID;
	reset_results(results, n_problems);
	if (!n_problems)
		return MULLS_OK;
	if (!params)
		return Refusal{ctx, who, -1}(MULLS_E_INVALID, "params is NULL");
	const bool fixed = params->fixed_num_corr != 0;
	bool device_set = false;
	// every problem is checked before any device work: the first refusal found ends the call, every result at 0
	std::vector<BatchProblem> act;
	std::vector<uint32_t> early_true;
	for (uint32_t b = 0; b < n_problems; b++)
	{
		BatchProblem A;
		int32_t ret;
		if (int rc = check_problem(Refusal{ctx, who, who == SINGLE ? -1 : (int64_t)b}, problems[b], *params, &device_set, &A, &ret))
			return rc;
		A.index = b;
		if (ret < 0)
			act.push_back(A);
		else if (ret)
			early_true.push_back(b);
	}
	for (uint32_t b : early_true)
		results[b].ret = 1;
	if (act.empty())
		return MULLS_OK;
	if (!ctx->ncc)
		ctx->ncc = new mulls_ncc_scratch();
	if (!limit)
		limit = MULLS_NCC_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<uint64_t> bytes(act.size()), wgs(act.size());
	for (size_t k = 0; k < act.size(); k++)
	{
		const mulls_ncc_problem &P = problems[act[k].index];
		bytes[k] = ncc_batch_problem_bytes(P.tgt.n, P.src.n, fixed, act[k].K);
		wgs[k] = ncc_batch_wgs_bound(P.tgt.n, P.src.n);
	}
	std::vector<uint32_t> cuts;
	ncc_batch_cuts(bytes.data(), wgs.data(), (uint32_t)act.size(), limit, &cuts);
	for (size_t c = 0; c + 1 < cuts.size(); c++)
		if (int rc = ncc_sub_batch(ctx, problems, &act[cuts[c]], cuts[c + 1] - cuts[c], params, results))
		{
			reset_results(results, n_problems);
			return rc;
		}
	return MULLS_OK;
}
} // namespace

extern "C"
{
	void mulls_ncc_default_params(mulls_ncc_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->fixed_num_corr = 0; // cregistration.hpp:411
		p->corr_num = 2000;
		p->reciprocal_on = 1;
	}

	int mulls_ncc_correspond(mulls_ctx *ctx, const mulls_cloud *tgt_kpts, const mulls_cloud *src_kpts, const mulls_ncc_params *params, int32_t *tgt_idx,
							 int32_t *src_idx, uint32_t cap, uint32_t *n_corr)
	try
	{
		if (!ctx || !tgt_kpts || !src_kpts || !params || !n_corr || (cap && (!tgt_idx || !src_idx)))
			return MULLS_E_INVALID;
		*n_corr = 0;
		mulls_ncc_problem P;
		P.tgt = *tgt_kpts, P.src = *src_kpts;
		P.tgt_idx = tgt_idx, P.src_idx = src_idx, P.cap = cap, P.reserved = 0;
		mulls_ncc_result R;
		if (int rc = ncc_run(ctx, SINGLE, &P, 1, params, 0, &R)) // (the default scratch limit; a lone problem runs whatever its size)
			return rc;
		*n_corr = R.n_corr;
		return R.ret;
	}
	catch (...)
	{
		return mulls::abi_caught(ctx); // nothing is thrown across the ABI
	}

	int mulls_ncc_correspond_batch(mulls_ctx *ctx, const mulls_ncc_problem *problems, uint32_t n_problems, const mulls_ncc_params *params,
								   uint64_t scratch_limit_bytes, mulls_ncc_result *results)
	try
	{
		return ncc_run(ctx, BATCH, problems, n_problems, params, scratch_limit_bytes, results);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}
}
