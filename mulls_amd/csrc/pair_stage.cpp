// pair_stage.cpp — the host side the two coarse-registration solvers share (pair_stage.h): where a cloud lies, the stride check, the packing of host clouds
// and the staging of a list of problems' pairs into a device arena.
#include "pair_stage.h"

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

void pack_xyzw(const mulls_cloud &c, const int32_t *idx, uint32_t n, float *out)
{
	const unsigned char *p = static_cast<const unsigned char *>(c.pts);
	for (uint32_t i = 0; i < n; i++, out += 4)
		std::memcpy(out, p + (size_t)(idx ? (uint32_t)idx[i] : i) * c.stride, 16);
}

int check_strides(const Refusal &refuse, const mulls_cloud &T, const mulls_cloud &S, BatchProblem *A)
{
	A->t_dev = cloud_on_device(refuse.ctx, T), A->s_dev = cloud_on_device(refuse.ctx, S);
	if ((A->t_dev && T.stride != MULLS_POINT_BYTES) || (A->s_dev && S.stride != MULLS_POINT_BYTES) || (!A->t_dev && (T.stride < 16u || T.stride % 4u)) ||
		(!A->s_dev && (S.stride < 16u || S.stride % 4u)))
		return refuse(MULLS_E_INVALID, "stride (device clouds: 48; host clouds: a multiple of 4, at least 16)");
	return MULLS_OK;
}

int stage_pairs(mulls_ctx *ctx, hipStream_t st, unsigned char *d, unsigned char *h, const PairStagePlaces &L, const PairStageItem *items, uint32_t count)
{
	PairGather *jobs = reinterpret_cast<PairGather *>(h + L.p_jobs);
	uint32_t n_jobs = 0, n_max = 0;
	bool any_host = false, any_idx = false;
	for (uint32_t k = 0; k < count; k++)
	{
		const PairStageItem &I = items[k];
		const uint32_t n = I.n, indexed = I.indexed ? 1u : 0u;
		if (I.indexed && (I.t_dev || I.s_dev))
		{
			int32_t *h_idx = reinterpret_cast<int32_t *>(h + L.p_idx + (I.o_idx - L.o_idx));
			std::memcpy(h_idx, I.tgt_idx, (size_t)n * 4u);
			std::memcpy(h_idx + n, I.src_idx, (size_t)n * 4u);
			any_idx = true;
		}
		if (I.t_dev)
			jobs[n_jobs++] = PairGather{static_cast<const unsigned char *>(I.tgt->pts), I.o_idx, I.o_tgt, n, indexed}, n_max = std::max(n_max, n);
		else
			pack_xyzw(*I.tgt, I.indexed ? I.tgt_idx : nullptr, n, reinterpret_cast<float *>(h + L.p_pts + (I.o_tgt - L.o_pts))), any_host = true;
		if (I.s_dev)
			jobs[n_jobs++] = PairGather{static_cast<const unsigned char *>(I.src->pts), I.o_idx + (uint64_t)n * 4u, I.o_src, n, indexed}, n_max = std::max(n_max, n);
		else
			pack_xyzw(*I.src, I.indexed ? I.src_idx : nullptr, n, reinterpret_cast<float *>(h + L.p_pts + (I.o_src - L.o_pts))), any_host = true;
	}
	if (any_host) // (the places of device-resident clouds go up as they are and are gathered over below)
		HIPCHK(ctx, hipMemcpyAsync(d + L.o_pts, h + L.p_pts, L.pts_bytes, hipMemcpyHostToDevice, st));
	if (any_idx)
		HIPCHK(ctx, hipMemcpyAsync(d + L.o_idx, h + L.p_idx, L.idx_bytes, hipMemcpyHostToDevice, st));
	if (n_jobs)
	{
		HIPCHK(ctx, hipMemcpyAsync(d + L.o_jobs, jobs, sizeof(PairGather) * n_jobs, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, launch_pair_gather(st, reinterpret_cast<const PairGather *>(d + L.o_jobs), n_jobs, n_max, d));
	}
	return MULLS_OK;
}
