// k_fpfh_batch.hip — SAC-IA for the problems of a sub-batch in lock step (mulls_coarse_reg_fpfhsac_batch; gfx950).  The steps are fpfh_device.h's, the
// text k_fpfh.hip's kernels call; here a wave, a lane or a workgroup finds its problem in the sub-batch's table (fpfh_launch.h) and takes the sizes from
// it.  The descriptors are launch_fpfh_features', whose blockIdx.y is the cloud, and the nearest-target pass is mulls_ndt's, a slot per hypothesis.  No
// atomics; no kernel waits for another workgroup.  Every loop is bounded by a table field, a launch argument or a constant.
#include <hip/hip_runtime.h>

#include "fpfh_device.h"
#include "fpfh_launch.h"

namespace
{
constexpr uint32_t WAVES = 4; // samples of a 256-thread workgroup

// the problem that holds flat hypothesis h: the last b < P with first_hyp <= h (at most 32 halvings)
__device__ __forceinline__ uint32_t problem_of(const FpfhProb *__restrict__ prob, uint32_t P, uint32_t h)
{
	uint32_t lo = 0, hi = P;
	for (int step = 0; step < 32 && hi - lo > 1u; step++)
	{
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (prob[mid].first_hyp <= h)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

__global__ void __launch_bounds__(256) k_fpfh_batch_similar(const FpfhProb *__restrict__ prob, uint32_t P, unsigned char *arena, const int32_t *__restrict__ samples,
															const int32_t *__restrict__ ranks, uint32_t n_samples, int32_t *corr)
{
	const uint32_t s = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (s >= n_samples || P == 0u)
		return;
	const FpfhProb &B = prob[problem_of(prob, P, s / 3u)];
	if (s < B.first_sample || s - B.first_sample >= 3u * B.n_hyp)
		return;
	fpfh_dev::similar_wave(at<const float>(arena, B.o_src_hist), at<const float>(arena, B.o_tgt_hist), samples, ranks, s, B.n_src, B.n_tgt, B.k_eff, lane, corr);
}

__global__ void __launch_bounds__(256) k_fpfh_batch_models(const FpfhProb *__restrict__ prob, uint32_t P, unsigned char *arena, const int32_t *__restrict__ samples,
														   const int32_t *__restrict__ corr, uint32_t n_hyp, double *frames)
{
	const uint32_t h = blockIdx.x * 256u + threadIdx.x;
	if (h >= n_hyp || P == 0u)
		return;
	const FpfhProb &B = prob[problem_of(prob, P, h)];
	if (h < B.first_hyp || h - B.first_hyp >= B.n_hyp)
		return;
	fpfh_dev::model_of(at<const float>(arena, B.o_src), at<const float>(arena, B.o_tgt), samples + 3 * (size_t)h, corr + 3 * (size_t)h, B.n_src, B.n_tgt, frames + 12 * (size_t)h);
}

__device__ __forceinline__ NdtDesc base_of(const FpfhProb &B)
{
	NdtDesc base{};
	base.n_src_in = B.n_src, base.n_tgt_in = B.n_tgt;
	base.o_src = B.o_src, base.o_tgt = B.o_tgt;
	return base;
}

__global__ void __launch_bounds__(256) k_fpfh_batch_slots(const FpfhProb *__restrict__ prob, uint32_t P, uint32_t h0, uint32_t n, uint64_t o_pool, uint64_t d0, NdtDesc *desc,
														  NdtRec *rec)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= n || P == 0u)
		return;
	const uint32_t h = h0 + j;
	const FpfhProb &B = prob[problem_of(prob, P, h)];
	const uint64_t d = B.dist_first + 4ull * B.n_src * (h - B.first_hyp);
	fpfh_dev::slot_of(base_of(B), B.n_src, B.n_tgt, o_pool + (d - d0), desc + j, rec + j);
}

__global__ void __launch_bounds__(256) k_fpfh_batch_errors(const NdtDesc *__restrict__ desc, unsigned char *arena, float thr, int huber, double *err)
{
	__shared__ double s_p[256];
	const uint32_t j = blockIdx.x;
	const double sum = fpfh_dev::error_sum(at<const float>(arena, desc[j].o_dist), desc[j].n_src_in, thr, huber, s_p);
	if (threadIdx.x == 0)
		err[j] = sum;
}

__global__ void __launch_bounds__(256) k_fpfh_batch_pick(const FpfhProb *__restrict__ prob, const double *__restrict__ err, const double *__restrict__ frames, FpfhSacOut *out,
														 double *win_frames, NdtDesc *desc, NdtRec *rec)
{
	__shared__ double s_e[256];
	__shared__ uint32_t s_i[256];
	const uint32_t b = blockIdx.x, t = threadIdx.x;
	const FpfhProb &B = prob[b];
	fpfh_dev::pick_into(err + B.first_hyp, frames + 12 * (size_t)B.first_hyp, B.n_hyp, out + b, s_e, s_i);
	const uint32_t best = s_i[0] < B.n_hyp ? s_i[0] : 0u;
	if (t < 12)
		win_frames[12u * b + t] = frames[12 * ((size_t)B.first_hyp + best) + t];
	if (t == 0)
		fpfh_dev::slot_of(base_of(B), B.n_src, B.n_tgt, B.o_win_dist, desc + b, rec + b);
}
} // namespace

hipError_t launch_fpfh_batch_similar(hipStream_t st, const FpfhProb *prob, uint32_t P, unsigned char *arena, const int32_t *samples, const int32_t *ranks,
									 uint32_t n_samples, int32_t *corr)
{
	hipLaunchKernelGGL(k_fpfh_batch_similar, dim3(blocks_of(n_samples, WAVES)), dim3(256), 0, st, prob, P, arena, samples, ranks, n_samples, corr);
	return hipGetLastError();
}
hipError_t launch_fpfh_batch_models(hipStream_t st, const FpfhProb *prob, uint32_t P, unsigned char *arena, const int32_t *samples, const int32_t *corr,
									uint32_t n_hyp, double *frames)
{
	hipLaunchKernelGGL(k_fpfh_batch_models, dim3(blocks_of(n_hyp, 256)), dim3(256), 0, st, prob, P, arena, samples, corr, n_hyp, frames);
	return hipGetLastError();
}
hipError_t launch_fpfh_batch_slots(hipStream_t st, const FpfhProb *prob, uint32_t P, uint32_t h0, uint32_t n, uint64_t o_pool, uint64_t d0, NdtDesc *desc, NdtRec *rec)
{
	hipLaunchKernelGGL(k_fpfh_batch_slots, dim3(blocks_of(n, 256)), dim3(256), 0, st, prob, P, h0, n, o_pool, d0, desc, rec);
	return hipGetLastError();
}
hipError_t launch_fpfh_batch_errors(hipStream_t st, const NdtDesc *desc, uint32_t n, unsigned char *arena, float thr, int huber, double *err)
{
	hipLaunchKernelGGL(k_fpfh_batch_errors, dim3(n), dim3(256), 0, st, desc, arena, thr, huber, err);
	return hipGetLastError();
}
hipError_t launch_fpfh_batch_pick(hipStream_t st, const FpfhProb *prob, uint32_t P, const double *err, const double *frames, FpfhSacOut *out, double *win_frames,
								  NdtDesc *desc, NdtRec *rec)
{
	hipLaunchKernelGGL(k_fpfh_batch_pick, dim3(P), dim3(256), 0, st, prob, err, frames, out, win_frames, desc, rec);
	return hipGetLastError();
}
