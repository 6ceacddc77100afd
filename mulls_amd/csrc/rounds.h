// rounds.h — the host loop around a device fixed point that is settled by repeated launches (extract_batch.cpp: the promotion of vertex candidates and the
// suppression rounds of the class clouds; nms.cpp: the multi-launch path of mulls_non_max_suppress).
#pragma once
#include "ctx.h"

namespace
{
// Rounds of a settle-until-nothing-is-undecided loop: launch(slot) runs one round that adds the points it leaves undecided to round_cnt[slot].  A round over
// a settled state changes nothing, so rounds are launched in batches and the counters read once per batch — the first batch as long as the previous call's
// loop turned out to be (+ 2: consecutive frames need about the same), further ones `step` rounds: one wait per loop instead of one per `step` rounds (28 us
// each on the frame path).  n_waits counts the waits (the statistics of mulls_extract_features_batch).  All 64 counters come down, so the round that settled is known and the hint follows the data both ways.
template <class Launch>
int run_rounds(mulls_ctx *ctx, hipStream_t st, uint32_t *round_cnt, uint32_t step, uint32_t *hint, const Launch &launch, const char *what, uint32_t *n_waits = nullptr)
{
	uint32_t h[64];
	// a multiple of `step` (4 or 8; 32 is one of both), so that `round` stays one and the reset below meets every multiple of 64
	const uint32_t first = std::min(32u, std::max(step, (*hint + 2u + step - 1u) / step * step));
	for (uint32_t round = 0;;)
	{
		const uint32_t lo = round, batch = round == 0 ? first : step;
		for (uint32_t r = 0; r < batch; r++, round++)
			launch(round & 63u);
		HIPCHK(ctx, hipMemcpyAsync(h, round_cnt, sizeof(h), hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		if (n_waits)
			++*n_waits;
		if (h[(round - 1u) & 63u] == 0)
		{
			uint32_t needed = round;
			for (uint32_t r = lo; r < round; r++)
				if (h[r & 63u] == 0)
				{
					needed = r + 1u;
					break;
				}
			*hint = needed;
			return MULLS_OK;
		}
		if ((round & 63u) == 0)
			HIPCHK(ctx, hipMemsetAsync(round_cnt, 0, 64 * 4, st));
		if (round > (1u << 22))
		{
			ctx->err = what;
			return MULLS_E_HIP;
		}
	}
}
} // namespace
