// nms_batch.h — mulls_non_max_suppress_batch (include/mulls_hip.h): the records the kernels of k_nms.hip read per problem and per device-resident cloud,
// and the planner that cuts a batch into sub-batches and lays a sub-batch out in the device arena.  Host code without HIP, so that
// tests/nms_batch_harness.cpp can hold it on the CPU.  A sub-batch's arena is, in this order:
//   head      the problem records, the cloud records, the clouds' first blocks of 256 points     \  go up in one copy (the key pass sends the head alone)
//   up        the device-resident clouds' permutations, the host clouds' records in visiting order /
//   work      the device-resident clouds' records in visiting order (gathered on the device), their keys, their non-finite flags (one word per cloud)
//   down      the cursor of the kept records, every problem's header, every problem's kept positions: comes down in one copy
//   out       the kept records of all problems, compact: a problem reserves its range when it knows its count (the cursor); comes down in one copy of
//             as many records as were reserved
// The pinned host mirror has the same offsets.
#pragma once
#include <stdint.h>

#include <map>
#include <tuple>
#include <vector>

#include "../../include/mulls_hip.h"
#include "subbatch.h"

#define MULLS_NMS_BATCH_MAX_PROBLEMS 16384u // problems of one sub-batch: the suppression launch's grid at most

// one problem of the suppression launch as the device sees it.  Offsets are bytes from the arena's base, multiples of 256.
struct NmsBatchDesc
{
	uint64_t recs; // the cloud's records in visiting order (several problems may share them)
	uint64_t hdr;  // NmsBatchHeader
	uint64_t kept; // n positions
	uint32_t n, H; // 10 <= n <= MULLS_NMS_LDS_MAX_POINTS; H = nms_buckets(n)
	uint32_t out_cap, problem; // kept records the problem may return: min(n, cap); its index in the sub-batch
};
// what the suppression leaves per problem
struct NmsBatchHeader
{
	uint32_t n_kept, rounds;
	uint32_t out_at, pad; // first record of the problem's range in the out region
};
// one device-resident cloud of the key launch and of the gather launch
struct NmsBatchSrc
{
	uint64_t src;			   // device address of the caller's 48-byte records
	uint64_t keys, perm, recs; // arena offsets: n keys; n permutation entries and 48 n bytes (0 for a cloud that does not take the one-workgroup path)
	uint32_t n, blk;		   // its first block of 256 points
};

struct NmsBatchShape // what the planner needs of a problem
{
	const void *pts; // with n and stride: identifies a cloud for staging once
	uint32_t n, stride, cap;
	uint32_t on_dev; // device-resident
	uint32_t lds;	 // takes the one-workgroup path (10 <= n <= MULLS_NMS_LDS_MAX_POINTS and the path allows it); 0: below the gate, or the multi-launch path
	uint32_t stage;	 // index of the staged cloud (set by nms_batch_layout), or ~0u
};

struct NmsBatchStaged // a cloud of a sub-batch that takes arena: every one-workgroup cloud, and every device-resident cloud of 10 points or more (its keys)
{
	uint32_t owner; // the first problem of the sub-batch that named it
	uint32_t n, on_dev, lds;
	uint32_t src; // index in NmsBatchLayout::src, or ~0u
	uint64_t recs, keys, perm;
};

struct NmsBatchLayout
{
	std::vector<NmsBatchDesc> desc; // the one-workgroup problems, in problem order
	std::vector<NmsBatchSrc> src;
	std::vector<uint32_t> blk; // src.size() + 1 entries: the last is the key launch's grid
	std::vector<NmsBatchStaged> staged;
	uint32_t n_max = 0;								  // the largest cloud of desc: it sizes the suppression launch's LDS
	uint32_t gather_blk = 0;						  // blocks of the device-resident clouds that are gathered (they come first in src)
	uint32_t n_gather = 0;
	uint64_t o_desc = 0, o_src = 0, o_blk = 0, head_bytes = 0, up_bytes = 0;
	uint64_t o_keys = 0, keys_bytes = 0, o_bad = 0; // the keys of all device-resident clouds and the flags behind them: [o_keys, o_bad + 4 src.size()) comes down
	uint64_t o_cursor = 0, down_bytes = 0;			// [o_cursor, o_cursor + down_bytes): cursor, headers, kept positions
	uint64_t o_out = 0, out_records = 0;
	uint64_t dev_bytes = 0;
};

inline uint32_t nms_batch_takes_lds(uint32_t n, int path) { return n >= 10u && n <= MULLS_NMS_LDS_MAX_POINTS && path != 2 ? 1u : 0u; }

// arena bytes of a staged cloud, and of a problem besides its cloud (its share of the head counted as 256 bytes)
inline uint64_t nms_batch_cloud_bytes(uint32_t n, bool on_dev, bool lds)
{
	if (n < 10u || (!on_dev && !lds))
		return 0;
	return (lds ? up256((uint64_t)n * 48u) : 0u) + (on_dev ? 256u + up256((uint64_t)n * 4u) + (lds ? up256((uint64_t)n * 4u) : 0u) : 0u); // (256: its cloud record)
}
inline uint64_t nms_batch_problem_bytes(uint32_t n, uint32_t cap, bool lds)
{
	if (!lds)
		return 0;
	return 256u + up256((uint64_t)n * 4u) + (uint64_t)(n < cap ? n : cap) * 48u;
}
#define MULLS_NMS_BATCH_FIXED_BYTES 2048u // the roundings of the head's tables, the flags and the cursor

inline uint64_t nms_batch_limit(uint64_t scratch_limit_bytes) { return scratch_limit_bytes ? scratch_limit_bytes : MULLS_NMS_BATCH_DEFAULT_SCRATCH_BYTES; }

// Consecutive cuts, by subbatch.h's rule (a sub-batch takes problems while its bytes stay at or below the limit and holds one at least), with one
// difference: a cloud that several problems of a sub-batch name counts once in it.  bytes, when given, gets every sub-batch's count.
inline void nms_batch_cuts(const NmsBatchShape *shape, uint32_t count, uint64_t scratch_limit_bytes, std::vector<uint32_t> *cuts, std::vector<uint64_t> *bytes = nullptr)
{
	const uint64_t limit = nms_batch_limit(scratch_limit_bytes);
	cuts->assign(1, 0u);
	if (bytes)
		bytes->clear();
	std::map<std::tuple<const void *, uint32_t, uint32_t>, int> seen;
	uint64_t held = MULLS_NMS_BATCH_FIXED_BYTES;
	for (uint32_t b = 0; b < count; b++)
	{
		const NmsBatchShape &P = shape[b];
		const auto key = std::make_tuple(P.pts, P.n, P.stride);
		const uint64_t cloud = nms_batch_cloud_bytes(P.n, P.on_dev != 0, P.lds != 0), own = nms_batch_problem_bytes(P.n, P.cap, P.lds != 0);
		uint64_t add = own + (cloud && !seen.count(key) ? cloud : 0u);
		if (b > cuts->back() && ((add && held + add > limit) || b - cuts->back() >= MULLS_NMS_BATCH_MAX_PROBLEMS)) // (a problem that takes no arena cuts nothing)
		{
			if (bytes)
				bytes->push_back(held);
			cuts->push_back(b), held = MULLS_NMS_BATCH_FIXED_BYTES, seen.clear();
			add = own + cloud;
		}
		held += add;
		if (cloud)
			seen.emplace(key, 1);
	}
	if (count)
	{
		cuts->push_back(count);
		if (bytes)
			bytes->push_back(held);
	}
}

inline uint32_t nms_batch_buckets(uint32_t n) // buckets of the one-workgroup path's hashed grid: the power of two that is at least n (and at least 64)
{
	uint32_t h = 64u;
	while (h < n)
		h <<= 1;
	return h;
}

// the arena of the problems shape[0 .. count), and their records
inline void nms_batch_layout(NmsBatchShape *shape, uint32_t count, NmsBatchLayout *L)
{
	*L = NmsBatchLayout();
	// the staged clouds, each distinct (pointer, n, stride) once; the gathered ones first among the device-resident
	std::map<std::tuple<const void *, uint32_t, uint32_t>, uint32_t> seen;
	for (uint32_t b = 0; b < count; b++)
	{
		NmsBatchShape &P = shape[b];
		P.stage = ~0u;
		if (!nms_batch_cloud_bytes(P.n, P.on_dev != 0, P.lds != 0))
			continue;
		const auto found = seen.emplace(std::make_tuple(P.pts, P.n, P.stride), (uint32_t)L->staged.size());
		P.stage = found.first->second;
		if (found.second)
			L->staged.push_back(NmsBatchStaged{b, P.n, P.on_dev, P.lds, ~0u, 0, 0, 0});
	}
	for (int pass = 0; pass < 2; pass++) // pass 0: gathered (one-workgroup path), pass 1: keys only
		for (size_t s = 0; s < L->staged.size(); s++)
		{
			NmsBatchStaged &S = L->staged[s];
			if (!S.on_dev || (S.lds != 0) != (pass == 0))
				continue;
			S.src = (uint32_t)L->src.size();
			L->src.push_back(NmsBatchSrc{0, 0, 0, 0, S.n, 0});
			if (pass == 0)
				L->n_gather++;
		}
	uint32_t n_lds = 0;
	for (uint32_t b = 0; b < count; b++)
		n_lds += shape[b].lds ? 1u : 0u;

	uint64_t off = 0;
	auto take = [&](uint64_t bytes) {
		const uint64_t at = off;
		off += up256(bytes);
		return at;
	};
	L->o_desc = take(sizeof(NmsBatchDesc) * (uint64_t)n_lds);
	L->o_src = take(sizeof(NmsBatchSrc) * (uint64_t)L->src.size());
	L->o_blk = take(4u * ((uint64_t)L->src.size() + 1u));
	L->head_bytes = off;
	for (NmsBatchStaged &S : L->staged)
		if (S.on_dev && S.lds)
			S.perm = take((uint64_t)S.n * 4u);
	for (NmsBatchStaged &S : L->staged)
		if (!S.on_dev)
			S.recs = take((uint64_t)S.n * 48u);
	L->up_bytes = off;
	for (NmsBatchStaged &S : L->staged)
		if (S.on_dev && S.lds)
			S.recs = take((uint64_t)S.n * 48u);
	L->o_keys = off;
	for (NmsBatchStaged &S : L->staged)
		if (S.on_dev)
			S.keys = take((uint64_t)S.n * 4u);
	L->keys_bytes = off - L->o_keys;
	L->o_bad = take(4u * (uint64_t)L->src.size());
	// the cloud records and their blocks
	L->blk.assign(L->src.size() + 1u, 0u);
	uint32_t blk = 0;
	for (int pass = 0; pass < 2; pass++)
		for (const NmsBatchStaged &S : L->staged)
			if (S.on_dev && (S.lds != 0) == (pass == 0))
			{
				NmsBatchSrc &R = L->src[S.src];
				R.keys = S.keys, R.perm = S.perm, R.recs = S.lds ? S.recs : 0u, R.blk = blk;
				L->blk[S.src] = blk;
				blk += (S.n + 255u) / 256u;
				if (pass == 0)
					L->gather_blk = blk;
			}
	L->blk[L->src.size()] = blk;
	// the problems of the suppression launch
	L->o_cursor = take(4);
	L->desc.reserve(n_lds);
	for (uint32_t b = 0; b < count; b++)
	{
		const NmsBatchShape &P = shape[b];
		if (!P.lds)
			continue;
		NmsBatchDesc D;
		D.recs = L->staged[P.stage].recs;
		D.hdr = D.kept = 0;
		D.n = P.n, D.H = nms_batch_buckets(P.n);
		D.out_cap = P.n < P.cap ? P.n : P.cap, D.problem = b;
		L->desc.push_back(D);
		L->n_max = P.n > L->n_max ? P.n : L->n_max;
	}
	const uint64_t o_hdr = take(sizeof(NmsBatchHeader) * (uint64_t)n_lds);
	for (uint32_t k = 0; k < n_lds; k++)
		L->desc[k].hdr = o_hdr + sizeof(NmsBatchHeader) * (uint64_t)k;
	for (NmsBatchDesc &D : L->desc)
		D.kept = take((uint64_t)D.n * 4u);
	L->down_bytes = off - L->o_cursor;
	L->o_out = off;
	for (const NmsBatchDesc &D : L->desc)
		L->out_records += D.out_cap;
	(void)take(L->out_records * 48u);
	L->dev_bytes = off;
}
