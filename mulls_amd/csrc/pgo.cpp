// pgo.cpp — mulls_pgo_optimize / mulls_pgo_optimize_batch: GlobalOptimize::optimize_pose_graph_ceres (graph_optimizer.cpp:478-700) and the edge check
// of update_optimized_edges (:713-776).  Host side: argument checks of every problem before any device work, the node classes and limits, the tables of
// the block skyline, the sub-batches, the lock-step iteration loop (k_pgo.hip), the output poses and the edge check.  include/mulls_hip.h has the
// definition this file follows.
#include <cmath>

#include "ctx.h"
#include "pgo_launch.h"
#include "pgo_math.h"
#include "subbatch.h"

// a context's scratch of this entry point: one device arena, one pinned host buffer; grow-only
struct mulls_pgo_scratch
{
	unsigned char *dev = nullptr, *pin = nullptr;
	size_t dev_cap = 0, pin_cap = 0;
};

void mulls_pgo_release(mulls_ctx *ctx)
{
	if (!ctx->pgo)
		return;
	staggered_free(ctx->pgo->dev);
	if (ctx->pgo->pin)
		(void)hipHostFree(ctx->pgo->pin);
	delete ctx->pgo;
	ctx->pgo = nullptr;
}

namespace
{
constexpr uint32_t MAX_SUB_BATCH = 4096u; // problems of one sub-batch (one grid dimension of the per-edge launches)

// what the host works out of one problem before any device work
struct Plan
{
	bool early = false; // status -1
	std::vector<uint32_t> used;			 // input indices of the used edges
	std::vector<int32_t> unk, boxed;	 // per node
	std::vector<double> limit;			 // per node: t, r
	std::vector<uint32_t> node, first, rowoff, colmax, adj0, adj;
	uint32_t n_unk = 0, n_blocks = 0, n_free = 0, n_boxed = 0, n_fixed = 0;
	size_t bytes = 0; // of the arena
	PgoDesc D{};
};

bool all_finite(const double *v, int n)
{
	for (int i = 0; i < n; i++)
		if (!std::isfinite(v[i]))
			return false;
	return true;
}

// the one checker of a problem's arguments; msg: what is wrong (without the entry point's name)
int check_problem(const mulls_pgo_problem &P, std::string &msg)
{
	if ((P.n_nodes && (!P.nodes || !P.poses_out)) || (P.n_edges && !P.edges))
	{
		msg = "a NULL array";
		return MULLS_E_INVALID;
	}
	if (P.n_nodes > MULLS_PGO_MAX_NODES)
	{
		msg = "more than 4096 nodes";
		return MULLS_E_UNSUPPORTED;
	}
	if (P.n_edges > MULLS_PGO_MAX_EDGES)
	{
		msg = "more than 131072 edges";
		return MULLS_E_UNSUPPORTED;
	}
	for (uint32_t i = 0; i < P.n_nodes; i++)
		if (!all_finite(P.nodes[i].pose_init, 16))
		{
			msg = "pose_init of node " + std::to_string(i) + " is not finite";
			return MULLS_E_INVALID;
		}
	for (uint32_t e = 0; e < P.n_edges; e++)
	{
		const mulls_pgo_edge &E = P.edges[e];
		if (E.a < 0 || E.b < 0 || (uint32_t)E.a >= P.n_nodes || (uint32_t)E.b >= P.n_nodes)
		{
			msg = "edge " + std::to_string(e) + " names a node outside the problem";
			return MULLS_E_INVALID;
		}
		if (E.a == E.b)
		{
			msg = "edge " + std::to_string(e) + " joins a node to itself";
			return MULLS_E_INVALID;
		}
		if (E.type < MULLS_PGO_REGISTRATION || E.type > MULLS_PGO_NONE)
		{
			msg = "edge " + std::to_string(e) + " has an unknown type";
			return MULLS_E_INVALID;
		}
		if (!all_finite(E.T, 16) || !all_finite(E.info, 36))
		{
			msg = "T or info of edge " + std::to_string(e) + " is not finite";
			return MULLS_E_INVALID;
		}
	}
	return MULLS_OK;
}

const char *check_params(const mulls_pgo_params &p)
{
	if (p.num_iterations < 0 || p.num_iterations > 1000)
		return "num_iterations outside 0 .. 1000";
	const double v[] = {p.t_limit, p.r_limit, p.function_tolerance, (double)p.robust_delta, (double)p.quat_tran_ratio, (double)p.wrong_edge_translation_thre,
						(double)p.wrong_edge_rotation_thre, (double)p.wrong_edge_ratio_thre};
	for (double x : v)
		if (!(x >= 0.0) || !std::isfinite(x))
			return "a negative or non-finite limit, tolerance, delta, ratio or threshold";
	return nullptr;
}

bool edge_used(const mulls_pgo_edge &E) { return E.type != MULLS_PGO_NONE && E.type != MULLS_PGO_HISTORY; }

// classes, limits, the skyline's tables and the arena's size; MULLS_E_UNSUPPORTED above the skyline's capacity
int make_plan(const mulls_pgo_problem &P, const mulls_pgo_params &prm, Plan &L, std::string &msg)
{
	const uint32_t n = P.n_nodes;
	uint32_t flagged = 0;
	for (uint32_t i = 0; i < n; i++)
		flagged += P.nodes[i].fixed ? 1u : 0u;
	bool with_reg = false;
	int32_t m = 0;
	for (uint32_t e = 0; e < P.n_edges; e++)
		if (edge_used(P.edges[e]))
		{
			L.used.push_back(e);
			if (P.edges[e].type == MULLS_PGO_REGISTRATION)
			{
				m = with_reg ? std::min(m, P.edges[e].a) : P.edges[e].a;
				with_reg = true;
			}
		}
	if ((size_t)(n - flagged) > L.used.size())
	{
		L.early = true;
		return MULLS_OK;
	}
	L.unk.assign(n, -1), L.boxed.assign(n, 0), L.limit.assign(2 * (size_t)n, 0.0);
	int32_t stable_index = with_reg ? m : 0;
	for (uint32_t i = 0; i < n; i++)
	{
		if ((with_reg && (int32_t)i <= m) || P.nodes[i].fixed)
		{
			L.n_fixed++;
			continue;
		}
		L.unk[i] = (int32_t)L.node.size();
		L.node.push_back(i);
		if (prm.free_all_nodes)
		{
			L.n_free++;
			continue;
		}
		double f = 1.0;
		if (P.nodes[i].stable)
			stable_index = (int32_t)i;
		else
			f = (double)((int32_t)i - stable_index);
		L.boxed[i] = 1, L.n_boxed++;
		L.limit[2 * i] = f * prm.t_limit, L.limit[2 * i + 1] = f * prm.r_limit;
	}
	const uint32_t U = L.n_unk = (uint32_t)L.node.size(), E = (uint32_t)L.used.size();
	// the nodes' edge lists (ascending edge index) and the block rows' first columns
	L.adj0.assign(n + 1, 0);
	for (uint32_t k = 0; k < E; k++)
		L.adj0[P.edges[L.used[k]].a + 1]++, L.adj0[P.edges[L.used[k]].b + 1]++;
	for (uint32_t i = 0; i < n; i++)
		L.adj0[i + 1] += L.adj0[i];
	L.adj.assign(2 * (size_t)E, 0);
	{
		std::vector<uint32_t> fill(L.adj0.begin(), L.adj0.end() - 1);
		for (uint32_t k = 0; k < E; k++)
			L.adj[fill[P.edges[L.used[k]].a]++] = k, L.adj[fill[P.edges[L.used[k]].b]++] = k;
	}
	L.first.resize(U), L.rowoff.resize(U + 1), L.colmax.resize(U);
	for (uint32_t u = 0; u < U; u++)
		L.first[u] = u, L.colmax[u] = u;
	for (uint32_t k = 0; k < E; k++)
	{
		const int32_t ua = L.unk[P.edges[L.used[k]].a], ub = L.unk[P.edges[L.used[k]].b];
		if (ua < 0 || ub < 0)
			continue;
		const uint32_t hi = (uint32_t)std::max(ua, ub), lo = (uint32_t)std::min(ua, ub);
		L.first[hi] = std::min(L.first[hi], lo);
	}
	uint64_t blocks = 0;
	for (uint32_t u = 0; u < U; u++)
	{
		L.rowoff[u] = (uint32_t)blocks;
		blocks += u - L.first[u] + 1u;
		if (blocks > MULLS_PGO_MAX_BLOCKS)
		{
			msg = "the block skyline holds more than 262144 blocks";
			return MULLS_E_UNSUPPORTED;
		}
		for (uint32_t j = L.first[u]; j < u; j++) // (ascending u: the last writer is the largest row)
			L.colmax[j] = u;
	}
	if (U)
		L.rowoff[U] = (uint32_t)blocks;
	L.n_blocks = (uint32_t)blocks;
	return MULLS_OK;
}

// the byte offsets of a problem's tables behind `off` (the states of a sub-batch lie together in front: o_state is set by the caller)
void lay_out(Plan &L, uint32_t n, size_t &off)
{
	auto take = [&](size_t bytes) {
		const size_t at = off;
		off += up256(bytes);
		return (uint64_t)at;
	};
	const uint32_t U = L.n_unk, E = (uint32_t)L.used.size();
	PgoDesc &D = L.D;
	D.n_nodes = n, D.n_edges = E, D.n_unk = U, D.n_blocks = L.n_blocks;
	D.o_init = take(56ull * n), D.o_limit = take(16ull * n), D.o_unk = take(4ull * n), D.o_boxed = take(4ull * n);
	D.o_edges = take(sizeof(PgoEdge) * (size_t)E), D.o_adj0 = take(4ull * (n + 1)), D.o_adj = take(8ull * E);
	D.o_node = take(4ull * U), D.o_first = take(4ull * U), D.o_rowoff = take(4ull * (U + 1)), D.o_colmax = take(4ull * U), D.o_blkrow = take(4ull * L.n_blocks);
	D.o_cand = take(56ull * n), D.o_slot = take(8ull * MULLS_PGO_SLOT_DOUBLES * E), D.o_term = take(8ull * E);
	D.o_H = take(288ull * L.n_blocks), D.o_g = take(48ull * U), D.o_diag = take(48ull * U), D.o_delta = take(48ull * U);
}
size_t bytes_of(const Plan &L, uint32_t n)
{
	Plan t;
	t.n_unk = L.n_unk, t.n_blocks = L.n_blocks, t.used.resize(L.used.size());
	size_t off = 0;
	lay_out(t, n, off);
	return off + up256(56ull * n);
}

void weight_matrix(const mulls_pgo_edge &E, const mulls_pgo_params &prm, double *W)
{
	for (int i = 0; i < 36; i++)
		W[i] = 0.0;
	if (prm.use_equal_weight)
	{
		const double r = (double)prm.quat_tran_ratio, r2 = r * r;
		for (int k = 0; k < 6; k++)
			W[7 * k] = k < 3 ? 1.0 : r2;
	}
	else if (prm.use_diagonal_information_matrix)
		for (int k = 0; k < 6; k++)
			W[7 * k] = E.info[7 * k];
	else
		for (int k = 0; k < 6; k++)
			for (int l = 0; l < 6; l++)
				W[6 * k + l] = 0.5 * (E.info[k + 6 * l] + E.info[l + 6 * k]);
}

// the edge check of update_optimized_edges on the output poses
void check_edges(const mulls_pgo_problem &P, const mulls_pgo_params &prm, mulls_pgo_result &res)
{
	const double t_thre = (double)prm.wrong_edge_translation_thre, r_thre = (double)prm.wrong_edge_rotation_thre / 180.0 * 3.14159265358979323846;
	int wrong = 0, correct_reg = 0, checked = 0;
	for (uint32_t e = 0; e < P.n_edges; e++)
	{
		const mulls_pgo_edge &E = P.edges[e];
		if (P.edge_wrong)
			P.edge_wrong[e] = 0;
		if (E.type != MULLS_PGO_REGISTRATION && E.type != MULLS_PGO_ADJACENT)
			continue;
		checked++;
		const double *A = P.poses_out + 16ull * E.a, *B = P.poses_out + 16ull * E.b;
		// (column-major: element (r, c) of X is X[r + 4 c])
		double R[9], t[3], Rd[9], td[3];
		const double d[3] = {B[12] - A[12], B[13] - A[13], B[14] - A[14]};
		for (int r = 0; r < 3; r++)
		{
			for (int c = 0; c < 3; c++)
				R[3 * r + c] = (A[0 + 4 * r] * B[0 + 4 * c] + A[1 + 4 * r] * B[1 + 4 * c]) + A[2 + 4 * r] * B[2 + 4 * c];
			t[r] = (A[0 + 4 * r] * d[0] + A[1 + 4 * r] * d[1]) + A[2 + 4 * r] * d[2];
		}
		const double dd[3] = {E.T[12] - t[0], E.T[13] - t[1], E.T[14] - t[2]};
		for (int r = 0; r < 3; r++)
		{
			for (int c = 0; c < 3; c++)
				Rd[3 * r + c] = (R[0 + r] * E.T[0 + 4 * c] + R[3 + r] * E.T[1 + 4 * c]) + R[6 + r] * E.T[2 + 4 * c];
			td[r] = (R[0 + r] * dd[0] + R[3 + r] * dd[1]) + R[6 + r] * dd[2];
		}
		double q[4];
		pgo::rot2quat(Rd, q);
		const double tn = std::sqrt((td[0] * td[0] + td[1] * td[1]) + td[2] * td[2]);
		const double vn = std::sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
		const double ang = 2.0 * mulls::det::atan2_cr(vn, std::fabs(q[3]));
		if (tn > t_thre || ang > r_thre)
		{
			wrong++;
			if (P.edge_wrong)
				P.edge_wrong[e] = 1;
		}
		else if (E.type == MULLS_PGO_REGISTRATION)
			correct_reg++;
	}
	res.wrong_edges = wrong, res.correct_reg_edges = correct_reg;
	res.edges_ok = !((double)wrong / (double)checked > (double)prm.wrong_edge_ratio_thre || correct_reg == 0);
}

// one sub-batch: problems idx[0 .. B) of the call, all of them with device work
int run_sub_batch(mulls_ctx *ctx, const mulls_pgo_problem *problems, std::vector<Plan> &plans, const uint32_t *idx, uint32_t B, const mulls_pgo_params &prm,
				  mulls_pgo_result *results)
{
	mulls_pgo_scratch &sc = *ctx->pgo;
	hipStream_t st = ctx->stream;
	mulls::StreamDrain drain{st};
	// the arena: descriptors, records, the running counters, every problem's state, then the problems' tables one after another
	size_t off = 0;
	const size_t o_desc = off;
	off += up256(sizeof(PgoDesc) * (size_t)B);
	const size_t o_rec = off;
	off += up256(sizeof(PgoRec) * (size_t)B);
	const size_t o_cnt = off;
	off += up256(4ull * 1001u);
	const size_t o_states = off;
	uint32_t n_max = 0, e_max = 0;
	uint64_t w_max = 0;
	for (uint32_t k = 0; k < B; k++)
	{
		Plan &L = plans[idx[k]];
		L.D.o_state = off;
		off += up256(56ull * problems[idx[k]].n_nodes);
	}
	const size_t o_tables = off;
	for (uint32_t k = 0; k < B; k++)
	{
		Plan &L = plans[idx[k]];
		lay_out(L, problems[idx[k]].n_nodes, off);
		n_max = std::max(n_max, L.D.n_nodes), e_max = std::max(e_max, L.D.n_edges);
		w_max = std::max<uint64_t>(w_max, 36ull * L.D.n_blocks + 6ull * L.D.n_unk);
	}
	if (int rc = grow(ctx, &sc.dev, &sc.dev_cap, off))
		return rc;
	// the host image of what goes up: one problem at a time through the pinned buffer (its tables are contiguous up to o_cand)
	size_t pin_need = std::max(o_states, up256(sizeof(PgoRec) * (size_t)B));
	for (uint32_t k = 0; k < B; k++)
	{
		const Plan &L = plans[idx[k]];
		pin_need = std::max<size_t>(pin_need, L.D.o_cand - L.D.o_init);
	}
	pin_need = std::max(pin_need, o_tables - o_states);
	if (int rc = grow_pinned(ctx, &sc.pin, &sc.pin_cap, pin_need, hipHostMallocDefault))
		return rc;
	unsigned char *d = sc.dev, *h = sc.pin;
	// states
	std::memset(h, 0, o_tables - o_states);
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_pgo_problem &P = problems[idx[k]];
		double *x = reinterpret_cast<double *>(h + (plans[idx[k]].D.o_state - o_states));
		for (uint32_t i = 0; i < P.n_nodes; i++)
			pgo::pose2state(P.nodes[i].pose_init, x + 7ull * i);
	}
	HIPCHK(ctx, hipMemcpyAsync(d + o_states, h, o_tables - o_states, hipMemcpyHostToDevice, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_pgo_problem &P = problems[idx[k]];
		const Plan &L = plans[idx[k]];
		const PgoDesc &D = L.D;
		const size_t base = D.o_init, len = D.o_cand - D.o_init;
		std::memset(h, 0, len);
		double *x0 = reinterpret_cast<double *>(h + (D.o_init - base));
		for (uint32_t i = 0; i < P.n_nodes; i++)
			pgo::pose2state(P.nodes[i].pose_init, x0 + 7ull * i);
		std::memcpy(h + (D.o_limit - base), L.limit.data(), 16ull * P.n_nodes);
		std::memcpy(h + (D.o_unk - base), L.unk.data(), 4ull * P.n_nodes);
		std::memcpy(h + (D.o_boxed - base), L.boxed.data(), 4ull * P.n_nodes);
		PgoEdge *E = reinterpret_cast<PgoEdge *>(h + (D.o_edges - base));
		for (uint32_t e = 0; e < D.n_edges; e++)
		{
			const mulls_pgo_edge &in = P.edges[L.used[e]];
			double x[7];
			pgo::pose2state(in.T, x);
			E[e].a = in.a, E[e].b = in.b;
			for (int c = 0; c < 3; c++)
				E[e].th[c] = x[c];
			for (int c = 0; c < 4; c++)
				E[e].qh[c] = x[3 + c];
			weight_matrix(in, prm, E[e].W);
		}
		std::memcpy(h + (D.o_adj0 - base), L.adj0.data(), 4ull * (P.n_nodes + 1));
		std::memcpy(h + (D.o_adj - base), L.adj.data(), 8ull * D.n_edges);
		std::memcpy(h + (D.o_node - base), L.node.data(), 4ull * D.n_unk);
		std::memcpy(h + (D.o_first - base), L.first.data(), 4ull * D.n_unk);
		if (D.n_unk)
			std::memcpy(h + (D.o_rowoff - base), L.rowoff.data(), 4ull * (D.n_unk + 1));
		std::memcpy(h + (D.o_colmax - base), L.colmax.data(), 4ull * D.n_unk);
		uint32_t *blkrow = reinterpret_cast<uint32_t *>(h + (D.o_blkrow - base));
		for (uint32_t u = 0; u < D.n_unk; u++)
			for (uint32_t bidx = L.rowoff[u]; bidx < L.rowoff[u + 1]; bidx++)
				blkrow[bidx] = u;
		HIPCHK(ctx, hipMemcpyAsync(d + base, h, len, hipMemcpyHostToDevice, st));
		HIPCHK(ctx, hipStreamSynchronize(st)); // (the pinned buffer is reused)
	}
	{
		PgoDesc *hd = reinterpret_cast<PgoDesc *>(h);
		for (uint32_t k = 0; k < B; k++)
			hd[k] = plans[idx[k]].D;
		HIPCHK(ctx, hipMemcpyAsync(d + o_desc, h, sizeof(PgoDesc) * (size_t)B, hipMemcpyHostToDevice, st));
	}
	HIPCHK(ctx, hipMemsetAsync(d + o_cnt, 0, 4ull * 1001u, st));
	const PgoDesc *desc = reinterpret_cast<const PgoDesc *>(d + o_desc);
	PgoRec *rec = reinterpret_cast<PgoRec *>(d + o_rec);
	uint32_t *cnt = reinterpret_cast<uint32_t *>(d + o_cnt);
	PgoOpts opt{};
	opt.delta = (double)prm.robust_delta, opt.function_tolerance = prm.function_tolerance;
	opt.robustify = prm.robustify ? 1 : 0, opt.only_translation = prm.only_limit_translation ? 1 : 0, opt.num_iterations = prm.num_iterations;
	HIPCHK(ctx, launch_pgo_reset(st, rec, B));
	HIPCHK(ctx, launch_pgo_linearize(st, desc, B, e_max, d, opt, rec));
	HIPCHK(ctx, launch_pgo_begin(st, desc, B, d, opt, rec));
	HIPCHK(ctx, hipStreamSynchronize(st)); // (the descriptors have left the pinned buffer)
	uint32_t *h_running = reinterpret_cast<uint32_t *>(h);
	for (int it = 0; it < prm.num_iterations; it++)
	{
		HIPCHK(ctx, launch_pgo_linearize(st, desc, B, e_max, d, opt, rec));
		HIPCHK(ctx, launch_pgo_assemble(st, desc, B, w_max, d, rec));
		HIPCHK(ctx, launch_pgo_factor_solve(st, desc, B, d, rec));
		HIPCHK(ctx, launch_pgo_candidate(st, desc, B, n_max, d, opt, rec));
		HIPCHK(ctx, launch_pgo_cost(st, desc, B, e_max, d, opt, rec));
		HIPCHK(ctx, launch_pgo_decide(st, desc, B, d, opt, rec, cnt + it));
		HIPCHK(ctx, hipMemcpyAsync(h_running, cnt + it, 4, hipMemcpyDeviceToHost, st));
		HIPCHK(ctx, hipStreamSynchronize(st));
		if (*h_running == 0)
			break;
	}
	// down: the records, then the states
	std::vector<PgoRec> recs(B);
	HIPCHK(ctx, hipMemcpyAsync(h, rec, sizeof(PgoRec) * (size_t)B, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	std::memcpy(recs.data(), h, sizeof(PgoRec) * (size_t)B);
	HIPCHK(ctx, hipMemcpyAsync(h, d + o_states, o_tables - o_states, hipMemcpyDeviceToHost, st));
	HIPCHK(ctx, hipStreamSynchronize(st));
	for (uint32_t k = 0; k < B; k++)
	{
		const mulls_pgo_problem &P = problems[idx[k]];
		const Plan &L = plans[idx[k]];
		mulls_pgo_result &res = results[idx[k]];
		const PgoRec &R = recs[k];
		res.status = R.status;
		res.termination = R.termination;
		res.iterations = R.iterations, res.successful_steps = R.successful;
		res.initial_cost = R.initial_cost, res.final_cost = R.cost;
		if (R.status != 1)
		{
			for (uint32_t i = 0; i < P.n_nodes; i++)
				std::memcpy(P.poses_out + 16ull * i, P.nodes[i].pose_init, 128);
		}
		else
		{
			const double *x = reinterpret_cast<const double *>(h + (L.D.o_state - o_states));
			for (uint32_t i = 0; i < P.n_nodes; i++)
				pgo::state2pose(x + 7ull * i, P.poses_out + 16ull * i);
		}
		check_edges(P, prm, res);
	}
	return MULLS_OK;
}

int pgo_run(mulls_ctx *ctx, const mulls_pgo_problem *problems, uint32_t n_problems, const mulls_pgo_params *params, uint64_t scratch_limit_bytes,
			mulls_pgo_result *results, const char *name, bool single)
{
	if (!ctx || !params || (n_problems && (!problems || !results)))
		return MULLS_E_INVALID;
	const std::string who = std::string(name) + ": ";
	if (const char *bad = check_params(*params))
	{
		ctx->err = who + bad;
		return MULLS_E_INVALID;
	}
	std::vector<Plan> plans(n_problems);
	for (uint32_t b = 0; b < n_problems; b++)
	{
		std::string msg;
		int rc = check_problem(problems[b], msg);
		if (rc == MULLS_OK)
			rc = make_plan(problems[b], *params, plans[b], msg);
		if (rc != MULLS_OK)
		{
			ctx->err = who + (single ? std::string() : "problem " + std::to_string(b) + ": ") + msg;
			return rc;
		}
	}
	const size_t limit = scratch_limit_bytes ? (size_t)scratch_limit_bytes : (size_t)MULLS_PGO_BATCH_DEFAULT_SCRATCH_BYTES;
	std::vector<uint32_t> work;
	std::vector<uint64_t> bytes; // of the problems in `work`
	for (uint32_t b = 0; b < n_problems; b++)
	{
		const mulls_pgo_problem &P = problems[b];
		Plan &L = plans[b];
		mulls_pgo_result &res = results[b];
		std::memset(&res, 0, sizeof(res));
		res.n_edges_used = (uint32_t)L.used.size();
		if (L.early)
		{
			res.status = -1;
			for (uint32_t i = 0; i < P.n_nodes; i++)
				std::memcpy(P.poses_out + 16ull * i, P.nodes[i].pose_init, 128);
			check_edges(P, *params, res);
			continue;
		}
		res.n_free = L.n_free, res.n_boxed = L.n_boxed, res.n_fixed = L.n_fixed;
		if (P.n_nodes == 0)
		{
			res.status = 1, res.termination = MULLS_PGO_TERM_NO_FREE;
			check_edges(P, *params, res);
			continue;
		}
		L.bytes = bytes_of(L, P.n_nodes);
		work.push_back(b), bytes.push_back(L.bytes);
	}
	if (work.empty())
		return MULLS_OK;
	HIPCHK(ctx, hipSetDevice(ctx->device));
	if (!ctx->pgo)
		ctx->pgo = new mulls_pgo_scratch();
	std::vector<uint32_t> cuts;
	sub_batch_cuts(bytes.data(), (uint32_t)work.size(), limit, MAX_SUB_BATCH, &cuts);
	for (size_t c = 0; c + 1 < cuts.size(); c++)
		if (int rc = run_sub_batch(ctx, problems, plans, work.data() + cuts[c], cuts[c + 1] - cuts[c], *params, results))
			return rc;
	return MULLS_OK;
}
} // namespace

extern "C"
{
	void mulls_pgo_default_params(mulls_pgo_params *p)
	{
		if (!p)
			return;
		std::memset(p, 0, sizeof(*p));
		p->num_iterations = 100;
		p->robust_delta = 1.0f;
		p->quat_tran_ratio = 1000.0f;
		p->t_limit = 2.0;
		p->r_limit = 0.05;
		p->function_tolerance = 1e-16;
		p->wrong_edge_translation_thre = 5.0f;
		p->wrong_edge_rotation_thre = 25.0f;
		p->wrong_edge_ratio_thre = 0.1f;
	}

	int mulls_pgo_optimize(mulls_ctx *ctx, const mulls_pgo_node *nodes, uint32_t n_nodes, const mulls_pgo_edge *edges, uint32_t n_edges,
						   const mulls_pgo_params *params, double *poses_out, uint8_t *edge_wrong, mulls_pgo_result *result)
	try
	{
		if (!result)
			return MULLS_E_INVALID;
		mulls_pgo_problem P;
		P.nodes = nodes, P.n_nodes = n_nodes, P.edges = edges, P.n_edges = n_edges, P.poses_out = poses_out, P.edge_wrong = edge_wrong;
		return pgo_run(ctx, &P, 1, params, 0, result, "mulls_pgo_optimize", true);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}

	int mulls_pgo_optimize_batch(mulls_ctx *ctx, const mulls_pgo_problem *problems, uint32_t n_problems, const mulls_pgo_params *params,
								 uint64_t scratch_limit_bytes, mulls_pgo_result *results)
	try
	{
		return pgo_run(ctx, problems, n_problems, params, scratch_limit_bytes, results, "mulls_pgo_optimize_batch", false);
	}
	catch (...)
	{
		return mulls::abi_caught(ctx);
	}
}
