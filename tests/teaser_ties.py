"""Inputs with several maximum cliques for the clique search of mulls_coarse_reg_teaser (tests/test_teaser_search.py, tests/test_gpu_teaser_search.py): the
greedy bound's witness is a maximum clique here but not the lexicographically smallest one, so a search that only proves the bound's size and returns
the witness fails them, and the tasks of several roots hold a clique of the final size.  Built from teaser_restated.planted."""
import functools

import numpy as np

import teaser_restated as tr

NOISE_BOUND = 0.2


def unit(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def decoy_ties(seed):
    """N = 45: two consistent groups A and C of 12 pairs (two motions, C's sources + 500), 20 unrelated pairs (sources - 700).  Index 0 is A's first pair,
    index 1 a decoy (A's first pair, source and target each moved 7 m in independent random directions: consistent with pair 0 and nothing else), the rest
    is shuffled.  The greedy clique of vertex 0 is {0, 1}; the bound comes from a later vertex."""
    a = tr.planted(100 * seed, 12, 0.0, NOISE_BOUND, box=20.0)
    c = tr.planted(100 * seed + 1, 12, 0.0, NOISE_BOUND, box=20.0)
    o = tr.planted(100 * seed + 2, 20, 1.0, NOISE_BOUND, box=20.0)
    rng = np.random.default_rng(seed)
    decoy_t, decoy_s = a[0][:1].copy(), a[1][:1].copy()
    decoy_s[0, :3] += (7.0 * unit(rng)).astype(np.float32)
    decoy_t[0, :3] += (7.0 * unit(rng)).astype(np.float32)
    rest_t = np.concatenate([a[0][1:], c[0], o[0]])
    rest_s = np.concatenate([a[1][1:], c[1] + np.float32(500.0), o[1] - np.float32(700.0)])
    order = rng.permutation(len(rest_t))
    t = np.concatenate([a[0][:1], decoy_t, rest_t[order]])
    s = np.concatenate([a[1][:1], decoy_s, rest_s[order]])
    return np.ascontiguousarray(t, np.float32), np.ascontiguousarray(s, np.float32)


def multi(seed, G=8, k=12, n_out=32):
    """G disjoint consistent groups of k pairs (sources + 500 g), n_out unrelated pairs (sources - 700), all shuffled: G maximum cliques"""
    parts_t, parts_s = [], []
    for g in range(G):
        t, s = tr.planted(100 * seed + g, k, 0.0, NOISE_BOUND, box=20.0)[:2]
        parts_t.append(t)
        parts_s.append(s + np.float32(500.0 * g))
    t, s = tr.planted(100 * seed + G, n_out, 1.0, NOISE_BOUND, box=20.0)[:2]
    parts_t.append(t)
    parts_s.append(s - np.float32(700.0))
    t, s = np.concatenate(parts_t), np.concatenate(parts_s)
    order = np.random.default_rng(seed).permutation(len(t))
    return np.ascontiguousarray(t[order], np.float32), np.ascontiguousarray(s[order], np.float32)


def greedy_clique(adj, v):
    """what teaser_greedy_clique builds: v, then again and again the smallest vertex adjacent to all members so far"""
    cand, out = adj[v].copy(), [v]
    while cand.any():
        u = int(np.flatnonzero(cand)[0])
        out.append(u)
        cand &= adj[u]
    return sorted(out)


def greedy_bound(adj):
    """lb, the first vertex that gives it, and its clique: the witness"""
    sizes = [len(greedy_clique(adj, v)) for v in range(len(adj))]
    v = int(np.argmax(sizes))
    return sizes[v], v, greedy_clique(adj, v)


@functools.lru_cache(maxsize=None)
def tie_sets():
    """{name: (t, s, noise_bound)}"""
    out = {"decoy_ties_%d" % seed: decoy_ties(seed) + (NOISE_BOUND,) for seed in (9, 10)}
    out["multi_5"] = multi(5) + (NOISE_BOUND,)
    return out


@functools.lru_cache(maxsize=None)
def tie_case(name):
    """the numpy restatement of a tie set, its number of maximum cliques and its greedy bound, computed once"""
    t, s, nb = tie_sets()[name]
    adj = tr.graph(t, s, nb)
    r = tr.restate(t, s, nb, 8)
    lb, lb_v, witness = greedy_bound(adj)
    r.update(adj=adj, lb=lb, lb_v=lb_v, witness=witness)
    return r
