"""GPU tests of the device clique search of mulls_coarse_reg_teaser / mulls_coarse_reg_teaser_indexed (MULLS_OPT_TEASER_DEVICE_SEARCH = 1: k_teaser_clique.hip,
the scheme of mulls_amd/csrc/teaser_search.h that tests/test_teaser_search.py runs on the CPU), on a context of this module's own so that the option never
reaches the shared fixtures.

Every comparison is equality, as in tests/test_gpu_teaser.py: the search returns the lexicographically smallest maximum clique, which no order of the search
can change, and everything behind the clique is unchanged code — so status, n_edges, max_core, clique_size, clique_exact, gnc_iterations, both inlier counts,
the clique list and every bit of cost and T equal the fixture (tests/golden/teaser_cases.npz), the numpy restatement (the tie inputs of tests/teaser_ties.py)
or the host search on the same context.  clique_nodes is the effort of all workers together; with the option on it depends on when workers see each other's
bounds and is not compared."""
import numpy as np
import pytest

import teaser_restated as tr
import teaser_ties as tt
from mulls_amd import abi, lib
from test_gpu_teaser import assert_same, device
from test_teaser import demo, fixture_case, input_sets

pytestmark = pytest.mark.gpu
OPT = abi.OPT_TEASER_DEVICE_SEARCH


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    c.set_option(OPT, 1)
    yield c
    c.close()


def same_bits(a, b, what):
    assert_same(a, b, what)
    assert a["clique_size"] == len(a["clique"])


@pytest.mark.parametrize("name", sorted(tr.input_sets(None)) + ["demo_%s_nb%d" % (n, b) for n in tr.DEMO_LISTS for b in (25, 100)])
def test_device_search_equals_restatement(ctx, name):
    """the sets of test_gpu_teaser.py::test_device_equals_restatement: sizes 31 .. 65, 1023 .. 1025, 4097 and 8192 (7 934 kept vertices, W = 124), a complete
    graph of 300 (a stack 300 deep), two maximum cliques, no edge, a single edge, the planted sets and the demo lists (where the bound is below the size)"""
    assert ctx.get_option(OPT) == 1
    t, s, nb = input_sets()[name]
    want = fixture_case(name)
    assert want["clique_exact"] == 1
    same_bits(device(ctx, t, s, nb, tr.min_inlier(name)), want, name)


@pytest.mark.parametrize("name", ["decoy_ties_9", "decoy_ties_10", "multi_5"])
def test_tie_inputs(ctx, name):
    """several maximum cliques, and the greedy witness is one of them but not the smallest: the bound's size is already the answer's, the list is not"""
    t, s, nb = tt.tie_sets()[name]
    want = tt.tie_case(name)
    assert want["lb"] == want["clique_size"] == 12 and want["n_maximum_cliques"] == (8 if name == "multi_5" else 2)
    if name != "multi_5":
        assert want["witness"] != list(want["clique"])
    same_bits(device(ctx, t, s, nb), want, name)


def gathered(name, nb):
    Z = demo()
    a, b = (0, 15) if name.endswith("0_15") else (15, 0)
    pr = Z[name + "_pairs"]
    return Z["kpts_%d" % a], Z["kpts_%d" % b], pr


@pytest.mark.parametrize("name,n", [("fixed2000_0_15", 1543), ("fixed2000_15_0", 1538)])
def test_same_context_host_and_device(ctx, name, n):
    """the 2000-per-scan pair lists at 0.25 m (the host search takes 5 - 6 k nodes): option 1 against option 0, the unchanged host search, on one context"""
    kt, ks, pr = gathered(name, 0.25)
    assert len(pr) == n
    try:
        on = device(ctx, kt[pr[:, 0]], ks[pr[:, 1]], 0.25)
        ctx.set_option(OPT, 0)
        off = device(ctx, kt[pr[:, 0]], ks[pr[:, 1]], 0.25)
    finally:
        ctx.set_option(OPT, 1)
    assert off["clique_exact"] == 1 and 1000 < off["clique_nodes"] < 20000
    same_bits(on, off, name)
    assert on["clique_nodes"] >= 1


def test_repeats_and_context_state(ctx):
    """twice in a row the same bits; a small set after the largest after a small set (the grow-only scratch keeps nothing of the call before); the option
    switched 1 -> 0 -> 1 between calls; with the option at 0, clique_nodes is the host's count (which repeats)"""
    for name in ("size_31", "size_8192", "size_31", "complete_300", "single_edge", "demo_recip_15_0_nb100", "size_33"):
        t, s, nb = input_sets()[name]
        a, b = device(ctx, t, s, nb), device(ctx, t, s, nb)
        same_bits(a, fixture_case(name), name)
        same_bits(b, fixture_case(name), name)
    t, s, nb = input_sets()["demo_recip_15_0_nb100"]
    want = fixture_case("demo_recip_15_0_nb100")
    fresh = lib.Context(0)  # a default context: the host search's count
    try:
        assert fresh.get_option(OPT) == 0
        host_nodes = device(fresh, t, s, nb)["clique_nodes"]
    finally:
        fresh.close()
    try:
        for value in (1, 0, 1, 0, 1):
            ctx.set_option(OPT, value)
            assert ctx.get_option(OPT) == value
            got = device(ctx, t, s, nb)
            same_bits(got, want, value)
            if value == 0:
                assert got["clique_nodes"] == host_nodes
    finally:
        ctx.set_option(OPT, 1)


def test_budget_gives_the_greedy_witness(ctx):
    """251 kept roots are more than 50 nodes: every run is abandoned, and an abandoned search returns the greedy bound's witness whatever the workers did"""
    t, s, nb = input_sets()["demo_recip_15_0_nb100"]
    lb, lb_v, witness = tt.greedy_bound(tr.graph(t, s, nb))
    runs = [device(ctx, t, s, nb, budget=50) for _ in range(3)]
    for r in runs:
        assert r["clique_exact"] == 0 and r["clique_nodes"] > 50
        assert list(r["clique"]) == witness and r["clique_size"] == lb
        assert r["T"].tobytes() == runs[0]["T"].tobytes() and np.float64(r["cost"]).tobytes() == np.float64(runs[0]["cost"]).tobytes()
    same_bits(device(ctx, t, s, nb), fixture_case("demo_recip_15_0_nb100"), "after a budget exit")


def test_option_validation(ctx):
    for start in (1, 0, 1):
        ctx.set_option(OPT, start)
        for bad in (2, -1, 0.5, float("nan")):
            with pytest.raises(lib.MullsError):
                ctx.set_option(OPT, bad)
            assert ctx.get_option(OPT) == start
    fresh = lib.Context(0)
    try:
        assert fresh.get_option(OPT) == 0  # the default is the host search
    finally:
        fresh.close()


def test_indexed_entry_point(ctx):
    Z = demo()
    pr = Z["recip_0_15_pairs"]
    for nb in (0.25, 1.0):
        want = fixture_case("demo_recip_0_15_nb%d" % int(100 * nb))
        same_bits(device(ctx, Z["kpts_0"], Z["kpts_15"], nb, tgt_idx=pr[:, 0], src_idx=pr[:, 1]), want, ("indexed", nb))

