"""Every execution option of the ICP path that no other test moves away from its default (enum mulls_option, include/mulls_hip.h: "none of them changes a
result: every path returns the same bits"): CERTIFICATES, CERT_SLACK_MIN / MAX / RATE, GRID_H0, BM_H0, LDS_DEDUP, FIRST_DIRECT, SUBBATCHES, TWO_STREAMS,
SPLIT_MAX_PAIRS, LEAN_STAGING.

One rule for all of them: a form (a combination of option values) must return the default form's rows — every output field, floats as bytes — on the same
resident batch, whichever form ran before it, and the default form's rows must be the oracle's (icp_compare.compare, its tolerances, no other).  Every batch
holds healthy pairs and pairs that fail (a source 200 m off, an empty source, an empty target).

Where an option is consumed: everything but LEAN_STAGING (and STAGGER, which test_gpu_icp.py covers) is read by mulls_batch_run — init_cert and prepare_run
(batch.cpp), run_setup / launch_search / run_host_step (loop.cpp) — so one resident batch is re-run under every form; a previous form's scratch state (hints,
bounds, duplicate table, job tables) must then not leak into the next.  LEAN_STAGING is read by batch_fill of mulls_icp / mulls_icp_batch.

Did the other path run?  The profile counters that are filled without profiling events (nn_src_pts, nn_pair_evals, nn_corr_pts, nn_tgt_*, iterations;
k_finish_step and run_host_step) count LIVE points and, on the brute-force tier only, pair evaluations: none of them knows whether a point was certified or
searched, or what the cell edge was.  What does know is the diagnostic count MULLS_OPT_DEBUG_STOP = 20 / 21 switches on (mulls_profile.icp_search_ms[0] / [3],
icp_fused_ms[0] / [5]: leftover points of the light pass, class clouds its one-pass walk finished without the heavy pass; the switch adds atomics, no branch
of the search depends on it), and
launches_nn of the host-stepped loop (one per sub-batch and iteration).  Each test says which of these it asserts, or why nothing can be."""
import os
import re
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import ROOT, planes_scene, transformed_copy
from icp_compare import compare
from mulls_amd import abi, synth
from oracle import pyoracle

pytestmark = pytest.mark.gpu

PSETS = {
    # (fixed 12 iterations: the last ones move nothing, certificates get their converged iterations)
    "kitti12": lambda: abi.kitti_params(dis_thre_unit=2.4, converge_translation=0.0, converge_rotation_d=0.0, max_iter_num=12),
    "default": lambda: abi.default_params(),
    "all6": lambda: abi.default_params(used_feature_type="111111", faithful=0, rejector_strict=0),
}

# (CERTIFICATES, CERT_SLACK_MIN, CERT_SLACK_MAX, CERT_SLACK_RATE): default; off; no slack (the cube's radius is the hinted target's distance); a slack that
# follows the step without bound; a huge one (the sweep is clipped to the first-probe radius and widens from there); min > max (fminf(fmaxf(x, min), max) = max);
# a rate of a hundredth
CERT_FORMS = [(1, 0.02, 0.10, 1.0), (0, 0.02, 0.10, 1.0), (1, 0.0, 0.0, 0.0), (1, 0.0, 1000.0, 1000.0), (1, 1000.0, 1000.0, 0.0), (1, 0.5, 0.01, 1.0), (1, 0.0, 0.10, 0.01)]
CERT_GRID = [(f, k) for f in CERT_FORMS for k in (0, 1)]  # ... each with and without the k-candidate certificates


def row(x):
    return (x.code, x.iters, tuple(x.ncorr), tuple(x.nsrc0), tuple(x.ntgt0), x.cropped, tuple(x.crop_box), bytes(x.T), bytes(x.info), np.float32(x.sigma).tobytes(),
            np.float32(x.confidence).tobytes(), x.singular)  # (NaN-safe: bytes)


def rows(res):
    return [row(x) for x in res]


def trace_row(t):
    return (t.iter, tuple(t.ncorr), tuple(t.nsrc), bytes(t.thr), bytes(t.atpa), bytes(t.atpb), bytes(t.x))


@contextmanager
def own_context(nn_mode=0):
    """a context of the test's own (the session's contexts must never see one of these options), closed whatever happens"""
    from mulls_amd import lib

    c = lib.Context(0)
    try:
        c.set_nn_mode(nn_mode)
        yield c
    finally:
        c.close()


@contextmanager
def resident(c, pairs):
    b = c.batch(pairs)
    try:
        yield b
    finally:
        b.close()


def set_cert(c, form, kcert=1):
    for opt, v in zip((abi.OPT_CERTIFICATES, abi.OPT_CERT_SLACK_MIN, abi.OPT_CERT_SLACK_MAX, abi.OPT_CERT_SLACK_RATE), form):
        c.set_option(opt, v)
        assert c.get_option(opt) == v
    c.set_option(abi.OPT_KCERT, kcert)


_ORACLE = {}


def oracle(pair, pname, trace_cap=0):
    """the oracle's result of one pair, computed once per module run (the pair object is kept: its id is the key)"""
    key = (id(pair), pname, trace_cap)
    if key not in _ORACLE:
        _ORACLE[key] = (pair, pyoracle.icp(pair, PSETS[pname](), trace_cap=trace_cap))
    return _ORACLE[key][1][0]


def check_oracle(pairs, pname, res, trace_cap=0):
    """every distinct pair of the batch against the oracle; codes 1 and -2 both occur"""
    seen = set()
    for i, p in enumerate(pairs):
        if id(p) not in seen:
            seen.add(id(p))
            compare(oracle(p, pname, trace_cap), res[i], check_trace=trace_cap > 0)
    assert {1, -2} <= {r.code for r in res}


def searched_points(c, b, P, want):
    """(points the light pass's certificate left over, points searched, class clouds the one-pass walk finished without the heavy pass, class clouds the heavy
    pass took — each summed over the iterations) of one device-stepped run, counted by the kernels under MULLS_OPT_DEBUG_STOP = 20; the run returns the same rows"""
    c.set_option(abi.OPT_DEBUG_STOP, 20)
    try:
        assert rows(b.run(P)) == want
        pf = c.profile()
        return int(pf.icp_search_ms[0]), int(pf.icp_search_ms[3]), int(pf.icp_fused_ms[5]), int(pf.icp_phase_ms[4])
    finally:
        c.set_option(abi.OPT_DEBUG_STOP, 0)


# ---- the batches ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bad():
    """pairs that fail: the source 200 m off (-2), an empty source (-2), an empty target"""
    rng = np.random.default_rng(29)
    tgt = planes_scene(rng)
    far = abi.PairData(tgt, transformed_copy(tgt, synth.se3(200.0, 0, 0)))
    empty = abi.PairData(tgt, [None] * 6)
    empty_t = abi.PairData([None] * 6, transformed_copy(tgt, synth.se3(0.1, 0, 0)))
    return [far, empty, empty_t]


@pytest.fixture(scope="module")
def healthy(pairs_small):
    """the small pairs (sources of 80 - 700 points per class on targets of 300 - 3 000: both sides of the 500-point duplicate gate and of the 512-lane class walk),
    each with its own guess and with a second one: six distinct pairs"""
    rng = np.random.default_rng(31)
    out = []
    for p, T_gt in pairs_small:
        out.append(p)
        pert = synth.se3(*rng.normal(0, 0.1, 3), *np.deg2rad(rng.normal(0, 0.3, 3)))
        out.append(abi.PairData(p.tgt, p.src, init_guess=pert @ T_gt, tgt_bound=p.tgt_bound))
    return out


@pytest.fixture(scope="module")
def batch21(healthy, bad):
    """21 pairs: the six healthy ones three times over, the failing ones in between and at the end"""
    return healthy + bad[:1] + healthy + bad[1:2] + healthy + bad[2:]


def lattice_planes():
    """target class clouds on a regular 0.5 m lattice on the three planes of conftest.planes_scene (ground z = -1.7, facades y = 9 and x = 12): 41 x 41 points each,
    every coordinate exact in float"""
    ax = np.arange(-10.0, 10.25, 0.5)
    u, v = [a.ravel() for a in np.meshgrid(ax, ax, indexing="ij")]
    out = []
    for axis, off, normal in ((2, -1.7, (0, 0, 1)), (1, 9.0, (0, -1, 0)), (0, 12.0, (-1, 0, 0))):
        p = np.zeros((u.size, 3))
        o = [k for k in range(3) if k != axis]
        p[:, o[0]], p[:, o[1]], p[:, axis] = u, v, np.float32(off)
        out.append((p, np.array(normal, float), o))
    return out


def lattice_pair(seed, guess_error, n_ground=600, n_facade=350):
    """A pair whose every source point sits between two lattice neighbours of its target cloud: the midpoint, displaced in the plane by a seeded offset whose
    magnitude is spread logarithmically over 1e-7 ... 1e-2 m — the two nearest targets then differ in distance by relative amounts on both sides of the
    certificate's 1e-5 margin (0.25 m away each: 4e-7 ... 4e-2).  The source is stored in its own frame (a known motion away); the guess is that motion times
    `guess_error`."""
    rng = np.random.default_rng(seed)
    T_true = synth.se3(0.3, -0.2, 0.05, 0.004, -0.003, 0.02)
    tgt_c, src_c = [], []
    for (p, normal, o), n in zip(lattice_planes(), (n_ground, n_facade, n_facade)):
        tgt_c.append(abi.make_points(p, np.tile(normal, (len(p), 1)), rng.uniform(0, 255, len(p))))
        inner = np.nonzero((p[:, o[0]] < 10.0) & (p[:, o[1]] < 10.0))[0]
        base = p[rng.choice(inner, n, replace=False)].copy()
        along = rng.integers(0, 2, n)  # the lattice neighbour: along the first or the second in-plane axis
        base[np.arange(n), np.where(along == 0, o[0], o[1])] += 0.25
        mag, ang = 10.0 ** rng.uniform(-7.0, -2.0, n), rng.uniform(0, 2 * np.pi, n)
        base[:, o[0]] += mag * np.cos(ang)
        base[:, o[1]] += mag * np.sin(ang)
        src_c.append(abi.make_points(base, np.tile(normal, (n, 1)), rng.uniform(0, 255, n)))
    tgt = [tgt_c[0], None, np.concatenate(tgt_c[1:]), None, None, None]
    src_world = [src_c[0], None, np.concatenate(src_c[1:]), None, None, None]
    return abi.PairData(tgt, transformed_copy(src_world, np.linalg.inv(T_true)), init_guess=guess_error @ T_true)


def near_tie_share(pair, rel=1e-4):
    """share of the pair's source points whose second-nearest target is within `rel` (relative) of the nearest one's distance at iteration 0 (the guess applied
    as the registration applies it: double math, float store)"""
    n_all = n_tie = 0
    for c in range(abi.NCLASS):
        if not len(pair.src[c]) or not len(pair.tgt[c]):
            continue
        s = pyoracle.transform(pair.src[c], pair.init_guess)
        sx = np.column_stack([s["x"], s["y"], s["z"]]).astype(np.float64)
        tx = np.column_stack([pair.tgt[c]["x"], pair.tgt[c]["y"], pair.tgt[c]["z"]]).astype(np.float64)
        d = np.sqrt(((sx[:, None, :] - tx[None, :, :]) ** 2).sum(-1))
        d.partition(1, axis=1)
        n_all += len(sx)
        n_tie += int((d[:, 1] - d[:, 0] <= rel * d[:, 0]).sum())
    return n_tie / n_all


@pytest.fixture(scope="module")
def lattice():
    """two lattice pairs: `still`, whose guess is off along z only — ground sources keep their near-ties from iteration 0 on, facade sources the ones along x —
    and `turned`, whose guess is off by a small rotation and translation in every axis: its near-ties form as the steps shrink"""
    pairs = [lattice_pair(41, synth.se3(0, 0, 0.04)), lattice_pair(43, synth.se3(0.03, -0.02, 0.015, 0.002, -0.001, 0.003))]
    # the scene's preconditions (CPU only; test_certificates_on_near_ties states them): a tenth of the sources or more are near-ties at iteration 0, and the
    # oracle's two searches (kd-tree; brute force, the lowest index wins a tie) agree on it bit for bit — its own tie handling is not what is tested
    share = [near_tie_share(p) for p in pairs]
    assert share[0] >= 0.1, share
    for p in pairs:
        for pname in PSETS:
            a, b = pyoracle.icp(p, PSETS[pname](), trace_cap=24, nn_mode=0)[0], pyoracle.icp(p, PSETS[pname](), trace_cap=24, nn_mode=1)[0]
            assert row(a) == row(b) and a.trace_len == b.trace_len
            assert all(trace_row(a.trace[k]) == trace_row(b.trace[k]) for k in range(a.trace_len))
    return pairs


def device_constants():
    """the #define values of mulls_amd/csrc/device_types.h"""
    text = open(os.path.join(ROOT, "mulls_amd", "csrc", "device_types.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(MULLS_\w+)\s+\(?(\d+)u?\b", text)}


def lds_dedup_max_pts():
    """batch.cpp: lds_dedup_max_pts(), restated — the largest target class cloud whose duplicate table fits on chip next to the staged cloud.  This copy (the
    160 KiB of LDS, MULLS_LDS_AUX = 320 + 2 * MULLS_LDS_QCHUNK, the 4096-cell table, 18 B per point) must follow batch.cpp and device_types.h: when the `big`
    fixture's assertion on 7 088 fails after a change of the LDS layout, it is this copy and the fixture's 7 089-point target that want updating, not the library."""
    K = device_constants()
    qchunk = K["MULLS_LDS_QCHUNK"]
    aux = 320 + 2 * qchunk  # MULLS_LDS_AUX
    room = 160 * 1024 - 64 - K["MULLS_LDS_CELL_RESERVE"] - qchunk * 16 - aux - 2 * (4096 + 8)
    return (room // 18) & ~7


@pytest.fixture(scope="module")
def big(bad):
    """Global-memory tier: two pairs made like the zoo of test_gpu_mixed.py — small sources, a 7 089-point ground target (the first size above the on-chip duplicate
    table's limit, lds_dedup_max_pts() = 7 088) and an 11 500-point facade target (above the LDS tier's 9 728 as well) — each with a second guess, three times
    over, and the failing pairs: 15 pairs."""
    assert lds_dedup_max_pts() == 7088
    src = {abi.GROUND: 800, abi.PILLAR: 400, abi.FACADE: 1200, abi.BEAM: 200, abi.ROOF: 100}
    tgt = {abi.GROUND: 7089, abi.PILLAR: 1500, abi.FACADE: 11500, abi.BEAM: 600, abi.ROOF: 400}
    rng = np.random.default_rng(37)
    four = []
    for k in range(2):
        p, T_gt = synth.make_pair(720 + k, n_beams=128, n_az=1875, elev_deg=(-25.0, 15.0), src_counts=src, tgt_counts=tgt, vertex_count=300)
        assert len(p.tgt[abi.GROUND]) == 7089 and len(p.tgt[abi.FACADE]) == 11500
        pert = synth.se3(*rng.normal(0, 0.15, 3), *np.deg2rad(rng.normal(0, 0.3, 3)))
        four += [p, abi.PairData(p.tgt, p.src, init_guess=pert @ T_gt, tgt_bound=p.tgt_bound)]
    return four + bad[:1] + four + bad[1:2] + four + bad[2:]


# ---- 1 - 3: certificates ---------------------------------------------------------------------------------------------------------------------------------------

def run_cert_grid(c, b, pairs, pname, traced=()):
    """The default form against the oracle, then every certificate form in the order given and in reverse on the same resident batch: a form gets the same rows
    whichever form ran before it (bounds left by a run with another slack carry an older epoch and must not be believed).  traced: indices of pairs whose
    host-stepped run of every form is compared with the oracle's per-iteration traces as well."""
    P = PSETS[pname]()
    set_cert(c, CERT_FORMS[0])
    res = b.run(P)
    want = rows(res)
    check_oracle(pairs, pname, res)
    for form, kcert in CERT_GRID + CERT_GRID[::-1]:
        set_cert(c, form, kcert)
        assert rows(b.run(P)) == want, (pname, form, kcert)
    for form, kcert in CERT_GRID if traced else ():
        set_cert(c, form, kcert)
        res = b.run(P, trace_cap=24)
        assert rows(res) == want, (pname, form, kcert, "host-stepped")
        for i in traced:
            compare(oracle(pairs[i], pname, 24), res[i])
    set_cert(c, CERT_FORMS[0])
    return P, want


@pytest.mark.parametrize("nn_mode", [3, 0])
def test_certificates_off_and_slack_grid_on_the_lds_tier(batch21, nn_mode):
    """LDS tier (asked for, and chosen by auto mode): certificates off, and the sweep slack dh + clamp(rate * moved, min, max) at its edges, with and without the
    k-candidate certificates — the default form's rows, run after run in both orders, and the oracle's.

    That the other paths ran is counted by the light pass itself (MULLS_OPT_DEBUG_STOP = 20, loop stepped on the device).  Without certificates every live point
    of every light pass is left over: strictly more than with them, and the same number run after run.  Without slack a hinted search sweeps the cube whose radius is
    the hinted target's distance dh and leaves lb = min(second-smallest distance, dh) <= dh; the next certificate asks dh' + moved < lb, and the triangle
    inequality says dh' + moved >= dh: a point that was searched with a hint is searched again in the next iteration, always (only the bounds of iteration 0's
    unhinted searches, which sweep farther, let anything certify) — strictly more leftovers than at the default slack, where a searched point certifies as soon
    as the steps are shorter than the slack.  The other slack forms sweep other radii and leave other bounds: their leftover counts are printed and required to
    differ from the default's."""
    with own_context(nn_mode) as c, resident(c, batch21) as b:
        for pname in PSETS:
            P, want = run_cert_grid(c, b, batch21, pname)
            count = {}
            for form in CERT_FORMS + [CERT_FORMS[1]]:
                set_cert(c, form)
                got = searched_points(c, b, P, want)
                assert count.setdefault(form, got) == got  # (run to run)
            set_cert(c, CERT_FORMS[0])
            print(nn_mode, pname, "leftover / searched / one-pass / heavy-pass class clouds per form:", count)
            base = count[CERT_FORMS[0]]
            assert base[2] > 0 and 0 < base[1] <= base[0]
            assert count[CERT_FORMS[1]][0] > base[0] and count[CERT_FORMS[1]][1] > base[1]
            assert count[CERT_FORMS[2]][0] > base[0]
            for form in CERT_FORMS[3:]:
                assert count[form][0] != base[0], form


@pytest.mark.parametrize("nn_mode", [3, 0])
def test_certificates_on_near_ties(batch21, lattice, nn_mode):
    """Certificates where they are closest to wrong: sources halfway between two lattice targets, the two distances apart by relative amounts on both sides of the
    certificate's 1e-5 margin (lattice_pair), next to the synthetic pairs.  12 fixed iterations: the steps shrink through the range where certificates start to
    pass.  Every certificate form, device- and host-stepped: the default form's rows, the oracle's result and its per-iteration traces.

    Run on the CPU before relying on the scene: pyoracle.icp(..., nn_mode=0) (kd-tree) and nn_mode=1 (brute force, lowest index wins a tie) return identical
    rows and traces for both lattice pairs under the three parameter sets — the oracle's own tie handling is not what is tested — and the share of source points
    whose second-nearest target is within 1e-4 (relative) of the nearest at iteration 0 is 0.34 for the pair whose guess is off along z only and 0.00 for the one
    whose guess is off in every axis (its near-ties form as it converges).  The `lattice` fixture asserts both again (the share as at least one in ten)."""
    pairs = lattice + batch21
    with own_context(nn_mode) as c, resident(c, pairs) as b:
        for pname in PSETS:
            P, want = run_cert_grid(c, b, pairs, pname, traced=(0, 1))
            assert [want[0][0], want[1][0]] == [1, 1] and want[0][1] >= 3  # both lattice pairs register
            if pname == "kitti12":
                assert want[0][1] == want[1][1] == 12
            base = searched_points(c, b, P, want)
            set_cert(c, CERT_FORMS[1])
            off = searched_points(c, b, P, want)
            set_cert(c, CERT_FORMS[0])
            assert off[0] > base[0] > 0  # certificates pass on this batch, and without them they do not


@pytest.mark.parametrize("nn_mode", [0, 2])
def test_certificates_on_the_global_memory_tier(big, nn_mode):
    """k_cert_big (big_tier.h): the same certificate and the same sweep slack on the occupancy-bitmap grid, for a 7 089-point ground and an 11 500-point facade
    target — as a mixed batch (auto mode: those two class clouds on the global-memory tier, the others on the LDS tier) and with everything on the global-memory
    tier (nn_mode 2) — crossed with BIG_EARLY_SETS 0 / 5 / 1000 (class-level jobs from iteration 0 on / after five iterations / chunk-level jobs + k_filter
    throughout).  Same rows, the oracle's.

    Non-vacuity (auto mode, BIG_EARLY_SETS = 0, MULLS_OPT_DEBUG_STOP = 21: the leftover queries of the class-level jobs, mulls_profile.icp_fused_ms[0]): without
    certificates strictly more than with them; without slack strictly more than at the default slack (as on the LDS tier)."""
    with own_context(nn_mode) as c, resident(c, big) as b:
        with own_context(3) as c3:  # the fixture really is beyond the LDS tier: asking for that tier is refused
            from mulls_amd import lib

            with pytest.raises(lib.MullsError):
                c3.icp(big[0], PSETS["kitti12"]())
        for pname in PSETS:
            P = PSETS[pname]()
            want = None
            for early in (5, 0, 1000):
                c.set_option(abi.OPT_BIG_EARLY_SETS, early)
                if want is None:
                    _, want = run_cert_grid(c, b, big, pname)
                else:
                    for form, kcert in CERT_GRID:
                        set_cert(c, form, kcert)
                        assert rows(b.run(P)) == want, (pname, early, form, kcert)
                    set_cert(c, CERT_FORMS[0])
            if nn_mode == 0:
                c.set_option(abi.OPT_BIG_EARLY_SETS, 0)
                c.set_option(abi.OPT_DEBUG_STOP, 21)
                left = {}
                for form in CERT_FORMS[:3]:
                    set_cert(c, form)
                    assert rows(b.run(P)) == want
                    left[form] = int(c.profile().icp_fused_ms[0])
                c.set_option(abi.OPT_DEBUG_STOP, 0)
                set_cert(c, CERT_FORMS[0])
                print(pname, "leftover queries of the class-level jobs per form:", left)
                assert left[CERT_FORMS[1]] > left[CERT_FORMS[0]] > 0 and left[CERT_FORMS[2]] > left[CERT_FORMS[0]]
            c.set_option(abi.OPT_BIG_EARLY_SETS, 5)


# ---- 4: cell edges -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nn_mode", [3, 2])
def test_grid_cell_edge(batch21, lattice, nn_mode):
    """GRID_H0, the LDS tier's preferred cell edge: the default (1.3 m), 0.01 (clamped to 0.05), 0.05 and 0.4 (crop_grid.h grows them until the box fits the cell
    budget), 0.5 (every target of the lattice pairs on a cell face), 1.3, 7.0, 10 000 (a grid of one cell) — on the LDS tier, and on the global-memory tier,
    which does not read the option.  Same rows, the oracle's.

    Non-vacuity (nn_mode 3, MULLS_OPT_DEBUG_STOP = 20): the first-probe radius of a search is min(r, 0.999 h - 2e-4) and a hinted sweep stops there when the hint
    is farther (lds_tier.h: search_query), so the bound lb = min(second-smallest distance, swept radius) a search leaves depends on the cell edge, and with it how
    many points the next light pass cannot certify: the leftover count at 0.05 m (h grown by crop_grid.h to what the cell budget allows, still far below 1.3 m)
    and at 10 000 m (one cell: the sweep is the rejection ball) must each differ from the default's.  On the global-memory tier the option is not read: get_option
    returns what was set, and the rows come from the same resident batch under every edge in turn."""
    pairs = lattice + batch21
    with own_context(nn_mode) as c, resident(c, pairs) as b:
        for pname in PSETS:
            P = PSETS[pname]()
            res = b.run(P)
            want = rows(res)
            check_oracle(pairs, pname, res)
            for h in (0.01, 0.05, 0.4, 0.5, 1.3, 7.0, 10000.0, 0.0, 0.5, 0.05):
                c.set_option(abi.OPT_GRID_H0, h)
                assert c.get_option(abi.OPT_GRID_H0) == h
                assert rows(b.run(P)) == want, (pname, h)
                assert rows(b.run(P, trace_cap=24)) == want, (pname, h, "host-stepped")
            count = {}
            for h in (0.0, 0.05, 10000.0) if nn_mode == 3 else ():
                c.set_option(abi.OPT_GRID_H0, h)
                count[h] = searched_points(c, b, P, want)
            c.set_option(abi.OPT_GRID_H0, 0)
            if nn_mode == 3:
                print(pname, "leftover / searched / one-pass / heavy-pass class clouds per GRID_H0:", count)
                assert count[0.0][0] > 0 and count[0.05][0] != count[0.0][0] and count[10000.0][0] != count[0.0][0], (pname, count)


@pytest.mark.parametrize("nn_mode", [0, 2])
def test_bitmap_cell_edge(big, nn_mode):
    """BM_H0, one fixed cell edge for every occupancy-bitmap grid of the global-memory tier (bm_auto = 0) instead of the edge taken from the point spacing:
    0.05 (the clamp), 0.25, 0.7, 50 (one cell) against the automatic edge, mixed batch and everything on that tier.  Same rows, the oracle's.

    Non-vacuity (auto mode, BIG_EARLY_SETS = 0, MULLS_OPT_DEBUG_STOP = 21: the leftover queries of k_cert_big's class-level jobs): the swept radius, and with it
    the bound a search leaves for the next certificate, depends on the cell edge as on the LDS tier — the counts at 0.05 m and at 50 m must differ.  With
    everything on the global-memory tier (nn_mode 2) the jobs are chunk-level and nothing counts them: get_option returns what was set."""
    with own_context(nn_mode) as c, resident(c, big) as b:
        for pname in PSETS:
            P = PSETS[pname]()
            res = b.run(P)
            want = rows(res)
            check_oracle(big, pname, res)
            for h in (0.05, 0.25, 0.7, 50.0, 0.0, 0.7):
                c.set_option(abi.OPT_BM_H0, h)
                assert c.get_option(abi.OPT_BM_H0) == h
                assert rows(b.run(P)) == want, (pname, h)
            left = {}
            if nn_mode == 0:
                c.set_option(abi.OPT_BIG_EARLY_SETS, 0)
                c.set_option(abi.OPT_DEBUG_STOP, 21)
                for h in (0.0, 0.05, 50.0):
                    c.set_option(abi.OPT_BM_H0, h)
                    assert rows(b.run(P)) == want, (pname, h)
                    left[h] = int(c.profile().icp_fused_ms[0])
                c.set_option(abi.OPT_DEBUG_STOP, 0)
                c.set_option(abi.OPT_BIG_EARLY_SETS, 5)
                print(pname, "leftover queries of the class-level jobs per BM_H0:", left)
                assert min(left.values()) > 0 and left[0.05] != left[50.0], (pname, left)
            c.set_option(abi.OPT_BM_H0, 0)


def test_cell_edge_options_are_validated():
    """mulls_set_option refuses a cell edge above 1e4 m or below 0 and keeps the old value"""
    from mulls_amd import lib

    with own_context() as c:
        for opt in (abi.OPT_GRID_H0, abi.OPT_BM_H0):
            c.set_option(opt, 0.7)
            for bad_value in (10000.5, 1e5, -0.01, -1.0):
                with pytest.raises(lib.MullsError):
                    c.set_option(opt, bad_value)
                assert c.get_option(opt) == 0.7
            c.set_option(opt, 1e4)
            assert c.get_option(opt) == 1e4


# ---- 5: LDS_DEDUP = 0, FIRST_DIRECT = 0 ------------------------------------------------------------------------------------------------------------------------

TAIL_FORMS = [(1, 1), (1, 0), (0, 1), (0, 0)]  # (LDS_DEDUP, FIRST_DIRECT)
N_CU = 256  # compute units of an MI355X (launch.h: DevLaunch::n_cu, read from the device)


@pytest.mark.parametrize("size", ["3 pairs", "174 pairs"])
def test_filter_kernel_tail_and_light_first_iteration(healthy, bad, size):
    """LDS_DEDUP = 0: duplicate rule and rejection chain in k_filter instead of inside the search kernels (the general three-walk light pass, no on-chip duplicate
    table).  FIRST_DIRECT = 0: iteration 0 runs a light pass like every other iteration instead of going straight to the staged search.  Crossed with each other,
    with FEW_LAUNCHES_MAX_PAIRS 640 / 0 and with two batch sizes.  Same rows, the oracle's.

    The search's launch form is chosen by launch_nn_lds (k_search.hip) from the number of class clouds alone: light and heavy pass in one launch (k_cert_nn) up to
    2 * n_cu = 512 class clouds, k_cert + k_nn_lds beyond.  FEW_LAUNCHES_MAX_PAIRS does not enter that choice (it picks the accumulation and step launches), and
    40 pairs of at most six classes stay fused; the smallest batch of these pairs that leaves the fused form under all three parameter sets has 171 pairs (the
    KITTI set searches three classes: 3 * 171 = 513), hence 174 = 29 x the six healthy pairs, plus the failing ones.  That count is per launch: the loop stepped on
    the device runs 96 pairs and more as two sub-batches (SPLIT_MIN_PAIRS), each of which is below it again, so the large batch is also run with the split
    switched off; the host-stepped loop runs it as one sub-batch anyway.

    That the large batch runs k_cert + k_nn_lds rests on that reading of launch_nn_lds and on the 256 compute units of an MI355X, and on one count: the class
    clouds the heavy pass took (MULLS_OPT_DEBUG_STOP = 20), fewer than the same pairs give in a fused batch (see the code below).

    Non-vacuity (MULLS_OPT_DEBUG_STOP = 20): with LDS_DEDUP = 0 no workgroup takes the one-pass walk (cert_job: flat needs rp.lds_dedup) — all its counts are 0,
    and positive by default; with FIRST_DIRECT = 0 the light pass of iteration 0 leaves every live point over (no point has a hint) — strictly more leftovers
    than by default, where iteration 0 has no light pass.  Without LDS_DEDUP, FIRST_DIRECT selects nothing (loop.cpp: `first` needs rp.lds_dedup):
    (0, 1) and (0, 0) launch the same kernels."""
    pairs = healthy[:2] + bad[:1] if size == "3 pairs" else healthy * 29 + bad
    assert len(pairs) * 3 <= 2 * N_CU if size == "3 pairs" else (len(pairs) - len(bad)) * 3 > 2 * N_CU
    # (a loop stepped on the device splits 96 pairs and more into two sub-batches with a launch set each: the large batch is run that way, and as one sub-batch)
    split_mins = (96,) if size == "3 pairs" else (96, 1 << 30)
    with own_context(3) as c, resident(c, pairs) as b:
        for pname in PSETS:
            P = PSETS[pname]()
            res = b.run(P)
            want = rows(res)
            check_oracle(pairs, pname, res)
            assert want[0][1] >= 2  # iteration 0 is not the last
            count = {}
            for few in (640, 0, 640):
                c.set_option(abi.OPT_FEW_LAUNCHES_MAX_PAIRS, few)
                for dedup, direct in TAIL_FORMS + TAIL_FORMS[::-1]:
                    c.set_option(abi.OPT_LDS_DEDUP, dedup)
                    c.set_option(abi.OPT_FIRST_DIRECT, direct)
                    assert (c.get_option(abi.OPT_LDS_DEDUP), c.get_option(abi.OPT_FIRST_DIRECT)) == (dedup, direct)
                    assert rows(b.run(P, trace_cap=24)) == want, (pname, few, dedup, direct, "host-stepped")
                    for split_min in split_mins:
                        c.set_option(abi.OPT_SPLIT_MIN_PAIRS, split_min)
                        assert rows(b.run(P)) == want, (pname, few, dedup, direct, split_min)
                    got = searched_points(c, b, P, want)  # (one sub-batch)
                    assert count.setdefault((dedup, direct), got) == got
                    c.set_option(abi.OPT_SPLIT_MIN_PAIRS, 96)
            c.set_option(abi.OPT_LDS_DEDUP, 1)
            c.set_option(abi.OPT_FIRST_DIRECT, 1)
            print(size, pname, "leftover / searched / one-pass / heavy-pass class clouds per (LDS_DEDUP, FIRST_DIRECT):", count)
            assert min(count[(1, 1)]) > 0 and count[(0, 1)][:3] == count[(0, 0)][:3] == (0, 0, 0)
            assert count[(1, 0)][0] > count[(1, 1)][0]
            if size == "174 pairs":
                # did the batch leave the fused launch?  A pair's leftover lists are the same in any batch (same bits), but the light pass hands a class cloud to the
                # heavy pass beyond its own search budget: 64 points in k_cert_nn (MULLS_CERT_SMALL), 512 or 768 in k_cert.  The six healthy pairs and the failing ones
                # as one small (fused) batch, and the failing ones alone: were the large batch (run as one sub-batch) fused too, its heavy-pass count would be 29 times the healthy pairs' share
                # plus the failing ones'; launched apart, every class cloud with 65 ... 512 leftovers in some iteration stays with the light pass
                small = {}
                for name, few in (("all", healthy + bad), ("bad", bad)):
                    with resident(c, few) as b9:
                        small[name] = searched_points(c, b9, P, rows(b9.run(P)))
                fused = 29 * (small["all"][3] - small["bad"][3]) + small["bad"][3]
                print(pname, "heavy-pass class clouds: large batch", count[(1, 1)][3], "if it were fused", fused)
                assert count[(1, 1)][0] == 29 * (small["all"][0] - small["bad"][0]) + small["bad"][0]  # (the same leftovers pair by pair)
                assert count[(1, 1)][3] < fused


def test_first_iteration_of_a_mixed_batch(healthy, bad, big):
    """FIRST_DIRECT 0 / 1 where both tiers' class clouds run in one launch (k_cert_mixed: a small mixed batch in auto mode): small pairs next to the pairs with
    7 089- and 11 500-point targets.  Same rows, the oracle's.  Non-vacuity as in test_filter_kernel_tail_and_light_first_iteration: with FIRST_DIRECT = 0 the
    LDS-tier class clouds' light pass of iteration 0 leaves every live point over."""
    pairs = healthy[:2] + big[:2] + bad[:2]
    with own_context(0) as c, resident(c, pairs) as b:
        for pname in PSETS:
            P = PSETS[pname]()
            res = b.run(P)
            want = rows(res)
            check_oracle(pairs, pname, res)
            count = {}
            for direct in (1, 0, 1, 0):
                c.set_option(abi.OPT_FIRST_DIRECT, direct)
                assert c.get_option(abi.OPT_FIRST_DIRECT) == direct
                assert rows(b.run(P)) == want, (pname, direct)
                assert rows(b.run(P, trace_cap=24)) == want, (pname, direct, "host-stepped")
                got = searched_points(c, b, P, want)
                assert count.setdefault(direct, got) == got
            c.set_option(abi.OPT_FIRST_DIRECT, 1)
            print(pname, "leftover / searched / one-pass / heavy-pass class clouds per FIRST_DIRECT:", count)
            assert count[0][0] > count[1][0]


@pytest.mark.parametrize("dedup", [1, 0])
def test_stage_correspond_with_and_without_lds_dedup(dedup):
    """mulls_stage_correspond hands out the raw nearest neighbours and lets k_filter apply the chain whatever LDS_DEDUP says (stage.cpp switches it off for its
    own run and puts the caller's value back): the oracle's indices, distances and flags bit for bit under both values, which the call leaves as it found them.
    Shapes of test_gpu_stages.py on both sides of the 500-point duplicate gate and of the tile sizes."""
    rng = np.random.default_rng(1)
    with own_context(0) as c:
        c.set_option(abi.OPT_LDS_DEDUP, dedup)
        for ns, nt in ((499, 2049), (500, 2048), (3, 3), (1025, 17)):
            tx = rng.uniform(-30, 30, (nt, 3))
            tgt = abi.make_points(tx, rng.normal(size=(nt, 3)))
            sx = tx[rng.integers(0, nt, ns)] + rng.normal(0, 0.3, (ns, 3))
            sx[: ns // 10] += 50.0  # a few sources with no neighbour inside the radius
            src = abi.make_points(sx, rng.normal(size=(ns, 3)))
            m0, d0, f0 = pyoracle.correspond(src, tgt, 0.8, True, 60.0, nn_mode=1)
            m1, d1, f1 = c.correspond(src, tgt, 0.8, True, 60.0)
            assert np.array_equal(m0, m1), (ns, nt)
            assert np.array_equal(d0[m0 >= 0].view(np.uint32), d1[m0 >= 0].view(np.uint32)), (ns, nt)
            assert np.array_equal(f0, f1), (ns, nt)
            assert c.get_option(abi.OPT_LDS_DEDUP) == dedup


# ---- 6: sub-batches and streams --------------------------------------------------------------------------------------------------------------------------------

def halves(healthy, bad, n, bad_first=False):
    """n pairs whose one half is healthy and whose other half only fails: the two sub-batches of a split run finish at different iterations"""
    lo, hi = n // 2, n - n // 2
    good = [healthy[k % len(healthy)] for k in range(hi if bad_first else lo)]
    fail = [bad[k % len(bad)] for k in range(lo if bad_first else hi)]
    return fail + good if bad_first else good + fail


@pytest.mark.parametrize("n", [2, 21, 40])
def test_host_stepped_sub_batches_and_streams(healthy, bad, n):
    """The loop stepped by the host (MULLS_OPT_HOST_STEP, and every run that asks for traces) as one sub-batch, as two on one stream, as two on two streams
    (the second on ctx->stream2), and with SUBBATCHES left to the batch size (one, below 2 048 pairs): batches of 2, 21 and 40 pairs whose first half is
    healthy and whose second half fails in its first iteration, with and without traces; two streams three times in a row (the second stream leaves nothing
    behind).  The rows of the device-stepped default, the oracle's, its traces.

    Non-vacuity: launches_nn of a host-stepped run counts one search launch per sub-batch and iteration (run_host_step), so two sub-batches give the sum of the
    halves' iteration counts where one gives the batch's — asserted, with the halves' counts differing.  Nothing counts the stream a kernel ran on: for
    TWO_STREAMS, get_option returns what was set and the run has two sub-batches (SUBBATCHES = 2, n >= 2: subbatch_count)."""
    pairs = halves(healthy, bad, n)
    with own_context(3) as c, resident(c, pairs) as b:
        for pname in PSETS:
            P = PSETS[pname]()
            res = b.run(P)
            want = rows(res)
            check_oracle(pairs, pname, res)
            it_lo, it_hi = max(r.iters for r in res[: n // 2]), max(r.iters for r in res[n // 2 :])
            assert it_lo != it_hi
            c.set_option(abi.OPT_HOST_STEP, 1)
            for sub, two in ((1, 0), (2, 0), (2, 1), (2, 1), (2, 1), (0, 1), (2, 0), (1, 0)):
                c.set_option(abi.OPT_SUBBATCHES, sub)
                c.set_option(abi.OPT_TWO_STREAMS, two)
                assert (c.get_option(abi.OPT_SUBBATCHES), c.get_option(abi.OPT_TWO_STREAMS)) == (sub, two)
                for cap in (0, 24):
                    res = b.run(P, trace_cap=cap)
                    assert rows(res) == want, (pname, sub, two, cap)
                    assert c.profile().launches_nn == (it_lo + it_hi if sub == 2 else max(it_lo, it_hi)), (pname, sub, two, cap)
                    if cap:
                        check_oracle(pairs, pname, res, trace_cap=24)
            c.set_option(abi.OPT_HOST_STEP, 0)
            c.set_option(abi.OPT_SUBBATCHES, 0)
            c.set_option(abi.OPT_TWO_STREAMS, 0)


def test_device_stepped_split_window(healthy, bad):
    """The loop stepped on the device runs batches of SPLIT_MIN_PAIRS .. SPLIT_MAX_PAIRS pairs as two sub-batches on two streams: MIN = 2 and MAX = 2^30 (split),
    1 (MAX < MIN: never), 20 (just below the 21 pairs: not split), 21 (at n: split).  Same rows, the oracle's.

    Non-vacuity: launches_nn of a device-stepped run counts the search launches of the FIRST sub-batch (run_device_step).  The batch's first half only fails, in
    its first iteration: split, the first sub-batch queues at most three launch sets (it keeps two in flight and stops when the third-last reports nobody
    left); not split, the one sub-batch holds the healthy pairs and queues one per iteration of theirs."""
    pairs = halves(healthy, bad, 21, bad_first=True)
    with own_context(3) as c, resident(c, pairs) as b:
        for pname in PSETS:
            P = PSETS[pname]()
            res = b.run(P)
            want = rows(res)
            check_oracle(pairs, pname, res)
            iters = max(r.iters for r in res)
            assert max(r.iters for r in res[:10]) <= 1 and iters > 3
            c.set_option(abi.OPT_SPLIT_MIN_PAIRS, 2)
            for split_max, split in ((1 << 30, True), (1, False), (20, False), (21, True), (1, False), (1 << 30, True)):
                c.set_option(abi.OPT_SPLIT_MAX_PAIRS, split_max)
                assert c.get_option(abi.OPT_SPLIT_MAX_PAIRS) == split_max
                assert rows(b.run(P)) == want, (pname, split_max)
                launches = c.profile().launches_nn
                assert (launches <= 3) if split else (launches >= iters), (pname, split_max, launches)
            c.set_option(abi.OPT_SPLIT_MIN_PAIRS, 96)
            c.set_option(abi.OPT_SPLIT_MAX_PAIRS, 1 << 30)


# ---- 7: lean staging -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("used", ["111000", "101100", "000011", "111111"])
def test_lean_staging(healthy, bad, used):
    """LEAN_STAGING = 1 (what the C++ bridge switches on for every real caller): mulls_icp / mulls_icp_batch stage only the classes of used_feature_type, plus
    the source ground / pillar / facade clouds while the intersection box is taken from them (filter on, no undistortion).  Every output but nsrc0 / ntgt0 is the
    same bits; nsrc0 / ntgt0 are equal for the staged classes and exactly 0 for the rest.  "000011" with the filter on is the edge: the box comes from classes
    the run does not otherwise use (every pair then ends with -2 after its first search, device and oracle alike: the reference's count test asks for 20
    pillar + beam + facade correspondences; the other class sets register the healthy pairs).

    Non-vacuity: mulls_profile.stage_bytes, the bytes staged by the call (batch_fill), is strictly smaller lean than full unless every class is staged anyway."""
    pairs = healthy[:3] + bad
    with own_context(0) as c:
        for crop in (0, 1):
            for undistort in (0, 1):
                P = abi.default_params(used_feature_type=used, apply_intersection_filter=crop, apply_motion_undistortion=undistort,
                                       min_neccessary_corr_ratio=0.0 if used == "000011" else 0.03)
                box_taken = crop and not undistort
                out, staged = {}, {}
                for lean in (0, 1, 0, 1):
                    c.set_option(abi.OPT_LEAN_STAGING, lean)
                    assert c.get_option(abi.OPT_LEAN_STAGING) == lean
                    rb = c.icp_batch(pairs, P)
                    nbytes = c.profile().stage_bytes
                    r1 = [c.icp(p, P)[0] for p in pairs]
                    assert rows(rb) == rows(r1)  # the single call stages the same clouds
                    assert out.setdefault(lean, rows(rb)) == rows(rb) and staged.setdefault(lean, nbytes) == nbytes
                c.set_option(abi.OPT_LEAN_STAGING, 0)
                full = c.icp_batch(pairs, P)  # full staging reports every size: every pair against the oracle
                assert rows(full) == out[0]
                for i, p in enumerate(pairs):
                    compare(pyoracle.icp(p, P)[0], full[i], check_trace=False)
                all_staged = used == "111111"
                assert staged[1] == staged[0] if all_staged else staged[1] < staged[0], (used, crop, undistort, staged)
                for full, lean in zip(out[0], out[1]):
                    assert full[:3] + full[5:] == lean[:3] + lean[5:], (used, crop, undistort)
                    for cls in range(abi.NCLASS):
                        src_staged = used[cls] == "1" or (box_taken and cls <= 2)
                        assert lean[3][cls] == (full[3][cls] if src_staged else 0), (used, crop, undistort, cls)
                        assert lean[4][cls] == (full[4][cls] if used[cls] == "1" else 0), (used, crop, undistort, cls)
                codes = {r[0] for r in out[0]}  # (the reference's count test asks for 20 pillar + beam + facade correspondences: "000011" cannot register)
                assert codes == {-2} if used == "000011" else {1, -2} <= codes, (used, crop, undistort, codes)
