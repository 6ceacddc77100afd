"""Live-point compaction (lds_tier.h: class_tail_flat<COMPACT>, k_reduce.hip: wave_trip): the tail of iteration 0's staged search moves a class cloud's
live points to the front of its range, the searches walk d.src_c slots from then on, and k_accum_wave maps original slots to compact records.

One rule: on the same resident batch the default run (compacting), MULLS_OPT_DEBUG_STOP = 31 (no compaction) and the host-stepped loop return the same
rows — every output field, floats as bytes — and the integer outputs are the oracle's.  The large-batch forms are forced on a handful of pairs:
ACCUM_WAVE_MIN_TRIPS = 1 (every accumulation launch is k_accum_wave's: the condition under which a run compacts), STEP_LAUNCH_MAX_PAIRS = 0,
FEW_LAUNCHES_MAX_PAIRS = 0.

The clouds are built so that every death of iteration 0 is known.  Targets are 0.5 m lattices on planes.  A source class cloud holds
  good   points 0.08 m at most (in the plane) from a lattice node of their own: they match it and stay;
  dup    points next to a node a good point already holds: under the duplicate rule (500 live points or more) one of the two vanishes;
  far    points 40 m outside the lattice (the rejection radius is 6 m): unmatched, they vanish under the same gate;
  mid    (ground and roof) points 4.5 m off the plane above nodes of their own: matched (and rejected by the distance test) while 2.5 * thr >= 4.5 m, i.e. for the first
         four iterations, then unmatched: deaths that continue after the compaction;
in a seeded random slot order.  A cloud of n >= 500 points therefore keeps exactly good + mid live points after iteration 0, and the kernels' count of the
slots taken out of the walks (MULLS_OPT_DEBUG_STOP = 20, mulls_profile.icp_search_ms[4]) must be the sum of those deaths over the compacted clouds — a number
the test works out from the geometry by brute force (removed_by_compaction; for the first four pairs it is the sum of dup + far, as constructed).  The intersection filter is off, so every staged point is a slot."""
from contextlib import contextmanager

import numpy as np
import pytest

from mulls_amd import abi, synth
from oracle import pyoracle

pytestmark = pytest.mark.gpu

GATE = 500  # live source points from which the duplicate rule and the "unmatched points vanish" rule are in force
COMPACT_MAX = 1536  # MULLS_COMPACT_MAX: the largest class cloud the one-pass walk takes, and the largest that is compacted
CLASSES = (abi.GROUND, abi.FACADE, abi.ROOF)  # three planar classes: z = -1.7, (y = 9 | x = 12), z = 5
USED = "101010"

PSETS = {
    # eight forced iterations: the mid points die in the fifth, the last ones run on a compacted cloud that shrank again
    "forced8": lambda: abi.kitti_params(dis_thre_unit=2.4, converge_translation=0.0, converge_rotation_d=0.0, max_iter_num=8, used_feature_type=USED,
                                        apply_intersection_filter=0),
    # the call site's thresholds: the pairs start from different guesses and finish at different iterations
    "converging": lambda: abi.kitti_params(dis_thre_unit=2.4, max_iter_num=20, used_feature_type=USED, apply_intersection_filter=0),
}


def lattice(cls, step=0.5):
    """(points, normals, in-plane axes) of a class's target cloud: 41 x 41 nodes per plane, 0.5 m apart, every coordinate exact in float (step 0.2: 101 x 101)"""
    ax = np.arange(-10.0, 10.0 + step / 2, step)
    u, v = [a.ravel() for a in np.meshgrid(ax, ax, indexing="ij")]
    planes = {abi.GROUND: [(2, -1.75, (0, 0, 1))], abi.ROOF: [(2, 5.0, (0, 0, 1))], abi.FACADE: [(1, 9.0, (0, -1, 0)), (0, 12.0, (-1, 0, 0))]}[cls]
    P, N, O = [], [], []
    for axis, off, normal in planes:
        o = [k for k in range(3) if k != axis]
        p = np.zeros((u.size, 3))
        p[:, o[0]], p[:, o[1]], p[:, axis] = u, v, off
        P.append(p), N.append(np.tile(np.asarray(normal, float), (u.size, 1))), O.append(np.tile([o[0], o[1], axis], (u.size, 1)))
    return np.concatenate(P), np.concatenate(N), np.concatenate(O)


def source_cloud(rng, cls, good, dup=0, far=0, mid=0):
    """the source class cloud described in the module docstring, in the target's frame; returns (points, normals)"""
    P, N, O = lattice(cls)
    n = good + dup + far + mid
    if n == 0:
        return np.zeros((0, 3)), np.zeros((0, 3))
    nodes = rng.choice(len(P), good + mid, replace=False)
    g, m = nodes[:good], nodes[good:]
    d = rng.choice(g, dup, replace=True) if dup else np.zeros(0, int)
    f = rng.choice(len(P), far, replace=True) if far else np.zeros(0, int)
    idx = np.concatenate([g, d, f, m]).astype(int)
    p, nrm, o = P[idx].copy(), N[idx], O[idx]
    rows = np.arange(n)
    # in-plane offsets of at most 0.08 m (a good point and its dups differ), guesses at most 0.1 m off: the nearest node is theirs, 0.25 m from the cell's edge
    p[rows, o[:, 0]] += rng.uniform(-0.08, 0.08, n)
    p[rows, o[:, 1]] += rng.uniform(-0.08, 0.08, n)
    k_far = np.arange(good + dup, good + dup + far)
    p[k_far, o[k_far, 0]] += np.where(p[k_far, o[k_far, 0]] < 0, -40.0, 40.0)
    k_mid = np.arange(good + dup + far, n)
    p[k_mid, o[k_mid, 2]] += 4.5 * np.where(cls == abi.FACADE, -1.0, 1.0)  # (away from the other classes' planes)
    order = rng.permutation(n)
    return p[order], nrm[order]


def make_pair(seed, spec, guess_error=None, src_shift=None, noise=0.0, dense_ground=False):
    """spec: {class: (good, dup, far, mid)}.  The source is stored a known motion away from the target frame; the guess is that motion times guess_error.
    noise: standard deviation of an error added to every source coordinate (a noisy pair takes more iterations to meet the convergence thresholds);
    dense_ground: the ground target is a 0.2 m lattice of 10 201 points — beyond the LDS tier, so that class cloud is searched on the global-memory tier"""
    rng = np.random.default_rng(seed)
    T_true = synth.se3(0.04, -0.03, 0.02, 0.001, -0.001, 0.003)
    inv = np.linalg.inv(T_true if src_shift is None else T_true @ src_shift)
    tgt, src = [None] * abi.NCLASS, [None] * abi.NCLASS
    for cls in CLASSES:
        P, N, _ = lattice(cls, 0.2 if dense_ground and cls == abi.GROUND else 0.5)
        tgt[cls] = abi.make_points(P, N, rng.uniform(0, 255, len(P)))
        p, nrm = source_cloud(rng, cls, *spec.get(cls, (0, 0, 0, 0)))
        if len(p):
            p = p + rng.normal(0, noise, p.shape) if noise else p
            src[cls] = abi.make_points(p @ inv[:3, :3].T + inv[:3, 3], nrm @ inv[:3, :3].T, rng.uniform(0, 255, len(p)))
    return abi.PairData(tgt, src, init_guess=(np.eye(4) if guess_error is None else guess_error) @ T_true)


def removed_by_compaction(pair, r=2.5 * 2.4):
    """slots the compaction takes out of the walks of a pair, from the geometry alone: in every class cloud of GATE .. COMPACT_MAX points, the points without a
    target within the rejection radius r and the points that are not the first (lowest slot) to claim their nearest target — or the whole cloud when nothing
    matches (the reference swaps such a cloud for an empty one).  Brute force in float64 on the source as the registration moves it by the guess."""
    out = 0
    for cls in CLASSES:
        n = len(pair.src[cls])
        if not GATE <= n <= COMPACT_MAX:
            continue
        s = pyoracle.transform(pair.src[cls], pair.init_guess)
        sx = np.column_stack([s["x"], s["y"], s["z"]]).astype(np.float64)
        tx = np.column_stack([pair.tgt[cls]["x"], pair.tgt[cls]["y"], pair.tgt[cls]["z"]]).astype(np.float64)
        d2 = ((sx[:, None, :] - tx[None, :, :]) ** 2).sum(axis=2)
        nearest = d2.argmin(axis=1)
        matched = d2[np.arange(n), nearest] <= r * r
        out += n - len(np.unique(nearest[matched])) if matched.any() else n
    return out


G, F, R = abi.GROUND, abi.FACADE, abi.ROOF
# (class: good, dup, far, mid) — sizes and live counts on both sides of a mask word (64), a 512-lane trip and a 1024-slot accumulation trip
SPECS = [
    {G: (65, 0, 0, 0), F: (1024, 300, 212, 0), R: (500, 300, 213, 12)},     # sizes 65 / 1536 / 1025; live 65 / 1024 / 512
    {G: (64, 0, 0, 0), F: (1025, 299, 212, 0), R: (501, 300, 212, 12)},     # sizes 64 / 1536 / 1025; live 64 / 1025 / 513
    {G: (63, 0, 0, 0), F: (1023, 301, 212, 0), R: (499, 301, 213, 12)},      # sizes 63 / 1536 / 1025; live 63 / 1023 / 511
    {G: (60, 250, 199, 4), F: (65, 500, 459, 0), R: (59, 500, 460, 4)},      # sizes 513 / 1024 / 1023; live 64 / 65 / 63
    {G: (511, 0, 0, 0), F: (350, 100, 50, 0), R: (300, 150, 50, 0)},         # 511 points, gated, none dies; exactly 500 points: gated
    {G: (300, 149, 50, 0), F: (600, 0, 0, 0)},                               # 499 points with dups and far points: not gated, none dies; no roof
    {G: (400, 50, 50, 0), F: (0, 0, 512, 0), R: (100, 0, 0, 0)},             # 512 facade points, all die (code -2 in iteration 0)
    {G: (400, 100, 12, 0), F: (900, 500, 400, 0), R: (700, 300, 500, 36)},   # sizes 512 / 1800 / 1536: the facade is beyond the one-pass walk (uncompacted)
]
# ... and a pair that ends with code -2 in iteration 0 (its source 200 m off: no correspondence at all), next to the healthy ones
FAR_SPEC = {G: (400, 100, 20, 0), F: (600, 0, 0, 0), R: (100, 0, 0, 0)}


@pytest.fixture(scope="module")
def scene():
    """the pairs (each from its own guess), what the compaction must remove from their walks, and the oracle's integer outputs per parameter set"""
    rng = np.random.default_rng(5)
    pairs, removed = [], 0
    for k, spec in enumerate(SPECS):
        # the first four pairs (the edges of SPECS) from guesses a few centimetres off, so that every point's nearest node is the one it was built on; the others
        # from decimetres off and with noisy sources (3 or 8 cm): they take more iterations to meet the convergence thresholds
        scale = (1 + k) if k < 4 else 10
        err = synth.se3(*np.clip(rng.normal(0, 0.004 * scale, 3), -0.1, 0.1), *np.deg2rad(np.clip(rng.normal(0, 0.01 * scale, 3), -0.2, 0.2)))
        pairs.append(make_pair(100 + k, spec, guess_error=err, noise=0.0 if k < 4 else (0.08 if k % 2 else 0.03)))
        removed += removed_by_compaction(pairs[-1])
        if k < 4:  # ... and the live counts after iteration 0 are the ones SPECS names
            assert removed_by_compaction(pairs[-1]) == sum(dup + far for good, dup, far, mid in spec.values() if good + dup + far + mid >= GATE)
    pairs.insert(3, make_pair(200, FAR_SPEC, src_shift=synth.se3(200.0, 0, 0)))
    removed += removed_by_compaction(pairs[3])
    want = {name: [(r.code, r.iters, tuple(r.ncorr), tuple(r.nsrc0), tuple(r.ntgt0)) for r in (pyoracle.icp(p, mk())[0] for p in pairs)] for name, mk in PSETS.items()}
    return pairs, removed, want


@contextmanager
def own_context(**options):
    from mulls_amd import lib

    c = lib.Context(0)
    try:
        for opt, v in dict(ACCUM_WAVE_MIN_TRIPS=1, STEP_LAUNCH_MAX_PAIRS=0, FEW_LAUNCHES_MAX_PAIRS=0, **options).items():
            c.set_option(getattr(abi, "OPT_" + opt), v)
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


def rows(res):
    return [(x.code, x.iters, tuple(x.ncorr), tuple(x.nsrc0), tuple(x.ntgt0), x.cropped, tuple(x.crop_box), bytes(x.T), bytes(x.info), np.float32(x.sigma).tobytes(),
             np.float32(x.confidence).tobytes(), x.singular) for x in res]


def run_with(c, b, P, stop=0, host_step=0):
    """(rows, slots the compaction removed as the kernels counted them) of one run; the options are put back"""
    c.set_option(abi.OPT_DEBUG_STOP, stop)
    c.set_option(abi.OPT_HOST_STEP, host_step)
    try:
        out = rows(b.run(P))
        return out, int(c.profile().icp_search_ms[4])
    finally:
        c.set_option(abi.OPT_DEBUG_STOP, 0)
        c.set_option(abi.OPT_HOST_STEP, 0)


def check_forms(c, b, P, want_ints, want_removed):
    """the rule of this module on one resident batch; returns the default run's rows"""
    new, _ = run_with(c, b, P)
    again, _ = run_with(c, b, P)  # the same batch a second time: the run resets src_c and the mark
    counted, removed = run_with(c, b, P, stop=20)
    former, zero = run_with(c, b, P, stop=31)
    host, _ = run_with(c, b, P, host_step=1)
    after, _ = run_with(c, b, P)  # ... and a compacting run behind runs that did not compact
    assert new == again and new == counted and new == after
    assert new == former
    assert new == host
    assert [r[:5] for r in new] == want_ints
    assert removed == want_removed and zero == 0
    return new


@pytest.mark.parametrize("pset", list(PSETS))
def test_same_bits_in_every_form(scene, pset):
    """every edge of SPECS in one batch: compacting, not compacting and host-stepped runs agree on every byte, the integers are the oracle's, and the kernels
    removed exactly the slots the construction says die in iteration 0 (nothing under MULLS_OPT_DEBUG_STOP = 31)"""
    pairs, removed, want = scene
    assert removed > 0
    with own_context() as c, resident(c, pairs) as b:
        new = check_forms(c, b, PSETS[pset](), want[pset], removed)
    bad = (3, len(new) - 2)  # the pair 200 m off and the pair whose facade cloud dies whole
    assert all(new[k][0] == -2 for k in bad) and all(r[0] == 1 for k, r in enumerate(new) if k not in bad), [r[:2] for r in new]
    if pset == "converging":
        assert len({r[1] for r in new if r[0] == 1}) > 1  # the pairs finish at different iterations


def test_first_direct_off_never_compacts(scene):
    """FIRST_DIRECT = 0: iteration 0 goes through the light pass, whose tail does not compact — same rows, nothing removed"""
    pairs, removed, want = scene
    P = PSETS["forced8"]()
    with own_context() as c, resident(c, pairs) as b:
        new, _ = run_with(c, b, P)
        c.set_option(abi.OPT_FIRST_DIRECT, 0)
        off, n_off = run_with(c, b, P, stop=20)
        c.set_option(abi.OPT_FIRST_DIRECT, 1)
        on, n_on = run_with(c, b, P, stop=20)
    assert new == off == on and [r[:5] for r in new] == want["forced8"]
    assert n_off == 0 and n_on == removed


def test_two_sub_batches_on_two_streams(scene):
    """SPLIT_MIN_PAIRS = 2: the nine pairs iterate as two sub-batches on two streams, each with its own accumulation launches"""
    pairs, removed, want = scene
    with own_context(SPLIT_MIN_PAIRS=2) as c, resident(c, pairs) as b:
        check_forms(c, b, PSETS["converging"](), want["converging"], removed)


def test_headline_kernels_on_a_large_batch(scene):
    """more than 512 class clouds: the light pass is k_cert<512, 3> (parked state, four workgroups per CU) and the heavy pass the persistent k_nn_lds — the
    bench workload's kernels.  The batch is the nine pairs 22 times over: every copy returns the nine-pair batch's rows"""
    pairs, removed, want = scene
    copies = 22
    P = PSETS["forced8"]()
    with own_context() as c:
        with resident(c, pairs) as b:
            small, _ = run_with(c, b, P)
        with resident(c, pairs * copies) as b:
            new, n_new = run_with(c, b, P, stop=20)
            former, _ = run_with(c, b, P, stop=31)
    assert new == former and new == small * copies
    assert n_new == removed * copies


def test_mixed_tier_batch(scene):
    """a pair whose ground target (10 201 points) is on the global-memory tier next to LDS-tier pairs: one launch set serves both tiers, the LDS-tier clouds are
    compacted (this pair's facade and roof among them), the global-memory cloud is not"""
    pairs, _, want = scene
    mixed = make_pair(300, {G: (300, 100, 50, 0), F: (700, 200, 100, 0), R: (400, 150, 50, 10)}, guess_error=synth.se3(0.03, -0.02, 0.01, 0.0, 0.0, 0.002), dense_ground=True)
    assert len(mixed.tgt[G]) > 9728 and len(mixed.src[G]) < GATE
    plist = pairs[:3] + [mixed]
    P = PSETS["forced8"]()
    o = pyoracle.icp(mixed, P)[0]
    ints = want["forced8"][:3] + [(o.code, o.iters, tuple(o.ncorr), tuple(o.nsrc0), tuple(o.ntgt0))]
    with own_context() as c, resident(c, plist) as b:
        new = check_forms(c, b, P, ints, sum(removed_by_compaction(p) for p in plist))
    assert new[3][0] == 1
