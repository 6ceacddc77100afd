"""GPU tests of mulls_non_max_suppress_batch (include/mulls_hip.h) through the C entry point: every problem of a batch against mulls_non_max_suppress
with path = 2 on the same cloud and context, and against the restated walk (tests/nms_restated.py: suppress where the keys are distinct, walk over the
visiting order where they tie — the order itself is then the single call's, which tests/test_gpu_nms.py holds against std::sort — and the fixture
tests/golden/nms_cases.npz where it has the case).

Every comparison is equality of bytes: out, n_kept, kept_idx, order, ran.  Behind every output lies a guard slot, and outputs a call may not touch are
filled with sentinels."""
import ctypes as C
import functools

import numpy as np
import pytest

import nms_restated as nr
from mulls_amd import abi
from test_gpu_nms import random_cloud, raw_call
from test_nms import demo_keypoints, fixture, tie_records

pytestmark = pytest.mark.gpu

LIMIT = abi.NMS_LDS_MAX_POINTS
R = 0.25


class DevBuf:
    """records in device memory (the HIP runtime the library has loaded)"""

    def __init__(self, raw):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.raw, self.p = np.ascontiguousarray(raw), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), self.raw.nbytes) == 0
        assert self.hip.hipMemcpy(self.p, C.c_void_p(self.raw.ctypes.data), self.raw.nbytes, 1) == 0

    def cloud(self):
        c = abi.Cloud()
        c.pts, c.n, c.stride = self.p.value, len(self.raw), abi.POINT_BYTES
        return c

    def download(self):
        back = np.zeros_like(self.raw)
        assert self.hip.hipMemcpy(C.c_void_p(back.ctypes.data), self.p, self.raw.nbytes, 2) == 0
        return back

    def free(self):
        self.hip.hipFree(self.p)


class Problem:
    """one problem with sentinel-filled outputs and a guard slot behind each"""

    def __init__(self, recs, cap=None, idx_cap=None, order=True, stride=None, n=None):
        if isinstance(recs, DevBuf):
            self.keep, self.cloud = recs, recs.cloud()
        else:
            self.keep = recs = np.ascontiguousarray(recs)
            self.cloud = abi.Cloud()
            self.cloud.pts, self.cloud.n, self.cloud.stride = (recs.ctypes.data if recs.size else None), len(recs) if n is None else n, recs.shape[1] if stride is None else stride
        n = self.cloud.n
        self.cap, self.idx_cap, self.want_order = n if cap is None else cap, n if idx_cap is None else idx_cap, order
        self.reset()

    def reset(self):
        self.out = np.full((self.cap + 1, abi.POINT_BYTES), 0xA5, np.uint8)
        self.idx = np.full(self.idx_cap + 1, -7, np.int32)
        self.order = np.full(self.cloud.n + 1 if self.want_order else 1, -9, np.int32)

    def fill(self, p):
        p.cloud = self.cloud
        p.out, p.cap = (self.out.ctypes.data if self.cap else None), self.cap
        p.kept_idx, p.idx_cap = (self.idx.ctypes.data if self.idx_cap else None), self.idx_cap
        p.order = self.order.ctypes.data if self.want_order else None

    def untouched(self):
        return (self.out == 0xA5).all() and (self.idx == -7).all() and (self.order == -9).all()


def batch_call(ctx, problems, radius=R, path=0, limit=0, params=True):
    n = len(problems)
    arr, reps = (abi.NmsProblem * max(n, 1))(), (abi.NmsReport * max(n, 1))()
    for b, q in enumerate(problems):
        q.reset()
        q.fill(arr[b])
    C.memset(reps, 0x5A, C.sizeof(reps))
    p = abi.nms_params(radius, path)
    rc = ctx.lib.mulls_non_max_suppress_batch(ctx.h, arr, n, C.byref(p) if params else None, limit, reps)
    for q in problems:  # nothing written past the capacities, whatever the call returned
        assert (q.out[q.cap] == 0xA5).all() and q.idx[q.idx_cap] == -7 and q.order[-1] == -9
    return rc, reps


def reference(ctx, recs, radius=R):
    """(kept_idx, order, ran) of a host cloud of 48-byte records: the single call with path = 2, held against the restated walk"""
    rc, n_out, o, i, perm, rep = raw_call(ctx, recs, radius, 2)
    assert rc == abi.MULLS_OK and rep.n_kept == n_out
    idx = i[:n_out].copy()
    assert o[:n_out].tobytes() == np.ascontiguousarray(recs[idx][:, :48]).tobytes()
    if len(recs) >= 10 and len(np.unique(nr.keys_of(recs))) == len(recs):
        w_idx, w_order, ran = nr.suppress(recs, radius)
        assert ran and np.array_equal(w_order, perm) and np.array_equal(w_idx, idx)
    elif len(recs) >= 10:
        assert np.array_equal(nr.walk(recs, perm, radius), idx)
    else:
        w_idx, w_order, ran = nr.suppress(recs, radius)
        assert not ran and np.array_equal(w_idx, idx) and np.array_equal(w_order, perm)
    return idx, perm.copy(), rep.ran


def check_problem(q, rep, want, recs, path, what):
    """every output of one problem against (kept_idx, order, ran); recs: the cloud's 48-byte records on the host"""
    w_idx, w_order, ran = want
    n, nk = len(recs), len(w_idx)
    assert (rep.n_in, rep.n_kept, rep.ran) == (n, nk, ran), (what, rep.n_in, rep.n_kept, rep.ran)
    k = min(nk, q.cap)
    assert q.out[:k].tobytes() == np.ascontiguousarray(recs[w_idx[:k]][:, :48]).tobytes(), what
    assert (q.out[k:] == 0xA5).all(), what  # bytes past the kept records (and past cap) are untouched
    k = min(nk, q.idx_cap)
    assert np.array_equal(q.idx[:k], w_idx[:k]) and (q.idx[k:] == -7).all(), what
    if q.want_order:
        assert np.array_equal(q.order[:n], w_order), what
    if not ran:
        assert (rep.path, rep.rounds) == (0, 0), what
    else:
        assert rep.path == (2 if path == 2 or n > LIMIT else 1) and 1 <= rep.rounds <= n, (what, rep.path, rep.rounds)


def chain_cloud():
    xyz = np.zeros((300, 3), np.float32)
    xyz[:, 0] = (np.arange(300) * (0.9 * R)).astype(np.float32)
    recs = nr.make_records(xyz, -np.arange(300, dtype=np.float32), 3)
    return recs[np.random.default_rng(3).permutation(300)]


def cluster_cloud(m=40):
    rng = np.random.default_rng(m)
    xyz = np.concatenate([rng.uniform(-0.07, 0.07, (m, 3)) + [5.0, 5.0, 0.0], rng.uniform(-1.0, 1.0, (300, 3))]).astype(np.float32)
    return nr.make_records(xyz, rng.permutation(len(xyz)).astype(np.float32), m)


def coincident_cloud():
    rng = np.random.default_rng(8)
    sites = rng.uniform(-2, 2, (40, 3)).astype(np.float32)
    return nr.make_records(sites[rng.integers(0, 40, 700)], rng.integers(0, 3, 700).astype(np.float32), 8)


@functools.lru_cache(maxsize=None)
def mixed_clouds():
    """name -> 48-byte host records, in the order of the batch"""
    clouds = {"n0": np.zeros((0, 48), np.uint8)}
    for n in (9, 10, 1023, 1024, 1025, LIMIT - 1, LIMIT, LIMIT + 1):
        clouds["n%d" % n] = random_cloud(n, levels=0 if n % 2 else 50, half=0.1 if n < 20 else None)
    clouds.update(cluster=cluster_cloud(), chain=chain_cloud(), coincident=coincident_cloud(), tie2=tie_records("tie2"), tie64=tie_records("tie64"),
                  tie_all=tie_records("tie_all"), kpts_0=demo_keypoints()["kpts_0"], kpts_15=demo_keypoints()["kpts_15"], wide=random_cloud(1500, levels=40),
                  resident=random_cloud(2000, seed=77, levels=30), twice=random_cloud(777, seed=5))
    return clouds


REFS = {}


def ref_of(ctx, name, radius=R):
    """computed once, shared, never changed"""
    if (name, radius) not in REFS:
        idx, order, ran = reference(ctx, mixed_clouds()[name], radius)
        idx.setflags(write=False), order.setflags(write=False)
        REFS[(name, radius)] = (idx, order, ran)
    return REFS[(name, radius)]


def mixed_problems(names):
    """-> (problems, names per problem, buffers to free): `wide` at stride 64, `resident` in device memory, `twice` named by two problems"""
    clouds, probs, who, bufs = mixed_clouds(), [], [], []
    for name in names:
        recs = clouds[name]
        if name == "wide":
            w = np.random.default_rng(64).integers(0, 256, (len(recs), 64), dtype=np.uint8)
            w[:, :48] = recs
            probs.append(Problem(w))
        elif name == "resident":
            bufs.append(DevBuf(recs))
            probs.append(Problem(bufs[-1]))
        else:
            probs.append(Problem(recs))
        who.append(name)
        if name == "twice":
            probs.append(Problem(recs))  # the same array: the same (pts, n, stride)
            assert probs[-1].cloud.pts == probs[-2].cloud.pts
            who.append(name)
    return probs, who, bufs


def check_mixed(ctx, probs, who, reps, path):
    for q, name, rep in zip(probs, who, reps):
        check_problem(q, rep, ref_of(ctx, name), mixed_clouds()[name], path, (name, path))
    assert reps[0].ms_total > 0 and len({r.ms_total for r in reps[:len(probs)]}) == 1  # the wall time of the whole call, in every report


# ---------------------------------------------------------------------------------------------------------------- the mixed batch
@pytest.mark.parametrize("path", [0, 1, 2])
def test_mixed_batch(ctx_auto, path):
    names = [k for k in mixed_clouds() if not (path == 1 and k == "n%d" % (LIMIT + 1))]
    probs, who, bufs = mixed_problems(names)
    rc, reps = batch_call(ctx_auto, probs, R, path)
    assert rc == abi.MULLS_OK, ctx_auto.lib.mulls_last_error(ctx_auto.h)
    check_mixed(ctx_auto, probs, who, reps, path)
    Z = fixture()  # the cases the fixture holds at this radius
    for name, key in (("tie2", "tie2"), ("tie_all", "tie_all"), ("kpts_0", "kpts_0_r0.25"), ("kpts_15", "kpts_15_r0.25")):
        assert nr.TIE_CASES.get(name, (0, 0, 0, 0, R))[4] == R
        assert np.array_equal(ref_of(ctx_auto, name)[0], Z[key + "_kept"]) and np.array_equal(ref_of(ctx_auto, name)[1], Z[name + "_order"])
    assert ref_of(ctx_auto, "chain")[0].size == 150 and (ref_of(ctx_auto, "cluster")[0] < 40).sum() == 1
    if path != 2:
        chain = reps[who.index("chain")]
        assert 295 <= chain.rounds <= 300  # (tests/test_gpu_nms.py::test_dependency_chain has the reason)
    assert bufs[0].download().tobytes() == mixed_clouds()["resident"].tobytes()  # the input is never modified
    for b in bufs:
        b.free()


def test_fixture_radius(ctx_auto):
    """tie64 at its fixture's radius of 0.4 m, next to the demo key points at 1 m's neighbours in the fixture (a batch has one radius: a batch each)"""
    Z = fixture()
    for names, radius, keys in ((["tie64", "tie2"], nr.TIE_CASES["tie64"][4], ["tie64", None]), (["kpts_0", "kpts_15"], 1.0, ["kpts_0_r1", "kpts_15_r1"])):
        probs = [Problem(mixed_clouds()[k]) for k in names]
        rc, reps = batch_call(ctx_auto, probs, radius)
        assert rc == abi.MULLS_OK
        for q, name, key, rep in zip(probs, names, keys, reps):
            check_problem(q, rep, ref_of(ctx_auto, name, radius), mixed_clouds()[name], 0, (name, radius))
            if key:
                assert np.array_equal(q.idx[:rep.n_kept], Z[key + "_kept"]) and np.array_equal(q.order[:-1], Z[name + "_order"])


def test_problem_order_reversed(ctx_auto):
    names = ["n10", "kpts_15", "n9", "n%d" % (LIMIT + 1), "resident", "twice", "tie_all", "n0", "n1025"]
    for order in (names, names[::-1]):
        probs, who, bufs = mixed_problems(order)
        rc, reps = batch_call(ctx_auto, probs)
        assert rc == abi.MULLS_OK
        check_mixed(ctx_auto, probs, who, reps, 0)  # every problem has its own cloud's result wherever it stands
        for b in bufs:
            b.free()


def test_tiny_limit_every_problem_alone(ctx_auto):
    names = ["n10", "n1024", "resident", "twice", "n9", "n%d" % LIMIT, "n%d" % (LIMIT + 1), "wide", "chain"]
    probs, who, bufs = mixed_problems(names)
    rc, reps = batch_call(ctx_auto, probs, limit=1)
    assert rc == abi.MULLS_OK
    check_mixed(ctx_auto, probs, who, reps, 0)
    for b in bufs:
        b.free()


def test_more_workgroups_than_compute_units(ctx_auto):
    """300 clouds of 64 points in one launch: each equal to its single call"""
    clouds = [random_cloud(64, seed=1000 + b, half=0.5, levels=0 if b % 3 else 7) for b in range(300)]
    probs = [Problem(c) for c in clouds]
    rc, reps = batch_call(ctx_auto, probs)
    assert rc == abi.MULLS_OK
    kept = 0
    for b, (q, c) in enumerate(zip(probs, clouds)):
        check_problem(q, reps[b], reference(ctx_auto, c), c, 0, b)
        kept += reps[b].n_kept
    assert 300 * 5 < kept < 300 * 60


def test_truncation_and_null_outputs_per_problem(ctx_auto):
    recs = mixed_clouds()["wide"]
    want = ref_of(ctx_auto, "wide")
    nk = len(want[0])
    assert 100 < nk < 1400
    big = mixed_clouds()["n%d" % (LIMIT + 1)]
    probs = [Problem(recs, cap=50, idx_cap=7), Problem(recs, cap=0, idx_cap=0, order=False), Problem(recs, idx_cap=0), Problem(recs, cap=nk - 1, order=False),
             Problem(big, cap=50, idx_cap=0, order=False), Problem(mixed_clouds()["n9"], cap=4, idx_cap=2, order=False), Problem(recs)]
    for path in (0, 2):
        rc, reps = batch_call(ctx_auto, probs, path=path)
        assert rc == abi.MULLS_OK
        for k, q in enumerate(probs):
            src = big if k == 4 else mixed_clouds()["n9"] if k == 5 else recs
            w = ref_of(ctx_auto, "n%d" % (LIMIT + 1)) if k == 4 else ref_of(ctx_auto, "n9") if k == 5 else want
            check_problem(q, reps[k], w, src, path, (k, path))  # (bytes past cap in the sentinel-filled buffers: untouched)
    arr = (abi.NmsProblem * 1)()
    q = Problem(recs)
    q.fill(arr[0])
    p = abi.nms_params(R, 0)
    assert ctx_auto.lib.mulls_non_max_suppress_batch(ctx_auto.h, arr, 1, C.byref(p), 0, None) == abi.MULLS_OK  # no reports
    assert np.array_equal(q.idx[:nk], want[0])


# ---------------------------------------------------------------------------------------------------------------- refusals
def refused(ctx, probs, code, problem=2, **kw):
    rc, reps = batch_call(ctx, probs, **kw)
    err = ctx.lib.mulls_last_error(ctx.h).decode()
    assert rc == code, (rc, err)
    assert "problem %d" % problem in err, err
    assert all(q.untouched() for q in probs)  # no output of any problem is written
    assert bytes(reps) == bytes(C.sizeof(reps))  # every report zeroed
    return err


def test_refusals(ctx_auto):
    good = [mixed_clouds()[k] for k in ("n1025", "twice", "kpts_15")]
    base = mixed_clouds()["n1023"]

    def batch_of(bad):
        return [Problem(good[0]), Problem(good[1]), bad, Problem(good[2])]

    x = base.copy()
    x[29, 28:32] = np.frombuffer(np.float32(np.nan).tobytes(), np.uint8)
    assert "NaN" in refused(ctx_auto, batch_of(Problem(x)), abi.MULLS_E_INVALID)
    assert raw_call(ctx_auto, x)[0] == abi.MULLS_E_INVALID  # the single call's code
    for bad in (np.nan, np.inf):
        y = base.copy()
        y[137, 4:8] = np.frombuffer(np.float32(bad).tobytes(), np.uint8)
        assert "not finite" in refused(ctx_auto, batch_of(Problem(y)), abi.MULLS_E_INVALID)
        assert "not finite" in refused(ctx_auto, batch_of(Problem(y[130:139].copy())), abi.MULLS_E_INVALID)  # below the gate too
    refused(ctx_auto, batch_of(Problem(base, stride=44)), abi.MULLS_E_INVALID)
    assert raw_call(ctx_auto, base, stride=44)[0] == abi.MULLS_E_INVALID
    # more than 2^18 points: refused before anything is read (the records behind the first 1023 do not exist)
    refused(ctx_auto, batch_of(Problem(base, n=abi.NMS_MAX_POINTS + 1, cap=0, idx_cap=0, order=False)), abi.MULLS_E_UNSUPPORTED)
    # a NaN key inside a device-resident cloud: found by the key pass, the same rule; so is a non-finite coordinate there
    for col in (28, 0):
        z = base.copy()
        z[500, col:col + 4] = np.frombuffer(np.float32(np.nan).tobytes(), np.uint8)
        dev = DevBuf(z)
        refused(ctx_auto, batch_of(Problem(dev)), abi.MULLS_E_INVALID)
        refused(ctx_auto, batch_of(Problem(dev)), abi.MULLS_E_INVALID, path=2)
        refused(ctx_auto, [Problem(good[0])] + batch_of(Problem(dev))[1:], abi.MULLS_E_INVALID, limit=1)  # ... in a later sub-batch than outputs ahead of it
        dev.free()
    # path 1 with a problem beyond the one-workgroup limit; a radius that is not finite; no params
    refused(ctx_auto, batch_of(Problem(mixed_clouds()["n%d" % (LIMIT + 1)])), abi.MULLS_E_UNSUPPORTED, path=1)
    refused(ctx_auto, batch_of(Problem(good[0])), abi.MULLS_E_INVALID, problem=0, radius=float("nan"))
    refused(ctx_auto, batch_of(Problem(good[0])), abi.MULLS_E_INVALID, problem=0, params=False)
    refused(ctx_auto, batch_of(Problem(good[0])), abi.MULLS_E_INVALID, problem=0, path=3)
    # a capacity without its buffer
    q = Problem(good[0])
    arr, reps = (abi.NmsProblem * 2)(), (abi.NmsReport * 2)()
    Problem(good[1]).fill(arr[0])
    q.fill(arr[1])
    arr[1].out = None
    p = abi.nms_params(R, 0)
    assert ctx_auto.lib.mulls_non_max_suppress_batch(ctx_auto.h, arr, 2, C.byref(p), 0, reps) == abi.MULLS_E_INVALID
    assert b"problem 1" in ctx_auto.lib.mulls_last_error(ctx_auto.h)
    # the empty batch, whatever else is passed
    assert ctx_auto.lib.mulls_non_max_suppress_batch(ctx_auto.h, None, 0, C.byref(p), 0, None) == abi.MULLS_OK
    assert ctx_auto.lib.mulls_non_max_suppress_batch(ctx_auto.h, arr, 0, None, 0, reps) == abi.MULLS_OK
    # the context still works
    probs = batch_of(Problem(base))
    rc, reps = batch_call(ctx_auto, probs)
    assert rc == abi.MULLS_OK
    check_problem(probs[2], reps[2], ref_of(ctx_auto, "n1023"), base, 0, "after the refusals")


# ---------------------------------------------------------------------------------------------------------------- reuse and the Python layer
def test_reuse_and_arena_growth(ctx_auto):
    """batch, single, a larger batch, the first batch again on one context: the same bytes each time, and the arena only grows"""
    arena = ctx_auto.lib.mulls_nms_batch_arena_bytes
    small, large = ["n10", "tie2", "n1024"], ["kpts_0", "n%d" % LIMIT, "n10", "tie2", "n1024", "kpts_15", "n%d" % (LIMIT - 1), "wide"]
    sizes = []
    for names in (small, None, large, small):
        if names is None:
            assert np.array_equal(raw_call(ctx_auto, mixed_clouds()["tie2"], R, 1)[3][:len(ref_of(ctx_auto, "tie2")[0])], ref_of(ctx_auto, "tie2")[0])
        else:
            probs, who, _ = mixed_problems(names)
            rc, reps = batch_call(ctx_auto, probs)
            assert rc == abi.MULLS_OK
            check_mixed(ctx_auto, probs, who, reps, 0)
        sizes.append(arena(ctx_auto.h))
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[3] == sizes[2]
    need = sum(48 * 2 * len(mixed_clouds()[k]) for k in large)
    from mulls_amd import lib

    fresh = lib.Context(0)
    assert arena(fresh.h) == 0
    probs, who, _ = mixed_problems(large)
    rc, reps = batch_call(fresh, probs)
    assert rc == abi.MULLS_OK and need < arena(fresh.h) < 3 * need  # sized by what the batch holds
    check_mixed(ctx_auto, probs, who, reps, 0)
    fresh.close()


def test_python_layer(ctx_auto):
    names = ["kpts_15", "n9", "n0", "twice", "twice", "n%d" % (LIMIT + 1)]
    clouds = [mixed_clouds()[k] for k in names]
    for path in (0, 2):
        res = ctx_auto.non_max_suppress_batch(clouds, R, path)
        assert len(res) == len(names)
        for name, c, (kept, idx, order, rep) in zip(names, clouds, res):
            one = ctx_auto.non_max_suppress(c, R, 2)
            assert kept.tobytes() == one[0].tobytes() and np.array_equal(idx, one[1]) and np.array_equal(order, one[2]), (name, path)
            assert (rep.n_in, rep.n_kept, rep.ran) == (one[3].n_in, one[3].n_kept, one[3].ran)
            assert np.array_equal(idx, ref_of(ctx_auto, name)[0])
    assert ctx_auto.non_max_suppress_batch([]) == []
    assert ctx_auto.non_max_suppress_batch(clouds[:2], scratch_limit_bytes=1)[0][3].n_kept == 851
