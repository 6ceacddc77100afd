"""The comparisons of a device registration result with the oracle's (and of two device results with each other) that the GPU parity tests share:
test_gpu_icp.py, test_gpu_mixed.py, test_gpu_options.py.

Tolerances (BASELINE.json north_star): transform within 1e-4 m / 1e-4 rad.  Observed agreement is ~1e-12; the tests
pin 1e-7 so a real regression cannot hide inside the contractual tolerance.  Integer outputs (process code, iteration
count, per-iteration correspondence and live-source counts) must be identical."""
import numpy as np

from mulls_amd import synth

TOL_T, TOL_R = 1e-7, 1e-7


def compare(ro, rg, check_trace=True, x_tol=1e-9):
    assert ro.code == rg.code and ro.iters == rg.iters
    assert list(ro.ncorr) == list(rg.ncorr)
    assert list(ro.nsrc0) == list(rg.nsrc0) and list(ro.ntgt0) == list(rg.ntgt0)
    assert ro.singular == rg.singular
    assert ro.cropped == rg.cropped and list(ro.crop_box) == list(rg.crop_box)
    if np.isnan(ro.T_matrix()).any():
        # singular normal matrix: the reference lets inf/NaN propagate (SURVEY B-11); both must agree on where
        assert np.array_equal(np.isnan(ro.T_matrix()), np.isnan(rg.T_matrix()))
    else:
        dt, dr = synth.pose_error(rg.T_matrix(), ro.T_matrix())
        assert dt <= TOL_T and dr <= TOL_R, (dt, dr)
    # sigma^2 = VTPV / (n - 6) goes negative / infinite with fewer than seven observations: NaN and inf propagate in both
    assert (np.isnan(ro.sigma) and np.isnan(rg.sigma)) or ro.sigma == rg.sigma or abs(ro.sigma - rg.sigma) <= 1e-6 * max(1.0, abs(ro.sigma))
    assert ro.confidence == rg.confidence or (np.isnan(ro.confidence) and np.isnan(rg.confidence))
    io, ig = ro.info_matrix(), rg.info_matrix()
    assert np.array_equal(np.isfinite(io), np.isfinite(ig))
    if np.isfinite(io).all():
        assert np.abs(io - ig).max() <= 1e-6 * np.abs(io).max()
    if check_trace:
        assert ro.trace_len == rg.trace_len
        for k in range(ro.trace_len):
            a, b = ro.trace[k], rg.trace[k]
            assert list(a.ncorr) == list(b.ncorr) and list(a.nsrc) == list(b.nsrc), k
            assert list(a.thr) == list(b.thr)
            if any(a.atpa[:]):
                A, Bm = np.array(a.atpa[:]), np.array(b.atpa[:])
                assert np.array_equal(np.isfinite(A), np.isfinite(Bm))  # 0/0 weights etc. turn up in the same places
                fin = np.isfinite(A)
                if fin.any():
                    assert np.abs(A[fin] - Bm[fin]).max() <= 1e-10 * np.abs(A[fin]).max()
                if np.isfinite(np.array(a.x[:])).all():
                    # the solve amplifies the 1e-12 differences of the sums by the condition number of the normal matrix
                    assert np.abs(np.array(a.x[:]) - np.array(b.x[:])).max() <= x_tol * max(1.0, np.abs(np.array(a.x[:])).max())
                else:
                    assert not np.isfinite(np.array(b.x[:])).all()


def same_bits(a, b):
    return (a.code, a.iters, list(a.ncorr), list(a.nsrc0), list(a.ntgt0)) == (b.code, b.iters, list(b.ncorr), list(b.nsrc0), list(b.ntgt0)) and list(a.T[:]) == list(b.T[:]) and \
        list(a.info[:]) == list(b.info[:]) and a.sigma == b.sigma


def oracle_equal(ro, rg):
    assert (ro.code, ro.iters, list(ro.ncorr), list(ro.nsrc0), list(ro.ntgt0)) == (rg.code, rg.iters, list(rg.ncorr), list(rg.nsrc0), list(rg.ntgt0))
    dt, dr = synth.pose_error(rg.T_matrix(), ro.T_matrix())
    assert dt <= 1e-7 and dr <= 1e-7, (dt, dr)
