"""Writes tests/golden/ransac_cases.npz: what tests/ransac_restated.py returns on every input set the GPU tests of mulls_coarse_reg_ransac reuse, so that the
restatement cannot drift unnoticed (tests/test_ransac.py recomputes and compares) and the GPU tests need not recompute it.  Made from this repository's
restatement only.  Per case `<set>_i<max_iter>_r<refine>`: _res = status, iterations, best_iteration, refine_iterations, n_inliers; _T = the 4 x 4; _inl = the
inlier mask, bit-packed.  Per set: _sha = SHA-1 of the generated input arrays (the generators' streams are pinned with the results).

    python tests/golden/make_ransac_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ransac_restated as rr  # noqa: E402


def sha(t, s):
    return np.frombuffer(hashlib.sha1(np.ascontiguousarray(t).tobytes() + np.ascontiguousarray(s).tobytes()).digest(), np.uint8)


def pack(r, n):
    mask = np.zeros(n, bool)
    mask[r["inliers"]] = True
    res = np.array([r["status"], r["iterations"], r["best_iteration"], r["refine_iterations"], r["n_inliers"]], np.int64)
    return res, np.asarray(r["T"], np.float64), np.packbits(mask)


def main():
    out, names = {}, []
    for name, (t, s, bound, iters) in rr.input_sets(np.load(os.path.join(HERE, "ncc_demo.npz"))).items():
        out[name + "_sha"] = sha(t, s)
        for (it, rf), r in rr.restate_set(t, s, bound, iters).items():
            case = rr.case_name(name, it, rf)
            out[case + "_res"], out[case + "_T"], out[case + "_inl"] = pack(r, len(t))
            names.append(case)
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "ransac_cases.npz"), **out)
    print(len(names), "cases")


if __name__ == "__main__":
    main()
