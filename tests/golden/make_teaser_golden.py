"""Writes tests/golden/teaser_cases.npz: the results of tests/teaser_restated.py (the numpy restatement of mulls_coarse_reg_teaser's definition) on every
input set of teaser_restated.input_sets — the demo key-point pair lists recip / fixed300 of both directions at the noise bounds 0.25 and 1.0, the planted
sets, the word- and wave-edge sizes up to 8192 pairs and the scripted edge cases.

It is made from the restatement: no TEASER++ exists where this project is built and tested, so there is nothing of TEASER++ to record.  The fixture pins
the restatement (tests/test_teaser.py) and spares the GPU tests its run time (tests/test_gpu_teaser.py).

    python tests/golden/make_teaser_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import teaser_restated as tr  # noqa: E402

INT_KEYS = ("status", "n_edges", "max_core", "clique_size", "clique_exact", "gnc_iterations", "n_rotation_inliers", "n_translation_inliers", "gnc_exit",
            "n_maximum_cliques")


def sha(t, s):
    return np.frombuffer(hashlib.sha1(np.ascontiguousarray(t).tobytes() + np.ascontiguousarray(s).tobytes()).digest(), np.uint8)


def main():
    demo = np.load(os.path.join(HERE, "ncc_demo.npz"))
    out = {}
    sets = tr.input_sets(demo)
    for name, (t, s, nb) in sets.items():
        r = tr.restate(t, s, nb, tr.min_inlier(name))
        out[name + "_sha"] = sha(t, s)
        out[name + "_res"] = np.array([r[k] for k in INT_KEYS], np.int64)
        out[name + "_T"] = r["T"]
        out[name + "_cost"] = np.float64(r["cost"])
        out[name + "_clique"] = r["clique"].astype(np.int32)
        print(name, len(t), dict(zip(INT_KEYS, out[name + "_res"].tolist())))
    out["cases"] = np.array(sorted(sets))
    path = os.path.join(HERE, "teaser_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
