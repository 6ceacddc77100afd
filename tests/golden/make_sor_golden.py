"""Writes tests/golden/sor_cases.npz: the expected results of the statistical outlier removal's large cases (tests/sor_restated.py LARGE_CASES: two synthetic
scans, a real demo scan, a merged map of eight poses), mean_k 20 and std_mul 2.0, so that the device tests need neither scipy nor minutes of brute force.
The inputs are regenerated from seeds or read from tests/golden/demo_pair.npz; per case the fixture holds mean, stddev and threshold (doubles), the keep mask
as packed bits, the SHA-256 of the mean_dist bytes and the cloud's size; for one case the mean_dist array itself, to locate a mismatch.

    python tests/golden/make_sor_golden.py

A case whose keep mask differs between the double and the float reading of PCL's sqrt is refused here: take another seed."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sor_restated as sr  # noqa: E402


def main():
    out = {}
    for name, make in sr.LARGE_CASES.items():
        xyz = make(HERE)
        r = sr.restate(xyz, 20, 2.0)
        rf = sr.restate(xyz, 20, 2.0, float_sqrt=True, d2_sorted=r["d2"])
        assert np.array_equal(r["keep"], rf["keep"]), name
        out[name + "_stats"] = np.array([r["mean"], r["stddev"], r["threshold"]], np.float64)
        out[name + "_keep"] = np.packbits(r["keep"])
        out[name + "_sha"] = np.frombuffer(hashlib.sha256(r["dist"].tobytes()).digest(), np.uint8)
        out[name + "_n"] = np.array([len(xyz), int(r["keep"].sum())], np.int64)
        if name == sr.KEEPS_DIST:
            out[name + "_dist"] = r["dist"]
        print("%-6s n %8d  removed %6d  threshold %.9g  gap %.2e (float sqrt: %.2e)" % (name, len(xyz), int((~r["keep"]).sum()), r["threshold"], sr.gap(r), sr.gap(rf)))
    np.savez_compressed(os.path.join(HERE, "sor_cases.npz"), **out)


if __name__ == "__main__":
    main()
