"""Writes tests/golden/nms_cases.npz: the expected results of the key-point non-maximum suppression where the visiting order depends on how std::sort
leaves equal keys, from the CPU harness (tests/nms_harness.cpp: upstream's record sort and sequential walk).  Per case the fixture holds the visiting order
and the kept indices, nothing else of the reference's data: the demo key points (74 and 43 equal keys) are read from tests/golden/ncc_demo.npz, at 0.25 m
and at 1.0 m; the tie-heavy synthetic clouds (tests/nms_restated.py TIE_CASES) are stored with their seeded coordinates and keys.

    python tests/golden/make_nms_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import nms_restated as nr  # noqa: E402
import test_nms  # noqa: E402


def main():
    H = test_nms.build_harness()
    out = {}
    for name, recs in test_nms.demo_keypoints().items():
        for radius in (0.25, 1.0):
            _, idx, order = H.suppress(recs, radius)
            assert np.array_equal(nr.walk(recs, order, radius), idx)
            out["%s_order" % name] = order
            out["%s_r%g_kept" % (name, radius)] = idx
            print("%-8s r %.2f  n %5d  kept %5d" % (name, radius, len(recs), len(idx)))
    for name, case in nr.TIE_CASES.items():
        xyz, keys = nr.tie_cloud(name)
        recs = nr.make_records(xyz, keys, seed=len(keys))
        _, idx, order = H.suppress(recs, case[4])
        assert np.array_equal(nr.walk(recs, order, case[4]), idx)
        out[name + "_xyz"], out[name + "_keys"], out[name + "_order"], out[name + "_kept"] = xyz, keys, order, idx
        print("%-8s r %.2f  n %5d  kept %5d  distinct keys %d" % (name, case[4], len(recs), len(idx), len(np.unique(keys))))
    np.savez_compressed(os.path.join(HERE, "nms_cases.npz"), **out)


if __name__ == "__main__":
    main()
