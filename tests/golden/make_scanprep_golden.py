"""Writes tests/golden/scanprep_cases.npz: a few cases of the scan preparation (tests/scanprep_restated.py) — the input records, regenerated from their seeds
by scanprep_restated.make_scan, and what the restatement makes of them: the kept records and the counts (after the dist filter, after the thinning).

    python tests/golden/make_scanprep_golden.py

A seed for which a point lies within 4 float ulps of a dist limit is refused (scanprep_restated.make_case): take another."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import scanprep_restated as sr  # noqa: E402
from mulls_amd import abi  # noqa: E402


def cases():
    """name -> (seed, n, params)"""
    C = abi.SCAN_CHUNK
    kitti = dict(calib_on=1, dist_filter_on=1, vertical_ang_correction_deg=0.195, min_dist=2.0, max_dist=80.0)
    return {
        "frame_loop": (301, 3 * C + 7, abi.scan_prep_params(calib_first=0, **kitti)),
        "export_stamps": (302, 2 * C + 1, abi.scan_prep_params(calib_first=1, downsample_ratio=5, timestamp_mode=1, **kitti)),
        "export_azimuth": (303, C + 1, abi.scan_prep_params(calib_first=1, downsample_ratio=2, timestamp_mode=2, scan_begin_ang_deg=90.0, **kitti)),
        "negate_z": (304, C - 1, abi.scan_prep_params(calib_on=1, vertical_ang_correction_deg=180.0, downsample_ratio=8, timestamp_mode=2)),
    }


def main():
    out = {}
    for name, (seed, n, p) in cases().items():
        scan = sr.make_case(seed, n, p)
        want, info = sr.prepare(scan, p)
        out[name + "_in"], out[name + "_out"] = scan, want
        out[name + "_counts"] = np.array([info["n_after_dist"], info["n_out"]], np.int64)
    path = os.path.join(HERE, "scanprep_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
