"""tests/golden/images_cases.npz: inputs made from seeds and the images tests/images_restated.py gives for them (python tests/golden/make_images_golden.py).
tests/test_images.py holds the restatement as it stands and the product's arithmetic (tests/images_harness.cpp) against the file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import images_restated as ir  # noqa: E402
from mulls_amd import abi  # noqa: E402


def cases():
    """name -> (cloud, 2-D map parameters, range image parameters)"""
    return {
        "frame": (ir.make_scan(31, 600), abi.bev_params(), abi.range_image_params()),  # the per-frame pictures of test/mulls_slam.cpp:722-733
        "export": (ir.make_scan(32, 700, offset=(12.3, -7.7, 1.0)), abi.image2d_params(m2pix=0.5, map_width=96, map_height=64, min_points_in_pix=1, max_points_in_pix=9),
                   abi.range_image_params(width=1800, height=16, f_up_deg=15.0, f_down_deg=15.0, max_distance=100.0)),
        "edges": (ir.edge_cloud(), abi.image2d_params(**ir.EDGE_MAP), abi.range_image_params(width=36, height=8)),
    }


def main():
    out = {}
    for name, (cloud, bp, rp) in cases().items():
        image, counts, info = ir.map_image(cloud, bp)
        out[name + "_in"] = cloud
        out[name + "_centre"] = info["centre"]
        out[name + "_tally"] = np.array([info["n_counted"], info["n_skipped_height"], info["n_skipped_frame"]], np.uint32)
        out[name + "_counts"], out[name + "_image"], out[name + "_range"] = counts, image, ir.range_image(cloud, rp)
    path = os.path.join(ROOT, "tests", "golden", "images_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
