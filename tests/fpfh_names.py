"""The names the FPFH / SAC-IA tests share (tests/test_fpfh.py, tests/test_gpu_fpfh.py, tests/golden/make_fpfh_golden.py): the fixture, its cases in
order, and the result fields it records.  Nothing is imported here, so the GPU tests need nothing but the fixture."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fpfh_cases.npz")
FPFH_CASES = ["one", "two", "three", "duplicates", "normals", "radius_edge", "sizes", "bin_edges", "dense_table"]
SAC_CASES = ["sac_default", "sac_three", "sac_few_targets", "sac_equal_descriptors", "sac_halving", "sac_it1", "sac_it64", "sac_it65", "sac_chunks", "sac_equal_error",
             "sac_threshold_truncated", "sac_threshold_huber", "sac_nan_errors", "sac_huber", "sac_recovery"]
INT_FIELDS = ("best_iteration", "iterations", "n_src", "n_tgt")
FLOAT_FIELDS = ("best_error", "fitness")
