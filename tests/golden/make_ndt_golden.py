"""Writes tests/golden/ndt_cases.npz: the scenes of tests/ndt_scenes.py with the results of the numpy restatement (tests/ndt_restated.py).
tests/test_ndt.py keeps the file equal to the restatement; tests/test_gpu_ndt.py compares the device with it.

    python tests/golden/make_ndt_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import ndt_restated as nr  # noqa: E402
import ndt_scenes  # noqa: E402

INT_FIELDS = ("code", "iterations", "evaluations", "converged", "n_leaves", "n_leaves_used", "n_src", "n_tgt", "line_search_reversals", "inner_steps")
FLOAT_FIELDS = ("fitness", "trans_probability", "gauss_d1", "gauss_d2", "gauss_d3")


def compute():
    cases, _ = ndt_scenes.build_cases()
    out = {"names": np.array(json.dumps(list(cases)))}
    for name, c in cases.items():
        res = nr.ndt(c["tgt"], c["src"], c["tgt_bound"], c["src_bound"], c["guess"], nr.default_params(**c["prm"]))
        out[name + "/tgt"], out[name + "/src"] = c["tgt"], c["src"]
        out[name + "/tgt_bound"], out[name + "/src_bound"], out[name + "/guess"] = c["tgt_bound"], c["src_bound"], c["guess"]
        out[name + "/prm"] = np.array(json.dumps(c["prm"]))
        out[name + "/ints"] = np.array([res[k] for k in INT_FIELDS], np.int64)
        out[name + "/floats"] = np.array([res[k] for k in FLOAT_FIELDS], np.float64)
        out[name + "/T"] = np.asarray(res["T"], np.float64)
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "ndt_cases.npz")
    np.savez_compressed(path, **compute())
    print(path, os.path.getsize(path), "bytes")
