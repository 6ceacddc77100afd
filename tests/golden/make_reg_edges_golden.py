"""Writes tests/golden/ndt_edges.npz and tests/golden/gicp_edges.npz: the scenes of tests/reg_edges.py with the results of the numpy restatements
(tests/ndt_restated.py, tests/gicp_restated.py).  Every cloud is stored once (cloud/<name>); a case names its clouds and the slice it takes of them
(<case>/tgt_ref, <case>/src_ref: name, first, last).  tests/test_reg_edges.py keeps the files equal to the restatements and asserts which case reaches
which edge; tests/test_gpu_reg_edges.py compares the device with them.

    python tests/golden/make_reg_edges_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import gicp_restated as gr  # noqa: E402
import ndt_restated as nr  # noqa: E402
import reg_edges  # noqa: E402
from make_gicp_golden import FLOAT_FIELDS as GICP_FLOATS, INT_FIELDS as GICP_INTS  # noqa: E402
from make_ndt_golden import FLOAT_FIELDS as NDT_FLOATS, INT_FIELDS as NDT_INTS  # noqa: E402

FILES = {"ndt": "ndt_edges.npz", "gicp": "gicp_edges.npz"}


def compute(solver):
    """-> the fixture's arrays, and per case what the restatement returned and its trace (one entry per evaluation): for the conditions"""
    clouds, cases = reg_edges.build(solver)
    out = {"names": np.array(json.dumps(list(cases)))}
    for name, P in clouds.items():
        out["cloud/" + name] = np.ascontiguousarray(P, np.float32)
    ints, floats = (NDT_INTS, NDT_FLOATS) if solver == "ndt" else (GICP_INTS, GICP_FLOATS)
    seen = {}
    for name, case in cases.items():
        c = reg_edges.resolve(clouds, case)
        trace = []
        if solver == "ndt":
            res = nr.ndt(c["tgt"], c["src"], c["tgt_bound"], c["src_bound"], c["guess"], nr.default_params(**c["prm"]), trace=trace)
        else:
            res = gr.gicp(c["tgt"], c["src"], c["tgt_bound"], c["src_bound"], c["guess"], gr.default_params(**c["prm"]), trace=trace)
        assert res is not None, name
        seen[name] = dict(res=res, trace=trace)
        out[name + "/tgt_ref"], out[name + "/src_ref"] = np.array(json.dumps(list(case["tgt"]))), np.array(json.dumps(list(case["src"])))
        out[name + "/tgt_bound"], out[name + "/src_bound"], out[name + "/guess"] = c["tgt_bound"], c["src_bound"], c["guess"]
        out[name + "/prm"] = np.array(json.dumps(c["prm"]))
        out[name + "/ints"] = np.array([res[k] for k in ints], np.int64)
        out[name + "/floats"] = np.array([res[k] for k in floats], np.float64)
        out[name + "/T"] = np.asarray(res["T"], np.float64)
    return out, seen


if __name__ == "__main__":
    for solver, file in FILES.items():
        path = os.path.join(HERE, file)
        np.savez_compressed(path, **compute(solver)[0])
        print(path, os.path.getsize(path), "bytes")
