"""Writes tests/golden/fpfh_batch_cases.npz: the scenes of the batched SAC-IA tests (mulls_coarse_reg_fpfhsac_batch), each a list of problems under one
set of parameters, with the result of the numpy restatement (tests/fpfh_restated.py) called once per problem.  Every cloud is one of
tests/golden/fpfh_cases.npz, so this file records only the parameters, which cloud of which case is a problem's target and source, and the expected
ints, floats and T per problem.  tests/test_fpfh_batch.py keeps the file equal to the restatement; tests/test_gpu_fpfh_batch.py compares the device with it.

    python tests/golden/make_fpfh_batch_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import fpfh_restated as fr  # noqa: E402
from fpfh_names import FLOAT_FIELDS, GOLDEN, INT_FIELDS  # noqa: E402

BATCH_GOLDEN = os.path.join(HERE, "fpfh_batch_cases.npz")
MIXED = dict(search_radius=0.4, max_iterations=65, max_correspondence_distance=0.25, k_correspondences=15, seed=11)  # 65: one lane past a wave


def own(name):
    """a case's own pair: (target, source), each (case, which of its clouds)"""
    return ((name, "tgt"), (name, "src"))


def scenes(g):
    """name -> (params, [(target, source), ...]); g: the single calls' fixture, whose cases' parameters some scenes take"""
    prm = lambda name: json.loads(str(g[name + "/prm"]))
    t80 = ("sac_it64", "tgt")  # the 80-point target
    return {
        # sizes 3/80, 8/24, 30/7 (k_eff = 7 beside 15), 60/80 and 10/20
        "mixed": (MIXED, [own(n) for n in ("sac_three", "sac_chunks", "sac_few_targets", "sac_it64", "sac_equal_descriptors")]),
        # 3 x 1 030 hypotheses: the stretches of 1 024 slots begin and end inside problems
        "chunks": (prm("sac_chunks"), [own(n) for n in ("sac_chunks", "sac_it64", "sac_halving")]),
        # one target against four sources, the first and the last the same cloud; then that target as a source against one of its sources as the target
        "shared": (MIXED, [(t80, ("sac_it64", "src")), (t80, ("sac_three", "src")), (t80, ("sac_halving", "src")), (t80, ("sac_it64", "src")), (("sac_it64", "src"), t80)]),
        # upstream's settings: the infinite range, hypothesis 0 wins
        "default": (prm("sac_default"), [own(n) for n in ("sac_default", "sac_few_targets", "sac_halving")]),
        "nan": (prm("sac_nan_errors"), [own(n) for n in ("sac_nan_errors", "sac_equal_descriptors")]),
        "huber": (prm("sac_huber"), [own(n) for n in ("sac_huber", "sac_three")]),
    }


SCENES = ("mixed", "chunks", "shared", "default", "nan", "huber")


def cloud_of(g, ref):
    case, which = ref
    return g["%s/%s" % (case, which)], g["%s/%s_nrm" % (case, which)]


def compute():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    out = {"scenes": np.array(json.dumps(list(SCENES)))}
    for name, (prm, problems) in scenes(g).items():
        out[name + "/prm"] = np.array(json.dumps(prm))
        out[name + "/problems"] = np.array(json.dumps(problems))
        ints, floats, poses = [], [], []
        for tgt, src in problems:
            (T, Tn), (S, Sn) = cloud_of(g, tgt), cloud_of(g, src)
            res = fr.fpfhsac(T, Tn, S, Sn, fr.fpfhsac_default_params(**prm))
            ints.append([res[k] for k in INT_FIELDS]), floats.append([res[k] for k in FLOAT_FIELDS]), poses.append(np.asarray(res["T"], np.float64))
        out[name + "/ints"], out[name + "/floats"], out[name + "/T"] = np.array(ints, np.int64), np.array(floats, np.float64), np.array(poses, np.float64)
    return out


if __name__ == "__main__":
    np.savez_compressed(BATCH_GOLDEN, **compute())
    print(BATCH_GOLDEN, os.path.getsize(BATCH_GOLDEN), "bytes")
