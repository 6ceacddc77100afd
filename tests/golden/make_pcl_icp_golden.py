"""Writes tests/golden/pcl_icp_cases.npz: the scenes of tests/pcl_icp_scenes.py with the results of the numpy restatement (tests/pcl_icp_restated.py),
and recorded inputs and outputs of its pieces (math/...: normals, one pair's plane terms, both steps, the loop's state over a whole run) for the host
harness.  A cloud that several cases share is stored once (cloud/<k>; <case>/tgt_id and <case>/src_id name it).  tests/test_pcl_icp.py keeps the file
equal to the restatement; tests/test_gpu_pcl_icp.py compares the device with it.

    python tests/golden/make_pcl_icp_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import pcl_icp_restated as pr  # noqa: E402
import pcl_icp_scenes  # noqa: E402

INT_FIELDS = ("code", "iterations", "converged", "stop", "n_src", "n_tgt", "n_corr", "n_fit")
FLOAT_FIELDS = ("fitness", "mse")
MATH_CASES = ("street", "street_plane", "crafted_plane")


def cloud_of(z, name, which):
    """the fixture's cloud of a case: which = "tgt" or "src\""""
    return z["cloud/%d" % int(z["%s/%s_id" % (name, which)])]


def math_records(res, trace, prm):
    out = {}
    metric = prm["metrics"]
    tgt = res["tgt_c"]
    if metric == pr.POINT2PLANE:
        flat, want = [], []
        for i in list(range(30)) + list(range(len(tgt) - 10, len(tgt))):
            nb = pr.neighbourhood(tgt, i, prm["neighbor_radius"])
            flat += [float(len(nb))] + [float(v) for v in tgt[i]] + [float(v) for v in tgt[nb].astype(np.float64).reshape(-1)]
            want.append([float(v) for v in pr.point_normal(tgt[nb].astype(np.float64), tgt[i])])
        out["normal_in"], out["normal_out"] = np.array(flat, np.float64), np.array(want, np.float64)
        match, d2 = pr.correspondences(res["src_c"], tgt, prm["dis_thre_unit"], prm["use_reciprocal_correspondence"])
        sel = np.flatnonzero(match >= 0)[:30]
        s, t, n = res["src_c"][sel].astype(np.float64), tgt[match[sel]].astype(np.float64), res["normals"][match[sel]].astype(np.float64)
        out["term_in"], out["term_out"] = np.concatenate([s, t, n], axis=1), pr.plane_terms(s, t, n)
        steps = np.array([tr[0][:27] for tr in trace[:8]] + [np.zeros(27)])
        out["plane_in"] = steps
        rows = []
        for srow in steps:
            R, t3, ok = pr.plane_step(srow)
            rows.append((list(R) + list(t3) if ok else [0.0] * 12) + [float(ok)])
        out["plane_out"] = np.array(rows, np.float64)
    else:
        rows_in, rows_out = [], []
        for sums, n in trace[:8]:
            cs, ct = [float(v) / float(n) for v in sums[pr.SUM_S:pr.SUM_S + 3]], [float(v) / float(n) for v in sums[pr.SUM_T:pr.SUM_T + 3]]
            R, t3 = pr.rigid_step(sums[pr.SUM_H:pr.SUM_H + 9], cs, ct)
            rows_in.append(list(sums[pr.SUM_H:pr.SUM_H + 9]) + cs + ct)
            rows_out.append(list(R) + list(t3))
        out["rigid_in"], out["rigid_out"] = np.array(rows_in, np.float64), np.array(rows_out, np.float64)
    S, rows = pr.State(), []
    for sums, n in trace:
        pr.advance(S, metric, sums, n, prm["max_iter_num"], prm["transformation_epsilon"], prm["euclidean_fitness_epsilon"])
        rows.append([float(v) for v in S.row()])
    out["run_in"] = np.array([list(sums) + [float(n)] for sums, n in trace], np.float64)
    out["run_out"] = np.array(rows, np.float64)
    return out


def compute():
    cases, _ = pcl_icp_scenes.build_cases()
    out = {"names": np.array(json.dumps(list(cases)))}
    clouds = []

    def cloud_id(c):
        for k, have in enumerate(clouds):
            if have.shape == c.shape and have.tobytes() == c.tobytes():
                return k
        clouds.append(c)
        out["cloud/%d" % (len(clouds) - 1)] = c
        return len(clouds) - 1

    for name, c in cases.items():
        prm = pr.default_params(**c["prm"])
        trace = []
        res = pr.pcl_icp(c["tgt"], c["src"], c["tgt_bound"], c["src_bound"], c["guess"], prm, trace=trace)
        out[name + "/tgt_id"], out[name + "/src_id"] = np.array(cloud_id(c["tgt"])), np.array(cloud_id(c["src"]))
        out[name + "/tgt_bound"], out[name + "/src_bound"], out[name + "/guess"] = c["tgt_bound"], c["src_bound"], c["guess"]
        out[name + "/prm"] = np.array(json.dumps(c["prm"]))
        out[name + "/ints"] = np.array([res[k] for k in INT_FIELDS], np.int64)
        out[name + "/floats"] = np.array([res[k] for k in FLOAT_FIELDS], np.float64)
        out[name + "/T"] = np.asarray(res["T"], np.float64)
        if name in MATH_CASES:
            for key, v in math_records(res, trace, prm).items():
                out["math/%s/%s" % (name, key)] = v
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "pcl_icp_cases.npz")
    np.savez_compressed(path, **compute())
    print(path, os.path.getsize(path), "bytes")
