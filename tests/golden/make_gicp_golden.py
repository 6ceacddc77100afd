"""Writes tests/golden/gicp_cases.npz: the scenes of tests/gicp_scenes.py with the results of the numpy restatement (tests/gicp_restated.py), and
recorded inputs and outputs of its pieces (math/...: point covariances, exp / log, one point's 28 sums, the Cholesky step, the loop's state) for the host harness.
tests/test_gicp.py keeps the file equal to the restatement; tests/test_gpu_gicp.py compares the device with it.

    python tests/golden/make_gicp_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import gicp_restated as gr  # noqa: E402
import gicp_scenes  # noqa: E402

INT_FIELDS = ("code", "iterations", "converged", "stop", "n_src", "n_tgt", "n_voxels", "n_corr")
FLOAT_FIELDS = ("fitness", "loss")


def math_records(res, trace, prm):
    """the pieces on the inputs the street and crafted cases produce"""
    out = {}
    k = prm["k_correspondences"]
    src = res["src_c"]
    nb = gr.neighbours(src, k)[:40]
    out["cov_in"] = src[nb].astype(np.float64)
    out["cov_out"] = np.array([gr.point_covariance(q) for q in out["cov_in"]])
    vecs = [t[0] for t in trace] + [[0.0, 0.0, 0.0], [1e-9, -2e-9, 3e-9], [0.3, -0.2, 0.1], [1.0, 0.5, -0.7]]
    out["exp_in"] = np.array(vecs, np.float64)
    out["exp_out"] = np.array([gr.so3_exp(v) for v in vecs])
    out["log_out"] = np.array([gr.so3_log(gr.so3_exp(v)) for v in vecs])
    return out


def compute():
    cases, _ = gicp_scenes.build_cases()
    out = {"names": np.array(json.dumps(list(cases)))}
    for name, c in cases.items():
        prm = gr.default_params(**c["prm"])
        trace = []
        res = gr.gicp(c["tgt"], c["src"], c["tgt_bound"], c["src_bound"], c["guess"], prm, trace=trace)
        out[name + "/tgt"], out[name + "/src"] = c["tgt"], c["src"]
        out[name + "/tgt_bound"], out[name + "/src_bound"], out[name + "/guess"] = c["tgt_bound"], c["src_bound"], c["guess"]
        out[name + "/prm"] = np.array(json.dumps(c["prm"]))
        out[name + "/ints"] = np.array([res[k] for k in INT_FIELDS], np.int64)
        out[name + "/floats"] = np.array([res[k] for k in FLOAT_FIELDS], np.float64)
        out[name + "/T"] = np.asarray(res["T"], np.float64)
        if name in ("street", "crafted"):
            for key, v in math_records(res, trace, prm).items():
                out["math/%s/%s" % (name, key)] = v
            # one point's 28 sums and the step, on the first evaluation's inputs
            r, t, R, sums, n_corr = trace[0]
            vm = gr.build_voxels(res["tgt_c"], res["C_tgt"], prm["voxel_resolution"])
            ap = gr.move(R, t, res["src_c"])
            coords, ok = gr.voxel_coords(ap.astype(np.float32), vm.resolution)
            vox = np.array([vm.index.get(gr.pack(cc), -1) if o else -1 for cc, o in zip(coords, ok)])
            sel = np.flatnonzero(vox >= 0)[:30]
            out["math/%s/term_in" % name] = np.concatenate([ap[sel], res["C_src"][sel], vm.mean[vox[sel]], vm.cov[vox[sel]], np.tile(R, (len(sel), 1))], axis=1)
            out["math/%s/term_out" % name] = gr.point_terms(ap[sel], res["C_src"][sel], vm.mean[vox[sel]], vm.cov[vox[sel]], R)
            steps = np.array([tr[3][:27] for tr in trace[:8]] + [np.zeros(27)])
            out["math/%s/step_in" % name] = steps
            S, rows = gr.State(prm["start_rotvec"]), []
            for tr in trace:
                gr.advance(S, tr[3], tr[4], prm["max_iterations"], prm["rotation_epsilon"], prm["transformation_epsilon"])
                rows.append(list(S.r) + list(S.t) + list(S.R) + [S.loss, S.n_corr, S.iterations, S.converged, S.stop, S.running])
            out["math/%s/run_in" % name] = np.array([list(tr[3]) + [float(tr[4])] for tr in trace])
            out["math/%s/run_out" % name] = np.array(rows, np.float64)
            out["math/%s/step_out" % name] = np.array([list(d) + [float(ok)] for d, ok in (gr.solve_step(s[:21], s[21:27]) for s in steps)])
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "gicp_cases.npz")
    np.savez_compressed(path, **compute())
    print(path, os.path.getsize(path), "bytes")
