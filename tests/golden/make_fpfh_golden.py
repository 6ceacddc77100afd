"""Writes tests/golden/fpfh_cases.npz: the scenes of tests/fpfh_scenes.py with the results of the numpy restatement (tests/fpfh_restated.py), and
recorded inputs and outputs of its pieces (math/...: pair features and bins, SPFH values, normalisations, error terms, descriptor distances, draw
sequences) for the host harness.  tests/test_fpfh.py keeps the file equal to the restatement; tests/test_gpu_fpfh.py compares the device with it.

    python tests/golden/make_fpfh_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import fpfh_restated as fr  # noqa: E402
import fpfh_scenes  # noqa: E402
from fpfh_names import FLOAT_FIELDS, INT_FIELDS  # noqa: E402

PAIR_CASES = ("duplicates", "normals", "bin_edges", "radius_edge")
DRAWS = (("sac_it65", 65), ("sac_halving", 3), ("sac_three", 4))


def inner_edges():
    """features exactly on inner bin edges: the doubles next to 2 k / 11 - 1 with 11 ((f + 1) 0.5) == k exactly as f2 and f3, those next to
    2 pi k / 11 - pi with 11 ((f1 + pi) (1 / (2 pi))) == k exactly as f1; the outer edges +-1 and +-pi; NaNs"""
    rows = []

    def near(centre, lands):
        for step in range(0, 17):
            for sign in (1, -1):
                c = centre
                for _ in range(step):
                    c = float(np.nextafter(c, np.inf * sign))
                if lands(c):
                    return c
        return None

    for k in range(1, 11):
        f = near(2.0 * k / 11.0 - 1.0, lambda c: 11.0 * ((c + 1.0) * 0.5) == float(k))
        if f is not None:
            rows.append([0.0, f, f])
        f1 = near(2.0 * fr.PI * k / 11.0 - fr.PI, lambda c: 11.0 * ((c + fr.PI) * fr.INV_2PI) == float(k))
        if f1 is not None:
            rows.append([f1, 0.0, 0.0])
    assert len(rows) >= 10
    rows += [[fr.PI, 1.0, 1.0], [-fr.PI, -1.0, -1.0], [float("nan"), 0.0, 0.0], [0.0, 0.0, float("nan")]]
    return np.array(rows, np.float64)


def math_records(fcases, fdetail, scases, sdetail):
    out = {}
    rows, want = [], []
    for name in PAIR_CASES:
        c = fcases[name]
        P, N = c["pts"], c["nrm"]
        for i in range(len(P)):
            others = [j for j in range(len(P)) if j != i][:24]
            f, ok = fr.pair_features(P[i], N[i], P[others], N[others])
            b, good = fr.bins_of(f)
            for j, fj, okj, bj, gj in zip(others, f, ok, b, good):
                adds = bool(okj and gj)
                rows.append(np.concatenate([P[i], N[i], P[j], N[j]]).astype(np.float64))
                want.append([1.0] + list(fj) + [float(v) for v in bj] if adds else [0.0] * 7)
    out["pair_in"], out["pair_out"] = np.array(rows), np.array(want, np.float64)
    edges = inner_edges()
    b, good = fr.bins_of(edges)
    out["bins_in"], out["bins_out"] = edges, np.concatenate([good[:, None].astype(np.float64), np.where(good[:, None], b, 0).astype(np.float64)], axis=1)
    d = fdetail["sizes"]
    sel = np.arange(0, len(d["counts"]), 7)
    out["spfh_in"] = np.stack([d["counts"][sel].astype(np.float64), np.broadcast_to(d["k"][sel, None].astype(np.float64), (len(sel), fr.DIMS))], axis=2).reshape(-1, 2)
    out["spfh_in"] = np.concatenate([out["spfh_in"], [[0.0, 1.0], [0.0, 0.0], [3.0, 2.0]]])
    out["spfh_out"] = fr.spfh_of_counts(out["spfh_in"][:, :1].astype(np.int64), out["spfh_in"][:, 1].astype(np.int64)).astype(np.float64)
    acc = np.concatenate([fdetail["sizes"]["acc"][::9], fdetail["three"]["acc"], fdetail["duplicates"]["acc"]])
    out["norm_in"], out["norm_out"] = acc, fr.normalise(acc).astype(np.float64)
    rows = []
    for name in ("sac_threshold_truncated", "sac_threshold_huber", "sac_default"):
        prm = fr.fpfhsac_default_params(**scases[name]["prm"])
        e = sdetail[name]["e"][2]
        for h in (0, 1):
            rows += [[float(v), float(np.float32(prm["max_correspondence_distance"])), float(h)] for v in e]
    E = np.array(rows, np.float64)
    out["error_in"] = E
    out["error_out"] = np.array([fr.error_terms(np.float32([e]), t, int(h))[0] for e, t, h in E], np.float64).reshape(-1, 1)
    hs, ht = sdetail["sac_it65"]["src_hist"], sdetail["sac_it65"]["tgt_hist"]
    out["dist_in"] = np.concatenate([np.repeat(hs[:6], 8, axis=0), np.tile(ht[:8], (6, 1))], axis=1).astype(np.float64)
    out["dist_out"] = np.concatenate([fr.desc_dist2(hs[i], ht[:8]) for i in range(6)]).astype(np.float64).reshape(-1, 1)
    vals = [0.0, 1.5, float("inf"), float("nan"), -0.0, 2.0]
    rows = [[a, i, b, j] for a in vals for b in vals for i, j in ((0, 1), (1, 0))]
    out["order_in"] = np.array(rows, np.float64)
    out["order_out"] = np.array([[1.0 if fr.first_hypothesis([b, a] if i else [a, b]) == i else 0.0] for a, i, b, j in rows], np.float64)
    for name, iters in DRAWS:
        c, prm = scases[name], fr.fpfhsac_default_params(**scases[name]["prm"])
        k_eff = min(prm["k_correspondences"], len(c["tgt"]))
        s, r, end = fr.draw_all(c["src"], k_eff, iters, prm["min_sample_distance"], prm["seed"])
        out["draw/%s/args" % name] = np.array([len(c["src"]), k_eff, iters, prm["min_sample_distance"], prm["seed"]], np.float64)
        out["draw/%s/out" % name] = np.concatenate([np.concatenate([s, r], axis=1).astype(np.float64), [[end, 0, 0, 0, 0, 0]]])
    return out


def compute():
    fcases, scases = fpfh_scenes.fpfh_cases(), fpfh_scenes.sac_cases()
    out = {"fpfh_names": np.array(json.dumps(list(fcases))), "sac_names": np.array(json.dumps(list(scases)))}
    fdetail, sdetail = {}, {}
    for name, c in fcases.items():
        d = {}
        hist, k = fr.fpfh(c["pts"], c["nrm"], c["search_radius"], d)
        d["k"] = k
        fdetail[name] = d
        out[name + "/pts"], out[name + "/nrm"], out[name + "/search_radius"] = c["pts"], c["nrm"], np.array(c["search_radius"])
        out[name + "/hist"], out[name + "/k"] = hist, k
        out[name + "/pairs_used"] = d["used"]
    for name, c in scases.items():
        d = {}
        res = fr.fpfhsac(c["tgt"], c["tgt_nrm"], c["src"], c["src_nrm"], fr.fpfhsac_default_params(**c["prm"]), d)
        sdetail[name] = d
        for key in ("tgt", "tgt_nrm", "src", "src_nrm"):
            out["%s/%s" % (name, key)] = c[key]
        out[name + "/prm"] = np.array(json.dumps(c["prm"]))
        out[name + "/ints"] = np.array([res[k] for k in INT_FIELDS], np.int64)
        out[name + "/floats"] = np.array([res[k] for k in FLOAT_FIELDS], np.float64)
        out[name + "/T"] = np.asarray(res["T"], np.float64)
        out[name + "/errors"] = d["errors"]
        out[name + "/samples"], out[name + "/corr"] = d["samples"].astype(np.int32), d["corr"].astype(np.int32)
        out[name + "/min_d"] = np.array(d["min_d"])
        if name == "sac_threshold_truncated":
            out[name + "/e2"] = d["e"][2]
    for key, v in math_records(fcases, fdetail, scases, sdetail).items():
        out["math/" + key] = v
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "fpfh_cases.npz")
    np.savez_compressed(path, **compute())
    print(path, os.path.getsize(path), "bytes")
