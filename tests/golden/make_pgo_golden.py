"""Writes tests/golden/pgo_cases.npz: the inputs of the pose graph optimisation cases that tests/test_pgo.py and tests/test_gpu_pgo.py use, and what
tests/pgo_restated.py returns for them.  Seeds are fixed.  Every case must keep its accept / reject ratios further than 1e-6 from 1e-3, so that no case
sits on a decision edge; the generator refuses to write otherwise.

    python tests/golden/make_pgo_golden.py

Also stored: the defaults of upstream's pgo_param_t and of the flags mulls_slam passes on (read off include/common/utility.hpp:743-791 and
test/mulls_slam.cpp:170-191 of the reference), as a list of names and values.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pgo_restated as R  # noqa: E402

KEYS = list(R.DEFAULTS)
INTS = ["status", "termination", "iterations", "successful_steps", "n_free", "n_boxed", "n_fixed", "n_edges_used", "wrong_edges", "correct_reg_edges", "edges_ok"]

# name, value, where: what the reference says, and what the library's default follows (the flag where mulls_slam overwrites the struct)
UPSTREAM_DEFAULTS = [
    ("num_iterations", 100, "mulls_slam.cpp:181 max_iter_inter_submap (utility.hpp:771 has 50)"),
    ("robustify", 0, "mulls_slam.cpp:190 robust_kernel_on (utility.hpp:760 has true)"),
    ("use_equal_weight", 0, "utility.hpp:761, mulls_slam.cpp:170"),
    ("use_diagonal_information_matrix", 0, "utility.hpp:763, mulls_slam.cpp:185"),
    ("free_all_nodes", 0, "utility.hpp:764, mulls_slam.cpp:191"),
    ("only_limit_translation", 0, "utility.hpp:762"),
    ("robust_delta", 1.0, "utility.hpp:766"),
    ("quat_tran_ratio", 1000.0, "utility.hpp:773"),
    ("t_limit", 2.0, "mulls_slam.cpp:177 inter_submap_t_limit"),
    ("r_limit", 0.05, "mulls_slam.cpp:178 inter_submap_r_limit"),
    ("function_tolerance", 1e-16, "graph_optimizer.cpp:445"),
    ("wrong_edge_translation_thre", 5.0, "utility.hpp:776, mulls_slam.cpp:186"),
    ("wrong_edge_rotation_thre", 25.0, "mulls_slam.cpp:187 (utility.hpp:777 has 20)"),
    ("wrong_edge_ratio_thre", 0.1, "utility.hpp:778"),
]


def rot(rng, deg):
    """a rotation by a random axis and an angle of at most deg degrees"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg) * rng.uniform(-1, 1)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def pose(Rm, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    return T


def inv(T):
    return pose(T[:3, :3].T, -T[:3, :3].T @ T[:3, 3])


def info(rng):
    B = np.diag([10.0, 10.0, 10.0, 100.0, 100.0, 100.0]) @ (np.eye(6) + 0.1 * rng.normal(size=(6, 6)))
    return B @ B.T


def walk(rng, n, step=1.0, turn=5.0):
    gt = [pose(rot(rng, 20.0), rng.normal(size=3))]
    for _ in range(n - 1):
        gt.append(gt[-1] @ pose(rot(rng, turn), np.array([step, 0.0, 0.0]) + 0.05 * rng.normal(size=3)))
    return gt


def noisy(rng, T, t_sigma, deg):
    return T @ pose(rot(rng, deg), t_sigma * rng.normal(size=3))


def chain(seed, n, t_sigma=0.02, deg=0.3, zero_info_at=None, both_ends=True):
    """odometry chain: the initial poses compose noisy odometry, the ends are pinned to the ground truth"""
    rng = np.random.default_rng(seed)
    gt = walk(rng, n)
    edges, init = [], [gt[0]]
    for i in range(n - 1):
        T = noisy(rng, inv(gt[i]) @ gt[i + 1], t_sigma, deg)
        edges.append((i, i + 1, R.ADJACENT, T, info(rng) if i != zero_info_at else np.zeros((6, 6))))
        init.append(init[-1] @ T)
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    if both_ends and n > 1:
        fixed[-1] = 1
        init[-1] = gt[-1]
    return np.array(init), fixed, np.zeros(n, np.uint8), edges, np.array(gt)


def loops14(seed):
    poses, fixed, stable, edges, gt = chain(seed, 14, both_ends=False)
    rng = np.random.default_rng(seed + 1000)
    for a, b in ((2, 9), (4, 7), (3, 12)):
        edges.append((a, b, R.SMOOTH, noisy(rng, inv(gt[a]) @ gt[b], 0.02, 0.3), info(rng)))
    edges.append((4, 7, R.SMOOTH, noisy(rng, inv(gt[4]) @ gt[7], 0.02, 0.3), info(rng)))  # a second edge between one pair
    edges.append((11, 5, R.SMOOTH, noisy(rng, inv(gt[11]) @ gt[5], 0.02, 0.3), info(rng)))  # a > b
    stable[6] = 1
    return poses, fixed, stable, edges, gt


def square40(seed):
    """40 submaps round a 100 m square, odometry with drift, one closing registration edge 39 -> 0 ... stated as (0, 39) so that only node 0 is fixed"""
    rng = np.random.default_rng(seed)
    gt = []
    for k in range(40):
        side, s = divmod(k, 10)
        c = [(10.0 * s, 0.0), (100.0, 10.0 * s), (100.0 - 10.0 * s, 100.0), (0.0, 100.0 - 10.0 * s)][side]
        yaw = np.pi / 2 * side
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])
        gt.append(pose(Rz, np.array([c[0], c[1], 0.0])))
    edges, init = [], [gt[0]]
    for i in range(39):
        T = noisy(rng, inv(gt[i]) @ gt[i + 1], 0.15, 0.4)
        edges.append((i, i + 1, R.ADJACENT, T, info(rng)))
        init.append(init[-1] @ T)
    edges.append((0, 39, R.REGISTRATION, noisy(rng, inv(gt[0]) @ gt[39], 0.02, 0.05), 4.0 * info(rng)))
    fixed = np.zeros(40, np.uint8)
    fixed[0] = 1
    return np.array(init), fixed, np.zeros(40, np.uint8), edges, np.array(gt)


def consistent(seed, n=12):
    """edges from the ground truth, the initial poses perturbed by 0.5 m / 3 degrees: the optimum is the ground truth, cost 0"""
    rng = np.random.default_rng(seed)
    gt = walk(rng, n)
    edges = [(i, i + 1, R.ADJACENT, inv(gt[i]) @ gt[i + 1], info(rng)) for i in range(n - 1)]
    for a, b in ((1, 8), (3, 10)):
        edges.append((a, b, R.SMOOTH, inv(gt[a]) @ gt[b], info(rng)))
    init = [gt[0]] + [pose(T[:3, :3] @ rot(rng, 3.0), T[:3, 3] + 0.5 * rng.uniform(-1, 1, 3) / np.sqrt(3)) for T in gt[1:]]
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return np.array(init), fixed, np.zeros(n, np.uint8), edges, np.array(gt)


def cases():
    out = {}

    def add(name, c, **kw):
        out[name] = (c[0], c[1], c[2], c[3], R.params(**kw), c[4])

    # smallest graphs
    c = chain(1, 2, both_ends=False)
    c[0][1] = noisy(np.random.default_rng(100), c[0][1], 0.3, 2.0)  # the free node starts off its answer T_0 T
    add("two_nodes", c)
    add("chain3", chain(2, 3))
    c = chain(3, 4)
    c[1][:] = 1
    add("all_fixed", c)
    add("one_node", chain(4, 1))
    # chains at the lane edges, one edge with zero information
    for n in (63, 64, 65, 257):
        add("chain%d" % n, chain(10 + n, n, zero_info_at=n // 3))
    add("chain151", chain(151, 151), t_limit=0.1, r_limit=0.01)
    # skyline fill
    add("loops14", loops14(20))
    add("square40", square40(21))
    # options
    add("w_equal", loops14(22), use_equal_weight=1)
    add("w_diag", loops14(23), use_diagonal_information_matrix=1)
    c = loops14(24)
    a, b, typ, T, I = c[3][14]
    c[3][14] = (a, b, typ, T @ pose(np.eye(3), np.array([10.0, 0.0, 0.0])), I)
    add("huber", c, robustify=1)
    add("only_translation", loops14(25), only_limit_translation=1, t_limit=0.05, r_limit=0.001)
    add("free_all", loops14(26), free_all_nodes=1)
    # active box: the closing edge is 10 m off, the boxes are tight
    c = square40(27)
    a, b, typ, T, I = c[3][-1]
    c[3][-1] = (a, b, typ, T @ pose(np.eye(3), np.array([10.0, 0.0, 0.0])), I)
    add("active_box", c, t_limit=0.1, r_limit=0.002)
    # stops
    add("iter0", loops14(28), num_iterations=0)
    add("iter1", loops14(28), num_iterations=1)
    # the early return: three nodes, one of them fixed, one edge
    c = chain(29, 3, both_ends=False)
    add("early_return", (c[0], c[1], c[2], c[3][:1], c[4]))
    # HISTORY and NONE edges are skipped
    c = loops14(30)
    c[3].append((1, 12, R.HISTORY, np.eye(4), info(np.random.default_rng(1))))
    c[3].append((0, 13, R.NONE, np.eye(4), info(np.random.default_rng(2))))
    add("skipped_edges", c)
    add("consistent", consistent(31))
    return out


def main():
    data = {"upstream_default_names": np.array([d[0] for d in UPSTREAM_DEFAULTS]), "upstream_default_values": np.array([float(d[1]) for d in UPSTREAM_DEFAULTS]),
            "upstream_default_where": np.array([d[2] for d in UPSTREAM_DEFAULTS]), "param_keys": np.array(KEYS), "int_keys": np.array(INTS)}
    names = []
    for name, (poses, fixed, stable, edges, p, gt) in cases().items():
        r = R.solve(poses, fixed, stable, edges, p)
        err0 = float(np.mean(np.linalg.norm(poses[:, :3, 3] - gt[:, :3, 3], axis=1)))
        err1 = float(np.mean(np.linalg.norm(r["poses"][:, :3, 3] - gt[:, :3, 3], axis=1)))
        rot_err = float(max(np.abs(r["poses"][:, :3, :3] - gt[:, :3, :3]).max(), 0.0)) if len(gt) else 0.0
        print("%-18s n %3d status %2d term %d it %3d ok %3d cost %.6e -> %.6e ratio-dist %.3e box %.3e terr %.3e -> %.3e rerr %.3e wrong %d" % (
            name, len(poses), r["status"], r["termination"], r["iterations"], r["successful_steps"], r["initial_cost"], r["final_cost"],
            r["min_ratio_distance"], r["max_box_excess"], err0, err1, rot_err, r["wrong_edges"]))
        assert r["min_ratio_distance"] > 1e-6, name
        names.append(name)
        m = len(edges)
        data[name + ".poses"], data[name + ".fixed"], data[name + ".stable"], data[name + ".gt"] = poses, fixed, stable, gt
        data[name + ".ab"] = np.array([[e[0], e[1], e[2]] for e in edges], np.int32).reshape(m, 3)
        data[name + ".T"] = np.array([e[3] for e in edges]).reshape(m, 4, 4)
        data[name + ".info"] = np.array([e[4] for e in edges]).reshape(m, 6, 6)
        data[name + ".params"] = np.array([float(p[k]) for k in KEYS])
        data[name + ".out_poses"] = r["poses"]
        data[name + ".out_ints"] = np.array([r[k] for k in INTS], np.int64)
        data[name + ".out_costs"] = np.array([r["initial_cost"], r["final_cost"]])
        data[name + ".out_wrong"] = r["edge_wrong"]
        data[name + ".out_extra"] = np.array([r["min_ratio_distance"], r["max_box_excess"], err0, err1, rot_err])
    data["names"] = np.array(names)
    path = os.path.join(HERE, "pgo_cases.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
