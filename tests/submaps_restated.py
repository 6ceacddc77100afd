"""numpy restatement of the submap archive's definition (include/mulls_hip.h, "the submap archive"): the merge order, CloudUtility::get_cloud_bbx as stored
and under pose_lo, Constraint_Finder::find_overlap_registration_constraint with calculate_iou and judge_adjacent_by_id, and the pairs handed to
mulls_icp_batch.  Written from the header and upstream's sources, not from the library's code; every comparison against it is exact.

PCL and FLANN are not available where this runs: the radius search (strict d2 < r2, (d2, id) order, the first max_neighbor) is restated from memory of them
and was compared with neither."""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
MERGE_ORDER = (0, 2, 1, 3, 4, 5)  # ground, facade, pillar, beam, roof, vertex in the ABI's class numbering (utility.hpp:471-482)
OVERLAP_DEFAULTS = dict(neighbor_search_dist=50.0, min_iou_thre=0.25, adjacent_id_thre=3, search_2d=1, max_neighbor=10)  # build_pose_graph.h:43-44


def merge(clouds):
    """six clouds of raw (n, 48) records in the ABI's class order -> the submap's records in merge order"""
    return np.concatenate([np.asarray(clouds[c], np.uint8).reshape(-1, 48) for c in MERGE_ORDER], axis=0)


def xyz_of(records):
    records = np.ascontiguousarray(np.asarray(records, np.uint8).reshape(-1, 48))
    return records[:, :12].copy().view(np.float32).reshape(-1, 3)


def cloud_bbx(xyz):
    """get_cloud_bbx (utility.hpp:817-847) on float coordinates -> [min_x, min_y, min_z, max_x, max_y, max_z].  `min > v` replaces the minimum and `max < v`
    the maximum, starting from +-DBL_MAX: only values below DBL_MAX can become a minimum, only values above -DBL_MAX a maximum, a NaN neither."""
    v = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    out = [DBL_MAX] * 3 + [-DBL_MAX] * 3
    for k in range(3):
        col = v[:, k]
        lo, hi = col[col < DBL_MAX], col[col > -DBL_MAX]
        if len(lo):
            out[k] = float(lo.min())
        if len(hi):
            out[3 + k] = float(hi.max())
    return np.array(out, np.float64)


def transform_points(xyz, pose):
    """pcl::transformPointCloud with a Matrix4d: ((m00 x + m01 y) + m02 z) + m03 in double per row, stored as float"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    M = np.asarray(pose, np.float64)
    with np.errstate(all="ignore"):
        rows = [((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3] for r in range(3)]
        return np.stack(rows, axis=1).astype(np.float32)


def submap_bounds(records, pose):
    """-> (local_bound, bound) of a submap's merged records"""
    xyz = xyz_of(records)
    return cloud_bbx(xyz), cloud_bbx(transform_points(xyz, pose))


def invert4(M):
    """the library's general 4 x 4 inverse (row-pivoted LU, the definition's [LIB] line for Trans1_2), operation by operation in Python floats"""
    n = 4
    a = [float(v) for v in np.asarray(M, np.float64).T.reshape(-1)]  # column-major: a[r + 4 c]
    row_of = list(range(n))
    for col in range(n):
        p, big = col, abs(a[col + n * col])
        for r in range(col + 1, n):
            if abs(a[r + n * col]) > big:
                big, p = abs(a[r + n * col]), r
        if p != col:
            for c in range(n):
                a[col + n * c], a[p + n * c] = a[p + n * c], a[col + n * c]
            row_of[col], row_of[p] = row_of[p], row_of[col]
        piv = np.float64(a[col + n * col])
        with np.errstate(all="ignore"):
            for r in range(col + 1, n):
                a[r + n * col] = float(np.float64(a[r + n * col]) / piv)
        for c in range(col + 1, n):
            top = a[col + n * c]
            for r in range(col + 1, n):
                a[r + n * c] -= a[r + n * col] * top
    out = np.zeros((4, 4), np.float64)
    for c in range(n):
        y = [1.0 if row_of[r] == c else 0.0 for r in range(n)]
        for r in range(1, n):
            for k in range(r):
                y[r] -= a[r + n * k] * y[k]
        for r in range(n - 1, -1, -1):
            for k in range(r + 1, n):
                y[r] -= a[r + n * k] * y[k]
            with np.errstate(all="ignore"):
                y[r] = float(np.float64(y[r]) / np.float64(a[r + n * r]))
        for r in range(n):
            out[r, c] = y[r]
    return out


def mul4(A, B):
    """4 x 4 product, each entry 0.0 + four products in ascending inner index"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.zeros((4, 4), np.float64)
    for c in range(4):
        for r in range(4):
            acc = 0.0
            for k in range(4):
                acc += float(A[r, k]) * float(B[k, c])
            out[r, c] = acc
    return out


def calculate_iou(b1, b2):
    """build_pose_graph.cpp:571-590, literally, on [min_x, min_y, min_z, max_x, max_y, max_z]; max_(a, b) = a > b ? a : b, min_(a, b) = a < b ? a : b"""
    b1, b2 = [np.float64(v) for v in b1], [np.float64(v) for v in b2]

    def max_(a, b):
        return a if a > b else b

    def min_(a, b):
        return a if a < b else b

    with np.errstate(all="ignore"):
        area1 = (b1[3] - b1[0]) * (b1[4] - b1[1])
        area2 = (b2[3] - b2[0]) * (b2[4] - b2[1])
        x1, y1 = max_(b1[0], b2[0]), max_(b1[1], b2[1])
        x2, y2 = min_(b1[3], b2[3]), min_(b1[4], b2[4])
        w, h = max_(np.float64(0.0), x2 - x1), max_(np.float64(0.0), y2 - y1)
        area1i2 = w * h
        return float(area1i2 / (area1 + area2 - area1i2))


def adjacent_by_id(id_1, id_2, diff):
    """build_pose_graph.cpp:560-569"""
    return id_1 <= id_2 + diff and id_1 >= id_2 - diff


def find_overlap(poses, bounds, ids, cur, neighbor_search_dist=50.0, min_iou_thre=0.25, adjacent_id_thre=3, search_2d=1, max_neighbor=10):
    """find_overlap_registration_constraint (build_pose_graph.cpp:123-209) for blocks = submaps 0 .. cur.  poses: 4 x 4 pose_lo per submap, bounds: their
    `bound`, ids: id_in_strip.  -> a list of dicts (tgt_id, src_id, overlapping_ratio, Trans1_2) in output order."""
    if cur + 1 < adjacent_id_thre + 2:
        return []
    dims = 2 if search_2d else 3
    r = np.float32(neighbor_search_dist)
    r2 = np.float32(np.float64(r) * np.float64(r))
    q = [np.float32(np.asarray(poses[cur], np.float64)[k, 3]) for k in range(dims)]
    nb = []
    with np.errstate(all="ignore"):
        for i in range(cur):
            d2 = np.float32(0.0)
            for k in range(dims):
                d = np.float32(q[k] - np.float32(np.asarray(poses[i], np.float64)[k, 3]))
                d2 = np.float32(d2 + np.float32(d * d))
            if d2 < r2:
                nb.append((float(d2), i))
    nb.sort()  # (d2, id) ascending
    if max_neighbor > 0:
        nb = nb[:max_neighbor]
    edges = []
    thr = float(np.float32(min_iou_thre))
    for _, i in nb:
        iou = calculate_iou(bounds[cur], bounds[i])
        if adjacent_by_id(int(ids[cur]), int(ids[i]), adjacent_id_thre) or not iou > thr:
            continue
        edges.append(dict(tgt_id=i, src_id=cur, overlapping_ratio=iou, Trans1_2=mul4(invert4(poses[i]), poses[cur])))
    edges.sort(key=lambda e: -e["overlapping_ratio"])  # stable: ties keep the neighbour order
    return edges


def pairs(edges, submap_clouds, local_bounds):
    """what mulls_submaps_pairs hands to mulls_icp_batch, from host data: per edge (tgt clouds, src clouds, tgt_bound, init_guess); submap_clouds[id]: the six
    class clouds as stored, local_bounds[id]: the submap's local_bound"""
    return [dict(tgt=submap_clouds[e["tgt_id"]], src=submap_clouds[e["src_id"]], tgt_bound=np.asarray(local_bounds[e["tgt_id"]], np.float64),
                 init_guess=np.asarray(e["Trans1_2"], np.float64)) for e in edges]
