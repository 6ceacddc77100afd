"""The byte counts of include/mulls_hip.h's scratch_limit_bytes clause for mulls_coarse_reg_fpfhsac_batch, restated from that text, and where the batch
fixture lies: what tests/test_fpfh_batch.py (which holds these against mulls_amd/csrc/fpfh_batch.h) and tests/test_gpu_fpfh_batch.py (which computes
its limits from them) share.  Nothing but the standard library is imported."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_GOLDEN = os.path.join(ROOT, "tests", "golden", "fpfh_batch_cases.npz")
SCENES = ("mixed", "chunks", "shared", "default", "nan", "huber")
HEAD_BYTES = 2 << 20  # per sub-batch: the slots of a stretch
MAX_SLOTS = 1024  # MULLS_FPFH_HYP_CHUNK: slots of a stretch, problems of a sub-batch
MAX_POOL_BYTES = 256 << 20


def up256(v):
    return (v + 255) // 256 * 256


def slots(n):
    s = 1024
    while s < 2 * n:
        s *= 2
    return s


def cloud_bytes(n):
    return 4 * up256(12 * n) + 2 * up256(132 * n) + 3 * up256(4 * n) + 20 * slots(n) + 1024


def problem_bytes(n_src, n_tgt, iters):
    return cloud_bytes(n_src) + cloud_bytes(n_tgt) + 140 * iters + 1280 + 2 * up256(4 * n_src) + 4096


def counted(sizes, iters):
    """what a sub-batch of these (n_src, n_tgt) problems is counted with"""
    return HEAD_BYTES + sum(problem_bytes(s, t, iters) for s, t in sizes)


def cuts(sizes, iters, limit):
    """the header's rule: consecutive sub-batches that fit, one problem at least, MAX_SLOTS at most"""
    out, held = [0], HEAD_BYTES
    for b, (s, t) in enumerate(sizes):
        w = problem_bytes(s, t, iters)
        if b > out[-1] and (held + w > limit or b - out[-1] >= MAX_SLOTS):
            out.append(b)
            held = HEAD_BYTES
        held += w
    return out + [len(sizes)]


def pool_bytes(n_srcs, iters, counted_bytes, limit):
    one = sum(up256(4 * n) for n in n_srcs)
    left = max(limit - (counted_bytes - one), 0)
    return max(4 * max(n_srcs), min(left, MAX_POOL_BYTES, sum(4 * n * iters for n in n_srcs)))
