"""CPU test of the one place that lays a registration cell table out (mulls_amd/csrc/reg_table.h, shared by mulls_gicp and mulls_pcl_icp): the program
tests/reg_table_harness.cpp, built with the address and undefined-behaviour sanitizers and run on its own, checks the slot rule, the shift, the arrays'
alignment, order and separation, the cleared arrays' extents and the dry layout against the real one; here its byte counts are also held against the rule
written out again, since a problem's bytes decide where a batch is cut into sub-batches."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = sorted({0, 1, 511, 512, 513} | {v for k in range(0, 21) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)})


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reg_table") / "reg_table_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "reg_table_harness.cpp"), "-o", exe])
    return exe


def up256(v):
    return (v + 255) & ~255


def test_layout_of_every_size(harness):
    assert {0, 1, 511, 512, 513, (1 << 20) - 1, 1 << 20, (1 << 20) + 1} <= set(SIZES)
    p = subprocess.run([harness] + [str(n) for n in SIZES], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    lines = p.stdout.split("\n")
    assert lines[-2] == "ok %d" % (2 * len(SIZES))
    got = {(int(a), int(b)): int(c) for a, b, c in (line.split() for line in lines[:-2])}
    for n in SIZES:
        slots = 1024
        while slots < 2 * n:
            slots *= 2
        table = up256(8 * slots) + 3 * up256(4 * slots)
        assert got[(n, 0)] == 2 * up256(4 * n) + table, n
        assert got[(n, 1)] == 2 * up256(4 * n) + up256(12 * n) + table, n
