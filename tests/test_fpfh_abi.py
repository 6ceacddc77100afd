"""The ctypes mirror, the defaults and the exports of mulls_fpfh and mulls_coarse_reg_fpfhsac against include/mulls_hip.h, which must still compile as
plain C.  These tests need neither a device nor mpmath; they fail on a tree without the two entry points."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

from mulls_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_layout_matches_header():
    fields = {"mulls_fpfh_params": abi.FpfhParams, "mulls_fpfhsac_params": abi.FpfhSacParams, "mulls_fpfhsac_result": abi.FpfhSacResult}
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "mulls_hip.h"', "int main(void){"]
    for cname, ct in fields.items():
        prog.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            prog.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog.append('printf("error %d %d\\n", MULLS_SACIA_TRUNCATED, MULLS_SACIA_HUBER);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])  # (the header is still plain C)
        out = subprocess.check_output([exe]).decode().split("\n")
    got = {line.split()[0]: line.split()[1:] for line in out if line}
    for cname, ct in fields.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got["%s.%s" % (cname, f)][0]) == getattr(ct, f).offset, (cname, f)
    assert [int(v) for v in got["error"]] == [abi.SACIA_TRUNCATED, abi.SACIA_HUBER] == [0, 1]
    chunk = re.search(r"#define MULLS_FPFH_HYP_CHUNK (\d+)u", open(os.path.join(ROOT, "mulls_amd", "csrc", "fpfh_launch.h")).read())
    assert int(chunk.group(1)) == abi.FPFH_HYP_CHUNK
    cell = re.search(r"#define MULLS_FPFH_MAX_CELL_POINTS (\d+)u", open(os.path.join(ROOT, "include", "mulls_hip.h")).read())
    assert int(cell.group(1)) == abi.FPFH_MAX_CELL_POINTS
    assert C.sizeof(abi.FpfhParams) == 8 and C.sizeof(abi.FpfhSacParams) == 32 and C.sizeof(abi.FpfhSacResult) == 160 and abi.FPFH_DIMS == 33


def test_exports_and_defaults():
    header = open(os.path.join(ROOT, "include", "mulls_hip.h")).read()
    declared = set(re.findall(r"\b(mulls_fpfh\w*|mulls_coarse_reg_fpfhsac)\s*\(", header))
    assert declared == {"mulls_fpfh_default_params", "mulls_fpfh", "mulls_fpfhsac_default_params", "mulls_coarse_reg_fpfhsac"} and declared <= set(lib.EXPORTS)
    L = lib.load()
    for name in declared:
        assert hasattr(L, name), name
    p, q = abi.FpfhSacParams(), abi.fpfhsac_params()
    L.mulls_fpfhsac_default_params(C.byref(p))
    r = dict(search_radius=1.0, nr_samples=3, k_correspondences=15, max_iterations=10, min_sample_distance=0.0, max_correspondence_distance=float("inf"),
             error_function=0, seed=0)  # (tests/test_fpfh.py holds the restatement's defaults to the same values)
    for name, _ in abi.FpfhSacParams._fields_:
        assert getattr(p, name) == getattr(q, name) == r[name], name
    assert (p.nr_samples, p.k_correspondences, p.max_iterations, p.min_sample_distance, p.error_function) == (3, 15, 10, 0.0, 0) and np.isinf(p.max_correspondence_distance)
    f = abi.FpfhParams(7.0, 7)
    L.mulls_fpfh_default_params(C.byref(f))
    assert (f.search_radius, f.reserved) == (abi.fpfh_params().search_radius, 0) == (1.0, 0)
    # argument checks that need no device
    assert L.mulls_fpfh(None, None, None, None, None) == abi.MULLS_E_INVALID
    assert L.mulls_coarse_reg_fpfhsac(None, None, None, None, None) == abi.MULLS_E_INVALID
