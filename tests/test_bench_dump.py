"""bench.py --dump-outputs DIR on a CPU box (the per-rank compute is the CPU oracle, tests/bench_cpu_shim.py): the results of the last timed step as one
float64 .npy per output, the same bits from run to run with the same arguments, the same numbers as the result table, and at most 64 MB in all."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "bench_cpu_shim.py")
NAMES = ("T", "information", "code", "iterations", "sigma", "confidence", "ncorr", "rows")


def _run(args, timeout=280):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, SHIM] + args, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load(d):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    out = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float64 for a in out.values())
    assert sum(os.path.getsize(os.path.join(d, n + ".npy")) for n in NAMES) <= 64 << 20
    return out


def test_dump_outputs_are_the_last_timed_step_and_repeat(tmp_path):
    common = ["--tiny", "--pairs", "3", "--steps", "2", "--warmup", "0", "--no-cpu-baseline", "--no-end-to-end", "--no-converging", "--sustain-s", "0"]
    d1, d2, table = tmp_path / "a", tmp_path / "b", str(tmp_path / "table.npy")
    j1 = _run(common + ["--dump-outputs", str(d1), "--dump-table", table])
    j2 = _run(common + ["--dump-outputs", str(d2)])
    assert j1["steps"] == j2["steps"] == 2 and j1["config"]["registrations_timed"] == 6 and j1["ms_per_step"] > 0
    a, b = _load(d1), _load(d2)
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
    t = np.load(table)
    assert a["T"].shape == (3, 4, 4) and a["information"].shape == (3, 6, 6) and a["ncorr"].shape == (3, 6)
    assert np.array_equal(a["rows"], np.arange(3))
    assert np.array_equal(a["T"], t[:, :16].reshape(3, 4, 4).transpose(0, 2, 1)) and np.array_equal(a["T"][:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (3, 1)))
    assert np.array_equal(a["information"], t[:, 16:52].reshape(3, 6, 6).transpose(0, 2, 1))
    assert np.array_equal(a["code"], t[:, 52]) and np.array_equal(a["iterations"], t[:, 53]) and (a["iterations"] == 3).all()
    assert np.array_equal(a["sigma"], t[:, 54]) and np.array_equal(a["confidence"], t[:, 55])
    assert (a["ncorr"].sum(axis=1) > 0).all()


def test_dump_outputs_of_the_large_configurations(tmp_path):
    j = _run(["--config", "4", "--tiny", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)])
    a = _load(tmp_path)
    n = j["config"]["pairs_per_gpu_per_step"]
    assert a["T"].shape == (n, 4, 4) and a["code"].shape == (n,) and np.array_equal(a["rows"], np.arange(n))
    assert np.array_equal(a["iterations"], np.full(n, 4.0))


def test_dump_outputs_samples_a_fixed_subset_above_the_cap(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 200_000)
    n = 5000
    table = np.random.default_rng(3).normal(size=(n, 56))
    ncorr = np.arange(n * 6, dtype=np.float64).reshape(n, 6)
    bench.dump_outputs(str(tmp_path / "a"), table, ncorr)
    bench.dump_outputs(str(tmp_path / "b"), table, ncorr)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", x + ".npy")) for x in NAMES) <= 200_000
    rows = a["rows"].astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0) and np.array_equal(a["rows"], b["rows"])
    assert np.array_equal(a["T"], table[rows, :16].reshape(-1, 4, 4).transpose(0, 2, 1)) and np.array_equal(a["ncorr"], ncorr[rows])
    assert np.array_equal(a["confidence"], table[rows, 55])
