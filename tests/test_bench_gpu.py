"""GPU box: bench.py itself, end to end on a small grid -- the JSON line the driver parses must carry every field of the
contract; with --full also live PMC traffic (rocprofv3 child processes), clocks and the CPU baseline; a plain run measures
only the headline, and --dump-outputs writes what its timed steps computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f"bench.py must print ONE line, got {len(lines)}"
    return json.loads(lines[0])


def test_bench_line_carries_the_contract_fields(tmp_path):
    d = _run("--grid", "4096", "--steps", "20", "--warmup", "5", "--repeats", "5", "--no-secondary", "--full",
             "--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "gpu_state"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"] and d["repeats"] == 5
    assert d["value"] > 1e5 and abs(d["ms_per_step"] * d["value"] * 1e6 / 1e3 - 4096 * 4096) / (4096 * 4096) < 0.02
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "steady_state", "overfetch", "kernel"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s"
    if r["traffic"] is not None:          # live PMC worked: the fraction is the per-launch bytes over the launch time
        assert abs(r["traffic"] / (r["avg_launch_ms"] * 1e-3) / 1e9 / 8000.0 - r["frac"]) < 0.01
        assert 0.9 < r["overfetch"] < 3 and 0.05 < r["frac"] < 1.0
    else:
        assert "traffic_note" in r
    assert r["steady_state"]["steps_per_launch"] == 16 and r["steady_state"]["avg_launch_ms"] > 0
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 1
    # three 64 MB fields: a window around the source and a seeded sample of each, within the 64 MB budget
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(f"{n}_{k}.npy" for n in ("Ez", "Hx", "Hy") for k in ("centre", "sample"))
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    ez = np.load(tmp_path / "Ez_centre.npy")
    assert ez.dtype == np.float32 and ez.shape == (1024, 1024) and np.isfinite(ez).all() and np.abs(ez).max() > 0


def test_bench_other_dtype_boundary_and_no_pmc():
    d = _run("--grid", "2048", "--cols", "4096", "--steps", "16", "--warmup", "0", "--repeats", "3", "--dtype", "f64", "--pmc", "off",
             "--no-secondary", "--no-cpu-baseline")
    assert d["dtype"] == "f64" and d["roofline"]["traffic"] is None and d["value"] > 1e4
    d = _run("--grid", "2048", "--cols", "4096", "--steps", "32", "--warmup", "16", "--repeats", "3", "--boundary", "pml", "--pmc", "off",
             "--no-secondary", "--no-cpu-baseline")
    assert d["config"]["boundary"] == "pml" and d["value"] > 1e4


def test_plain_run_is_lean_and_dumps_what_its_timed_steps_computed(tmp_path):
    """Without --full the line holds the headline alone (one timed run of exactly K steps), and --dump-outputs writes
    the fields the timed steps left: those of the untimed K-step runs from zero fields (400 steps in all here) and the K
    timed steps after them, value-identical to the NumPy oracle's."""
    sys.path.insert(0, ROOT)
    import bench
    import fdtd2d_amd as fd
    from oracle import fdtd_numpy as onp
    rows, cols, steps = 320, 400, 40
    d = _run("--grid", str(rows), "--cols", str(cols), "--steps", str(steps), "--warmup", "8", "--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    for k in ("cpu_baseline", "gpu_state", "secondary"):
        assert k not in d, k
    assert d["steps"] == steps and d["repeats"] == 1 and len(d["wall_ms_all"]) == 1 and d["roofline"]["traffic"] is None
    assert abs(d["ms_per_step"] * steps - d["wall_ms_all"][0]) < 1e-3 * d["wall_ms_all"][0] + 1e-4
    ref = onp.grid_zeros(rows, cols, np.float32)
    eps, mu = onp.vacuum_materials(rows, cols, np.float32)
    total = -(-bench.REHEARSAL_STEPS // steps) * steps + steps
    onp.leapfrog(*ref, eps, mu, bench.DT, bench.DX, total, rows // 2, cols // 2, amps=bench.amplitudes(fd, 0, total))
    for name, want in zip(("Ez", "Hx", "Hy"), ref):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, want), name
