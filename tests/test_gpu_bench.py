"""bench.py's plain run: the headline line only, --steps timed steps, and --dump-outputs writing
what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_plain_line_and_dump_outputs(tmp_path):
    rows, steps = 50000, 3
    out_dir, npz = tmp_path / "outputs", tmp_path / "dump.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", str(rows),
                        "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir), "--dump", str(npz)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "fit+predict points/sec, d=20 n=50000 p=4096"
    assert line["unit"] == "points/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == steps and len(line["step_ms"]) == steps
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - rows / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    # a plain run measures the headline and nothing else
    for key in ("kernels_ms", "parity_check", "alt_backend", "configs", "obfit_eval", "cpu_baseline", "roofline"):
        assert key not in line, key
    got = {f[:-4]: np.load(str(out_dir / f)) for f in os.listdir(str(out_dir))}
    assert set(got) == {"theta", "mean", "meansd"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["theta"].shape == (4096,) and got["mean"].shape == (rows,) and got["meansd"].shape == (3,)
    assert np.all(np.isfinite(got["mean"])) and np.any(got["theta"] != 0) and got["meansd"][2] == rows
    ref = np.load(str(npz))
    assert np.array_equal(ref["theta"], got["theta"]) and np.array_equal(ref["mean"], got["mean"][:1000])
    assert np.array_equal(ref["meansd"], got["meansd"])
