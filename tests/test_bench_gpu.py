"""bench.py's output contract on the GPU (one short --full run per storage family): one JSON line with the driver's keys,
the roofline object measured live, no CPU baseline when asked not to; a plain run: the same line with the extra
measurements left null."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cfg,dtype,bound", [("c2", "f32", "mfma"), ("c5", "bf16", "hbm")])
def test_bench_line(cfg, dtype, bound, tmp_path):
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--config", cfg, "--steps", "4", "--warmup", "2",
                          "--full", "--no-cpu-baseline", "--dump-outputs", str(dump)], capture_output=True, text=True,
                         timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["metric"] == "samples/sec" and line["n_gpus"] == 1 and line["steps"] == 4 and line["dtype"] == dtype
    assert line["value"] > 0 and line["vs_baseline"] is None and line["cpu_baseline"] is None and line["scaling"] == "weak"
    assert "workload" in line["config"] and line["config"]["hip_graph"] is True
    r = line["roofline"]
    assert r["bound"] == bound and r["unit"] == ("TFLOP/s" if bound == "mfma" else "GB/s")
    assert 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["avg_launch_us"] > 0
    assert abs(line["value"] - line["config"]["global_batch"] / line["ms_per_step"] * 1e3) <= 0.01 * line["value"]
    # --dump-outputs: the last timed step's outputs, within 64 MB; its loss is the one the line reports
    files = os.listdir(dump)
    assert all(f.endswith(".npy") for f in files) and sum(os.path.getsize(dump / f) for f in files) <= 64 * 10 ** 6
    for need in ("total_loss.npy", "latents.z.npy", "rec.PA.loc.npy", "rec.text.logits.npy"):
        assert need in files, need
    assert any(f.startswith("klds.") for f in files) and any(f.startswith("log_probs.") for f in files)
    loss = float(np.load(dump / "total_loss.npy"))
    assert loss == pytest.approx(line["config"]["last_total_loss"], rel=1e-6)
    for f in files:
        assert np.isfinite(np.load(dump / f)).all(), f


def test_plain_bench_line(tmp_path):
    """a plain run (no --full): the headline fields and --dump-outputs as in a --full run, no roofline pass, no CPU baseline
    and no host-cost steps"""
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "4", "--warmup", "2",
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["metric"] == "samples/sec" and line["unit"] == "samples/sec" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 4 and line["warmup"] == 2 and line["value"] > 0
    assert abs(line["value"] - line["config"]["global_batch"] / line["ms_per_step"] * 1e3) <= 0.01 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert line["config"]["host_ms_per_step_call_idle_queue"] is None and line["config"]["hip_graph"] is True
    files = os.listdir(dump)
    assert "total_loss.npy" in files and "rec.text.logits.npy" in files
    assert float(np.load(dump / "total_loss.npy")) == pytest.approx(line["config"]["last_total_loss"], rel=1e-6)
