"""GPU: bench.py on one GPU.  A plain run prints the headline and writes --dump-outputs, nothing else; `--full` adds what
is measured or checked besides the headline (here the parts that take seconds, not minutes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS = 6 * 450 * 800
FULL_ONLY = ("roofline", "cpu_baseline", "gpu_torch_baseline", "roofline_msda", "roofline_linear", "roofline_bwd",
             "strong_scaling", "extras", "parity", "hot_path", "detail_file")


def _bench_line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--preheat", "2",
           *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_the_dumped_outputs(tmp_path):
    line = _bench_line("--dump-outputs", str(tmp_path))
    assert line["metric"] == "rendered rays/sec (6-cam 450x800, 128 samples/ray)" and line["unit"] == "rays/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1
    assert abs(line["value"] - RAYS / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
    assert [k for k in FULL_ONLY if k in line] == []
    assert "parity_of_timed_frame" not in line["config"] and "hot_path_ms" not in line["config"]
    dumped = line["outputs_dumped"]
    assert dumped["arrays"] == ["acc", "depth", "fars", "max_depth", "nears"] and dumped["rays"] == dumped["of_rays"] == RAYS
    for k in dumped["arrays"]:
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == (RAYS,), k
        assert k not in ("depth", "acc") or np.isfinite(a).all(), k


def test_full_run_adds_the_kernel_roofline_and_the_detail_file():
    line = _bench_line("--full", "--no-cpu-baseline", "--no-extras", "--no-hotpath")
    assert abs(line["value"] - RAYS / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and roof["kernel_ms"] > 0 and 0 < roof["frac"] < 1
    assert line["cpu_baseline"] is None and "parity" not in line and "hot_path" not in line and "extras" not in line
    assert line["detail_file"] == "bench_out/bench_detail.json"
    with open(os.path.join(ROOT, line["detail_file"])) as f:
        detail = json.load(f)
    assert detail["line"]["value"] == line["value"] and detail["detail"]["roofline"]["kernel_ms"] == roof["kernel_ms"]
