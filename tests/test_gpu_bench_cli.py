"""bench.py as a command: a plain run times --steps steps and prints the result line
without the --full measurements; --dump-outputs writes the last timed step's outputs,
which equal a direct call of the same step bit for bit (the seeds depend only on the
arguments); --full adds the serialised probe, the roofline and the CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("kernels_ms_per_launch_serial", "roofline", "cpu_baseline", "cpu_baseline_reference")
R, STEPS = 96, 3


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--replicas", str(R), "--steps", str(STEPS), "--warmup", "1", *args],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path / "dump"
    line = _bench("--dump-outputs", str(d))
    assert line["metric"] == "redqueen_replicas_per_sec" and line["unit"] == "replicas/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == STEPS and line["full"] is False
    # the library counted the sweep launches of the timed region: one per step (two caller
    # streams, one chunk per call), so exactly STEPS steps were timed
    assert line["caller_streams"] == 2 and line["launches_per_step"] == 1.0
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - R / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert not [k for k in FULL_ONLY if k in line]
    got = {f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))}
    assert sorted(got) == ["counts", "means", "metrics", "status"]
    assert all(v.dtype == np.float64 for v in got.values())

    import bench
    from redqueen_amd import engine
    so, _ = bench.workload("c3")
    g = engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"],
                     so["end_time"])
    step, n, _ = bench.make_step("c3", g, so, R, 1, 0, torch.device("cuda", 0), (1,))
    assert n == R
    res, means = step(STEPS - 1)
    assert got["metrics"].shape == (R, 3) and got["counts"].shape == (R, 4)
    assert np.array_equal(got["metrics"], res.metrics.cpu().numpy())
    assert np.array_equal(got["counts"], res.counts.cpu().numpy())
    assert np.array_equal(got["status"], res.status.cpu().numpy())
    assert np.array_equal(got["means"], means.cpu().numpy())


def test_full_run_adds_probe_roofline_and_cpu_baseline():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    line = _bench("--full", "--cpu-sample", "16")
    assert line["full"] is True and line["steps"] == STEPS
    assert not [k for k in FULL_ONLY if k not in line]
    assert line["kernels_ms_per_launch_serial"]["sweep"] > 0
    assert line["roofline"]["kernel"] == "rq_sweep" and line["roofline"]["frac"] > 0
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["value"] > 0
