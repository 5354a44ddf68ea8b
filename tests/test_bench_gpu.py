"""bench.py on the device, at a small size: a plain run measures the headline alone (and dumps its last step); `--full`
adds every other leg of the line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--events-per-window", "20000", "--engines", "2")
FULL_ONLY = {"events_only", "value_edges", "ms_per_step_edges", "value_h2d", "h2d", "roofline", "stages", "image_branch",
             "latency_ms", "async_update", "cpu_baseline"}


def _bench(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *flags], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "events_per_sec" and line["unit"] == "events/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * 20000 / (line["ms_per_step"] / 1e3), rel=1e-3)
    return line


def test_plain_run_is_the_headline_alone(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path / "dump"))
    assert not FULL_ONLY & set(line), sorted(FULL_ONLY & set(line))
    assert not {"edges_per_step", "level_nodes_edges", "stage_sum_ms"} & set(line["config"])
    det, n = np.load(tmp_path / "dump" / "detections.npy"), np.load(tmp_path / "dump" / "n_keep.npy")
    assert det.dtype == np.float32 and det.shape[0] == 2 and det.shape[2] == 6 and n.shape == (2,)
    assert np.isfinite(det).all() and (n >= 0).all() and (n <= det.shape[1]).all()


def test_full_run_adds_every_leg():
    line = _bench("--full", "--latency-n", "20000", "--latency-windows", "2", "--latency-warmup", "1",
                  "--cpu-steps", "1", "--cpu-batch", "1")
    assert FULL_ONLY <= set(line), sorted(FULL_ONLY - set(line))
    assert {"edges_per_step", "level_nodes_edges", "stage_sum_ms"} <= set(line["config"])
    assert set(line["latency_ms"]) == {"protocol", "events_only", "image_resnet50"}
    assert line["events_only"]["value"] > 0 and line["events_only"]["cpu_baseline"]["value"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["value_edges"] > 0 and line["value_h2d"] > 0
