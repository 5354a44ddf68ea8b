"""scripts/run_test.py --evaluate_on_device: a labelled synthetic run scored with the matcher on the device writes the
metrics file a run without the flag writes (the sizes of tests/test_run_test_script_gpu.py's labelled run)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _metrics(out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run_test.py"), "--labelled", "--windows", "6", "--batch_size", "2",
           "--events_per_window", "4000", "--width", "240", "--height", "180", "--output_directory", str(out), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "metrics of the run (1 rank(s))" in r.stdout
    return json.load(open(out / "synthetic" / "detection" / "run_test" / "metrics.json"))


def test_run_test_evaluate_on_device_writes_the_same_metrics(tmp_path):
    host = _metrics(tmp_path / "host")
    device = _metrics(tmp_path / "device", "--evaluate_on_device")
    assert set(host) >= {"mAP", "mAP_50", "mAP_75"}
    assert device == host and list(device) == list(host)
