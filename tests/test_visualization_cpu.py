"""scripts/visualize_detections.py without a GPU: the reference's flags (the namespaces its own parser makes of the readme's
command lines, tests/golden/ref_py_viz.npz <- tests/make_golden_refpy_viz.py), and the run's refusals -- a missing DSEC
reader or dataset directory is an error, not a fallback; no --write_to_output (no window to show frames in) is an error
that names the flag.  The drawing itself is tests/test_visualization_gpu.py."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_refpy_viz import README_LINES  # noqa: E402  (the argv lists; the generator's main() is not run)

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ref_py_viz.npz"))
FLAGS = json.loads(str(GOLD["flags_json"]))


def _script():
    import visualize_detections
    return visualize_detections


@pytest.mark.parametrize("key", sorted(README_LINES))
def test_readme_command_line_parses_to_the_reference_namespace(key):
    ns = vars(_script().build_parser().parse_args(list(README_LINES[key])))
    want = FLAGS[key]
    assert set(ns) == set(want)
    for k, v in want.items():
        got = ns[k]
        if isinstance(got, Path):
            got = str(got)
        assert got == v and type(got) is type(v), (key, k, got, v)
    assert isinstance(ns["dataset_directory"], Path)
    assert ns["detections_folder"] is None or isinstance(ns["detections_folder"], Path)


def _detections_folder(tmp_path, sequence="zurich_city_13_b"):
    from dagr_amd.utils.buffers import DETECTION_DTYPE
    folder = tmp_path / "dets"
    folder.mkdir()
    np.save(folder / f"detections_{sequence}.npy", np.zeros(0, dtype=DETECTION_DTYPE))
    return folder


def test_missing_dataset_directory_is_an_error(tmp_path):
    det = _detections_folder(tmp_path)
    missing = tmp_path / "no_such_dsec"
    with pytest.raises(SystemExit) as e:
        _script().main(["--detections_folder", str(det), "--dataset_directory", str(missing), "--write_to_output"])
    assert str(missing) in str(e.value) and "does not exist" in str(e.value)
    assert not (det / "visualization").exists()


def test_missing_dsec_reader_is_an_error_not_a_fallback(tmp_path, monkeypatch):
    det = _detections_folder(tmp_path)
    monkeypatch.setitem(sys.modules, "dsec_det", None)          # importing it fails, installed or not
    with pytest.raises(SystemExit) as e:
        _script().main(["--detections_folder", str(det), "--dataset_directory", str(tmp_path), "--write_to_output"])
    assert "dsec_det" in str(e.value) and "no stand-in" in str(e.value)
    assert not (det / "visualization").exists()


def test_without_write_to_output_the_run_stops_and_names_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "visualize_detections.py"),
                        *README_LINES["readme:145-149"]], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--write_to_output" in r.stderr and "Traceback" not in r.stderr


def test_argument_checks_follow_the_reference(tmp_path):
    det = _detections_folder(tmp_path)
    base = ["--dataset_directory", str(tmp_path), "--write_to_output"]
    for bad in (["--vis_time_step_us", "0"], ["--event_time_window_us", "-5"]):
        with pytest.raises(SystemExit) as e:
            _script().main(base + ["--detections_folder", str(det)] + bad)
        assert "positive" in str(e.value)
    with pytest.raises(SystemExit) as e:                         # :29-31: --write_to_output needs the detections file
        _script().main(base)
    assert "--detections_folder" in str(e.value)
    with pytest.raises(SystemExit) as e:
        _script().main(base + ["--detections_folder", str(det), "--sequence", "thun_01_a"])
    assert "detections_thun_01_a.npy" in str(e.value)


def test_compute_index_restatement():
    ci = _script().compute_index
    ref = np.array([100, 200, 300])
    got = ci(ref, np.array([0, 99, 100, 150, 199, 200, 299, 300, 10 ** 6]))
    assert got.tolist() == [0, 0, 0, 0, 0, 1, 1, 2, 2]


def test_box_corners_truncate_toward_zero_and_class_ids_are_checked():
    from dagr_amd.visualization import bbox_viz as B
    x = np.array([1.9, -1.5, 10.0], dtype=np.float32)
    y = np.array([2.2, -0.5, 5.0], dtype=np.float32)
    w = np.array([3.3, 1.0, 0.4], dtype=np.float32)
    h = np.array([4.9, 0.2, 0.7], dtype=np.float32)
    corners, cls, scores = B.select_boxes(x, y, w, h, np.array([0, 1, 1]))
    assert scores is None and cls.tolist() == [0, 1, 1]
    assert corners.tolist() == [[int(x[i]), int(y[i]), int(x[i] + w[i]), int(y[i] + h[i])] for i in range(3)]
    with pytest.raises(IndexError):
        B.select_boxes(x, y, w, h, np.array([0, 2, 1]))
    with pytest.raises(ValueError):
        B.select_boxes(np.array([np.nan], np.float32), y[:1], w[:1], h[:1], np.array([0]))
    assert B.outline_colors().tolist() == [[0, 204, 25], [255, 170, 0]]
    assert B.label_colors(0) == ((0, 142, 17), (255, 255, 255)) and B.label_colors(1) == ((178, 119, 0), (0, 0, 0))
    assert B.label_text(1, np.float32(0.8731)) == "-pedestrian: 87.3"
