#!/usr/bin/env python
"""Golden outputs of the reference's OWN visualisation code, executed on CPU (build container only: it imports
/root/reference/src and /root/reference/scripts).  numba's decorator is an identity, cv2 / torchvision / dsec_det are stubs;
torchvision's ``batched_nms`` is stood in for by its coordinate-offset trick over ``oracle.postprocess.nms``.  Pins, in
tests/golden/ref_py_viz.npz:

  * ``visualization/event_viz.draw_events_on_image`` on 48 x 64 images: repeated events on one pixel with mixed
    polarities, rows with y >= H, p in {0, 1} and in {-1, 1}, alpha 0.5 and 0.3, an empty event list; and one 480 x 640
    case (inputs re-drawn from a seed by the test, output stored as a SHA-256 digest)
  * ``visualization/bbox_viz.filter_boxes`` masks (strict ``scores > conf``, NMS over all the boxes)
  * the namespace the reference script's own parser (``scripts/visualize_detections.py:16-24``) makes of the readme's two
    command lines (readme.md:79-83, 145-149; ``$LOG_DIR`` / ``$WANDB_DIR`` / ``$DSEC_ROOT`` as literal placeholder
    paths) and of an empty one: the script runs with stub modules and stops right after ``parse_args``

tests/test_visualization_cpu.py and tests/test_visualization_gpu.py hold this repository's visualisation to them.

  python tests/make_golden_refpy_viz.py      ->  tests/golden/ref_py_viz.npz
"""
import argparse
import hashlib
import json
import os
import runpy
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

README_LINES = {
    "readme:79-83": ["--detections_folder", "/LOG_DIR/WANDB_DIR", "--dataset_directory", "data/DSEC_fragment/test",
                     "--vis_time_step_us", "1000", "--event_time_window_us", "5000", "--sequence", "zurich_city_13_b"],
    "readme:145-149": ["--detections_folder", "/LOG_DIR/WANDB_DIR", "--dataset_directory", "/DSEC_ROOT/test/",
                       "--vis_time_step_us", "1000", "--event_time_window_us", "5000", "--sequence", "zurich_city_13_b"],
    "empty": [],
}

SMALL_H, SMALL_W = 48, 64


def event_cases():
    """name -> (img, x, y, p, alpha): the small draw_events_on_image cases (also stored in the golden file)."""
    g = np.random.default_rng(7)
    img = lambda: g.integers(0, 256, (SMALL_H, SMALL_W, 3)).astype(np.uint8)
    cases = {}
    # one pixel hit many times with mixed polarities (the last event decides), plus a few other pixels
    n = 40
    x = np.concatenate([np.full(n, 10), g.integers(0, SMALL_W, 20)]).astype(np.uint16)
    y = np.concatenate([np.full(n, 7), g.integers(0, SMALL_H, 20)]).astype(np.uint16)
    p = g.integers(0, 2, n + 20).astype(np.uint8)
    cases["repeat_p01_a05"] = (img(), x, y, p, 0.5)
    # rows with y >= H among in-range rows (uint16 as DSEC stores them)
    x = g.integers(0, SMALL_W, 300).astype(np.uint16)
    y = g.integers(0, SMALL_H + 12, 300).astype(np.uint16)
    p = g.integers(0, 2, 300).astype(np.uint8)
    cases["rows_beyond_h_a05"] = (img(), x, y, p, 0.5)
    # p in {-1, 1} (the model's convention), int16 coordinates, dense hits
    x = g.integers(0, SMALL_W, 2000).astype(np.int16)
    y = g.integers(0, SMALL_H, 2000).astype(np.int16)
    p = (2 * g.integers(0, 2, 2000) - 1).astype(np.int8)
    cases["pm1_a05"] = (img(), x, y, p, 0.5)
    cases["pm1_a03"] = (img(), x, y, p, 0.3)
    x = g.integers(0, SMALL_W, 500).astype(np.uint16)
    y = g.integers(0, SMALL_H + 4, 500).astype(np.uint16)
    p = g.integers(0, 2, 500).astype(np.uint8)
    cases["p01_a03"] = (img(), x, y, p, 0.3)
    e = np.zeros(0, dtype=np.uint16)
    cases["empty"] = (img(), e, e, np.zeros(0, dtype=np.uint8), 0.5)
    return cases


def full_case(seed=123, n=60000):
    """The 480 x 640 case: a random BGR image and DSEC-typed events (uint16 x / y with some rows beyond H, uint8 p)."""
    g = np.random.Generator(np.random.PCG64(seed))
    img = g.integers(0, 256, (480, 640, 3)).astype(np.uint8)
    x = g.integers(0, 640, n).astype(np.uint16)
    y = g.integers(0, 500, n).astype(np.uint16)
    p = g.integers(0, 2, n).astype(np.uint8)
    return img, x, y, p, 0.5


def box_cases():
    """name -> (x, y, w, h, labels, scores, conf, nms) of float32 records-like inputs with overlapping clusters."""
    g = np.random.default_rng(31)
    cases = {}
    for k, (n, conf, nms) in enumerate([(60, 0.3, 0.65), (60, 0.5, 0.45), (200, 0.3, 0.65), (7, 0.3, 0.65)]):
        centres = g.uniform(20, 600, (max(1, n // 6), 2))
        c = centres[g.integers(0, len(centres), n)] + g.normal(0, 6, (n, 2))
        wh = g.uniform(20, 90, (n, 2))
        x, y = (c[:, 0] - wh[:, 0] / 2).astype(np.float32), (c[:, 1] - wh[:, 1] / 2).astype(np.float32)
        w, h = wh[:, 0].astype(np.float32), wh[:, 1].astype(np.float32)
        labels = g.integers(0, 2, n).astype(np.uint8)
        scores = g.uniform(0, 1, n).astype(np.float32)
        scores[: n // 10] = np.float32(conf)                 # exactly at the threshold: strict > drops them
        cases[f"boxes{k}"] = (x, y, w, h, labels, scores, conf, nms)
    z = np.zeros(0, dtype=np.float32)
    cases["boxes_empty"] = (z, z, z, z, np.zeros(0, dtype=np.uint8), z, 0.3, 0.65)
    return cases


def namespace_dict(ns):
    return {k: (str(v) if not isinstance(v, (int, float, bool, str, type(None))) else v) for k, v in vars(ns).items()}


def main():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refpy_fakes
    from make_golden_refpy_data import _mod
    from oracle.postprocess import nms as oracle_nms

    def batched_nms(boxes, scores, idxs, iou_threshold):     # torchvision's _batched_nms_coordinate_trick
        if boxes.numel() == 0:
            return torch.empty((0,), dtype=torch.int64)
        max_coordinate = boxes.max()
        offsets = idxs.to(boxes) * (max_coordinate + torch.tensor(1).to(boxes))
        return oracle_nms(boxes + offsets[:, None], scores, iou_threshold)

    ident = lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f))
    _mod("numba", njit=ident, jit=ident)
    _mod("cv2")
    _mod("torchvision")
    _mod("torchvision.ops", batched_nms=batched_nms)
    for m in ("dsec_det", "dsec_det.directory", "dsec_det.io", "dsec_det.preprocessing"):
        _mod(m)
    refpy_fakes.use_reference_package("/root/reference/src")
    import importlib
    rev = importlib.import_module("dagr.visualization.event_viz")
    rbb = importlib.import_module("dagr.visualization.bbox_viz")
    out = {}

    for name, (img, x, y, p, alpha) in event_cases().items():
        res = rev.draw_events_on_image(img.copy(), x, y, p, alpha)
        out.update({f"ev_{name}_img": img, f"ev_{name}_x": x, f"ev_{name}_y": y, f"ev_{name}_p": p,
                    f"ev_{name}_alpha": np.float64(alpha), f"ev_{name}_out": res})
    img, x, y, p, alpha = full_case()
    res = rev.draw_events_on_image(img.copy(), x, y, p, alpha)
    out["ev_full_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(res).tobytes()).digest(), dtype=np.uint8)
    out["ev_full_changed"] = np.array(int((res != img).any(-1).sum()))

    for name, (x, y, w, h, labels, scores, conf, nms) in box_cases().items():
        mask = rbb.filter_boxes(x, y, w, h, labels, scores, conf, nms)
        out.update({f"{name}_x": x, f"{name}_y": y, f"{name}_w": w, f"{name}_h": h, f"{name}_labels": labels,
                    f"{name}_scores": scores, f"{name}_conf": np.float64(conf), f"{name}_nms": np.float64(nms),
                    f"{name}_mask": np.asarray(mask, dtype=bool)})

    class _Parsed(Exception):
        pass

    parsed = {}
    real_parse = argparse.ArgumentParser.parse_args

    def stop_after_parse(self, args=None, namespace=None):
        raise _Parsed(real_parse(self, args, namespace))

    argv0 = list(sys.argv)
    argparse.ArgumentParser.parse_args = stop_after_parse
    try:
        for key, argv in README_LINES.items():
            sys.argv = ["visualize_detections.py"] + argv
            try:
                runpy.run_path("/root/reference/scripts/visualize_detections.py", run_name="__main__")
            except _Parsed as e:
                parsed[key] = namespace_dict(e.args[0])
            else:
                raise RuntimeError("the reference script did not reach parse_args")
    finally:
        argparse.ArgumentParser.parse_args = real_parse
        sys.argv = argv0
    out["flags_json"] = np.array(json.dumps(parsed, sort_keys=True))

    path = os.path.join(os.environ.get("GOLDEN_OUT", os.path.join(ROOT, "tests", "golden")), "ref_py_viz.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
    print("full case: pixels changed", int(out["ev_full_changed"]), "; masks:",
          {k[:-5]: int(v.sum()) for k, v in out.items() if k.endswith("_mask")})


if __name__ == "__main__":
    main()
