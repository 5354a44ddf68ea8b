#!/usr/bin/env python
"""Twin of the reference's ``scripts/visualize_detections.py`` (:16-80): draws the detections that
``run_test_interframe.py`` wrote (``detections_<sequence>.npy``) over the events and frames of a DSEC sequence, one output
frame every ``--vis_time_step_us`` with the events of the last ``--event_time_window_us``.  Same flags and defaults as the
reference's parser.  The drawing runs on the device, up to 64 frames per call (``dagr.visualization.render_frames``);
the frames are read exactly as the reference reads them, with dsec_det, one call per frame.

Differences, on purpose:
* frames are only written (``--write_to_output``, PNGs in ``<detections_folder>/visualization``): there is no window
  backend for the reference's ``cv2.imshow``, so a run without the flag stops with an error;
* a missing dsec_det / h5py / hdf5plugin, or a missing ``--dataset_directory``, is an error: there is no stand-in data;
* label texts use PIL's default font, not OpenCV's (see ``dagr.visualization.bbox_viz``).

``main(argv, source=...)`` takes any object with ``t_range()``, ``image_timestamps``, ``image(i)`` (BGR uint8) and
``events(t0, t1)`` in place of the DSEC sequence; for such a source the reference's ``compute_index`` is restated below.
"""
import argparse
import collections
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr.visualization.bbox_viz import box_rows, draw_labels, select_boxes   # noqa: E402
from dagr.visualization.frames import render_frames                           # noqa: E402

CHUNK = 64          # frames per device call
SCALE = 2           # the detections are in half resolution (:70)
CONF, NMS = 0.3, 0.65


def build_parser():
    parser = argparse.ArgumentParser("""Visualization script to show bounding boxes""")
    parser.add_argument("--detections_folder", help="Path to folder with detections.", type=Path)
    parser.add_argument("--dataset_directory", help="Path to DSEC folder including which split.", type=Path,
                        default="/data/scratch1/daniel/datasets/DSEC_fragment/test")
    parser.add_argument("--vis_time_step_us", help="Number of microseconds to step each iteration.", type=int,
                        default=1000)
    parser.add_argument("--event_time_window_us", help="Length of sliding event time window for visualization.", type=int,
                        default=5000)
    parser.add_argument("--sequence", help="Sequence to visualize. Must be an official DSEC sequence e.g. zurich_city_13_b",
                        default="zurich_city_13_b", type=str)
    parser.add_argument("--write_to_output", help="Whether to save images in folder ${detections_folder}/visualization. "
                        "Otherwise, just cv2.imshow is used.", action="store_true")
    return parser


def compute_index(ref_timestamps, timestamps):
    """Index of the most recent reference timestamp at or before each timestamp, clipped to the valid range.  A
    restatement of dsec_det's ``compute_index`` for injected sources; dsec_det was not available to check it against."""
    ref_timestamps = np.asarray(ref_timestamps)
    return np.clip(np.searchsorted(ref_timestamps, timestamps, side="right") - 1, 0, len(ref_timestamps) - 1)


class DSECSource:
    """One DSEC sequence read through dsec_det, exactly as the reference script reads it (:37-62)."""

    def __init__(self, directory):
        from dsec_det.directory import DSECDirectory
        from dsec_det.io import extract_from_h5_by_timewindow, extract_image_by_index, load_start_and_end_time
        from dsec_det.preprocessing import compute_index as dsec_compute_index
        self.directory = DSECDirectory(directory)
        self._extract_events, self._extract_image = extract_from_h5_by_timewindow, extract_image_by_index
        self._t_range = load_start_and_end_time
        self.compute_index = dsec_compute_index

    def t_range(self):
        return self._t_range(self.directory)

    @property
    def image_timestamps(self):
        return self.directory.images.timestamps

    def image(self, i):
        return self._extract_image(self.directory.images.image_files_distorted, i)

    def events(self, t0, t1):
        return self._extract_events(self.directory.events.event_file, t0, t1)


def open_dsec(args):
    if not args.dataset_directory.exists():
        raise SystemExit(f"visualize_detections.py: --dataset_directory {args.dataset_directory} does not exist")
    missing = []
    for name in ("dsec_det", "h5py", "hdf5plugin"):
        try:
            __import__(name)
        except ImportError:
            missing.append(name)
    if missing:
        raise SystemExit(f"visualize_detections.py: reading a DSEC sequence needs {', '.join(missing)}, which is not "
                         f"installed; there is no stand-in data for this script")
    return DSECSource(args.dataset_directory / args.sequence)


def visualize(args, source, emit, detections=None, chunk=CHUNK):
    """Render every frame of ``np.arange(t0, t1, vis_time_step_us)`` and hand ``emit(step, frame)`` each one (BGR uint8,
    host) in step order.  ``detections``: the records of ``detections_<sequence>.npy``, or None for events and images
    only."""
    index = getattr(source, "compute_index", compute_index)
    t0, t1 = source.t_range()
    vis_timestamps = np.arange(t0, t1, step=args.vis_time_step_us)
    image_index = index(source.image_timestamps, vis_timestamps)
    if detections is not None:
        detection_timestamps = np.unique(detections["t"])
        boxes_index = index(detection_timestamps, vis_timestamps)
    selected = {}                         # detection timestamp index -> its filtered boxes (consecutive steps share them)
    for c0 in range(0, len(vis_timestamps), chunk):
        steps = range(c0, min(c0 + chunk, len(vis_timestamps)))
        uniq, frame_image = np.unique(image_index[steps.start:steps.stop], return_inverse=True)
        images = np.stack([np.asarray(source.image(int(i)), dtype=np.uint8) for i in uniq])
        xs, ys, ps, ev_ptr = [], [], [], [0]
        for s in steps:
            t = vis_timestamps[s]
            ev = source.events(t - args.event_time_window_us, t)
            xs.append(np.asarray(ev["x"]).astype(np.int32))
            ys.append(np.asarray(ev["y"]).astype(np.int32))
            ps.append(np.asarray(ev["p"]))
            ev_ptr.append(ev_ptr[-1] + len(xs[-1]))
        per_frame, rows, box_ptr = [], [], [0]
        if detections is not None:
            for s in steps:
                k = int(boxes_index[s])
                if k not in selected:
                    selected.clear()
                    b = detections[detections["t"] == detection_timestamps[k]]
                    sel = select_boxes(SCALE * b["x"], SCALE * b["y"], SCALE * b["w"], SCALE * b["h"], b["class_id"],
                                       b["class_confidence"], conf=CONF, nms=NMS)
                    selected[k] = sel + (box_rows(sel[0], sel[1]),)
                per_frame.append(selected[k])
                rows.append(selected[k][3])
                box_ptr.append(box_ptr[-1] + len(selected[k][3]))
        p_all = np.concatenate(ps) if ps else np.zeros(0, np.int8)
        out = render_frames(images, frame_image.reshape(-1), np.concatenate(xs), np.concatenate(ys), p_all, ev_ptr,
                            boxes=np.concatenate(rows) if detections is not None else None,
                            box_ptr=box_ptr if detections is not None else None)
        host = out.cpu().numpy()
        for j, s in enumerate(steps):
            if detections is not None:
                corners, cls, scores, _ = per_frame[j]
                draw_labels(host[j], corners, cls, scores)
            emit(s, host[j])
    return len(vis_timestamps)


class PNGWriter:
    """``%06d.png`` files from BGR frames (RGB on disk, as cv2.imwrite writes them), on a small thread pool; at most a
    few chunks of frames wait in memory."""

    def __init__(self, directory, max_pending=4 * CHUNK):
        from PIL import Image
        self.Image = Image
        self.directory = Path(directory)
        self.pool = ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0))))
        self.pending = collections.deque()
        self.max_pending = max_pending

    def _write(self, step, frame):
        self.Image.fromarray(np.ascontiguousarray(frame[..., ::-1])).save(self.directory / ("%06d.png" % step))

    def __call__(self, step, frame):
        self.pending.append(self.pool.submit(self._write, step, frame))
        while len(self.pending) > self.max_pending:
            self.pending.popleft().result()

    def close(self):
        try:
            while self.pending:
                self.pending.popleft().result()
        finally:
            self.pool.shutdown(wait=True)


def main(argv=None, source=None):
    args = build_parser().parse_args(argv)
    if not args.write_to_output:
        raise SystemExit("visualize_detections.py: frames cannot be shown in a window here (the reference uses "
                         "cv2.imshow); pass --write_to_output to write them to <detections_folder>/visualization")
    if args.vis_time_step_us <= 0 or args.event_time_window_us <= 0:
        raise SystemExit("visualize_detections.py: --vis_time_step_us and --event_time_window_us must be positive")
    detections_file = None if args.detections_folder is None else \
        args.detections_folder / f"detections_{args.sequence}.npy"
    if detections_file is None or not detections_file.exists():
        raise SystemExit(f"visualize_detections.py: --write_to_output needs --detections_folder holding "
                         f"detections_{args.sequence}.npy (got {detections_file})")
    if source is None:
        source = open_dsec(args)
    output_path = args.detections_folder / "visualization"
    output_path.mkdir(parents=True, exist_ok=True)
    writer = PNGWriter(output_path)
    try:
        n = visualize(args, source, writer, detections=np.load(detections_file))
    finally:
        writer.close()
    print(f"wrote {n} frames to {output_path}")
    return n


if __name__ == "__main__":
    main()
