#!/usr/bin/env python
"""Accumulation time, host ``_accumulate`` against ``dagr_coco_accumulate``, on synthetic matched arrays: ``--images``
images x ``--dets`` detections, 2 classes x 4 area ranges = 8 groups (a detection belongs to one class and to all four
area ranges), 10 IoU thresholds.  The host side is ``coco_eval._accumulate`` once per group on the per-image tuples the
matcher hands over; the device side is ``coco_eval.accumulate_device`` (two sorts, two launches) on the same arrays already on
the GPU, up to the copy of the precision array.  The two results are compared bit for bit.  Prints one JSON line per
size; ``--out FILE`` also writes the table as markdown.

  python tools/coco_accumulate_probe.py --images 1000 10000 50000 --out profiles/coco_accumulate.md
"""
import argparse
import json
import os
import platform
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                      # noqa: E402
import torch                                            # noqa: E402
from dagr_amd.utils import coco_eval as ce              # noqa: E402

CLASSES, T = 2, len(ce.IOU_THRS)


def synthetic(n_images, dets, seed=0):
    """Per group the per-image tuples (scores sorted descending inside an image, dtm, dt_ign, g_ign) -- views of one array
    per group, columns image after image, which is the matcher's layout."""
    rng = np.random.default_rng(seed)
    per_class = dets // CLASSES
    groups = []
    for c in range(CLASSES):
        scores = -np.sort(-(rng.integers(1, 1025, (n_images, per_class)) / 1024.0), axis=1).reshape(-1)
        for a in range(len(ce.AREA_RNG)):
            n = n_images * per_class
            dtm, dt_ign = rng.uniform(size=(T, n)) < 0.6, rng.uniform(size=(T, n)) < (0.0 if a == 0 else 0.5)
            g_ign = rng.uniform(size=(n_images, 3)) < (0.0 if a == 0 else 0.5)
            groups.append([(scores[i * per_class:(i + 1) * per_class], dtm[:, i * per_class:(i + 1) * per_class],
                            dt_ign[:, i * per_class:(i + 1) * per_class], g_ign[i]) for i in range(n_images)])
    return groups


def on_host(groups):
    out = -np.ones((T, len(ce.REC_THRS), len(groups)))
    for g, entries in enumerate(groups):
        p = ce._accumulate(entries)
        if p is not None:
            out[:, :, g] = p
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--images", type=int, nargs="+", default=[1000, 10000, 50000])
    p.add_argument("--dets", type=int, default=100)
    p.add_argument("--host_repeats", type=int, default=1)
    p.add_argument("--device_repeats", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for n_images in a.images:
        groups = synthetic(n_images, a.dets)
        host_s = []
        for _ in range(a.host_repeats):
            t0 = time.perf_counter()
            want = on_host(groups)
            host_s.append(time.perf_counter() - t0)
        sizes = [sum(len(e[0]) for e in entries) for entries in groups]
        arrays = [np.concatenate([e[0] for entries in groups for e in entries]),
                  np.concatenate([e[1] for entries in groups for e in entries], 1),
                  np.concatenate([e[2] for entries in groups for e in entries], 1),
                  np.repeat(np.arange(len(groups)), sizes), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                  np.array([sum(int((~e[3]).sum()) for e in entries) for entries in groups], dtype=np.int64)]
        del groups
        arrays = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in arrays]
        dev_s = []
        for _ in range(a.device_repeats + 1):                            # the first call loads the code objects: not timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            precision, status = ce.accumulate_device(*arrays)
            got = precision.cpu().numpy()                                # the copy back ends the device work
            dev_s.append(time.perf_counter() - t0)
        assert status.item() == 0
        row = {"images": n_images, "detections": n_images * a.dets, "columns": int(sum(sizes)), "equal": bool(np.array_equal(got, want)),
               "host_s": round(min(host_s), 4), "host_repeats": a.host_repeats, "device_s": round(min(dev_s[1:]), 5),
               "device_s_max": round(max(dev_s[1:]), 5), "device_repeats": a.device_repeats,
               "speedup": round(min(host_s) / min(dev_s[1:]), 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del arrays
    if a.out:
        with open(a.out, "w") as f:
            f.write("# Accumulating COCO precision: host `_accumulate` against `dagr_coco_accumulate`\n\n"
                    f"Written by `tools/coco_accumulate_probe.py --images {' '.join(str(n) for n in a.images)} --dets {a.dets}`.\n\n"
                    f"* Box: {torch.cuda.get_device_name(dev)} (torch {torch.__version__}); host side on {platform.processor() or platform.machine()}, "
                    f"{os.cpu_count()} logical CPUs, numpy {np.__version__}, one thread.\n"
                    f"* Synthetic matched arrays: {a.dets} detections an image, {CLASSES} classes x {len(ce.AREA_RNG)} area ranges = "
                    f"{CLASSES * len(ce.AREA_RNG)} groups, {T} IoU thresholds, scores in steps of 1 / 1024 (ties).\n"
                    "* Host: `coco_eval._accumulate` once per group on the per-image tuples (concatenation, stable sort, cumulative\n"
                    "  sums, the envelope loop, `searchsorted`), the code of the parent commit.  Device: `coco_eval.accumulate_device` on\n"
                    "  the same arrays already on the GPU -- two stable `torch.sort`s for `perm`, the gather and the accumulate kernel --\n"
                    "  up to and including the copy back of the precision array.\n"
                    f"* Host time: best of {a.host_repeats} run(s).  Device time: best (and worst) of {a.device_repeats} runs after one "
                    "untimed run.\n* `equal`: `np.array_equal` of the two float64 precision arrays.\n\n"
                    "| images | columns (detections x 4 area ranges) | host s | device s (best) | device s (worst) | host / device | equal |\n"
                    "|---:|---:|---:|---:|---:|---:|:--|\n")
            for r in rows:
                f.write(f"| {r['images']} | {r['columns']} | {r['host_s']} | {r['device_s']} | {r['device_s_max']} | {r['speedup']} | "
                        f"{r['equal']} |\n")
            f.write("\nWhat is not in these numbers: the matcher, the upload of the job list and the rest of `evaluate_detection`,\n"
                    "which are the same on both sides.\n")


if __name__ == "__main__":
    main()
