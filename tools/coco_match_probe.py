#!/usr/bin/env python
"""Evaluation time, host matcher against dagr_coco_match: the 64-image sweep of tests/coco_cases.py repeated to
``--images`` images (default 10 000), ``evaluate_detection`` with and without ``on_device``.  Prints one JSON line.

  python tools/coco_match_probe.py --images 10000
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                            # noqa: E402
from dagr_amd.utils import coco_eval as ce              # noqa: E402
from tests import coco_cases as cc                      # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--images", type=int, default=10000)
    a = p.parse_args()
    gts, dts = cc.random_sweep()
    reps = -(-a.images // len(gts))
    gts, dts = (gts * reps)[:a.images], (dts * reps)[:a.images]
    ce.evaluate_detection(gts[:64], dts[:64], classes=cc.CLASSES, on_device=True)        # library load, first launch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = {}
    dev = ce.evaluate_detection(gts, dts, classes=cc.CLASSES, on_device=True, stats=stats)
    t1 = time.perf_counter()
    images = ce.evaluated_images(gts, dts)
    t2 = time.perf_counter()
    jobs = ce.build_jobs(images, len(cc.CLASSES))
    t3 = time.perf_counter()
    ce.coco_match_device(jobs, list(range(len(jobs))), torch.device("cuda", torch.cuda.current_device()))
    t4 = time.perf_counter()
    host = ce.evaluate_detection(gts, dts, classes=cc.CLASSES)
    t5 = time.perf_counter()
    print(json.dumps({"images": len(gts), "jobs": len(jobs), "device_jobs": stats["device_jobs"], "equal": dev == host,
                      "evaluate_on_device_s": round(t1 - t0, 3), "evaluate_on_host_s": round(t5 - t4, 3),
                      "of_which_xywh_conversion_s": round(t2 - t1, 3), "job_list_s": round(t3 - t2, 3),
                      "upload_launch_copy_back_split_s": round(t4 - t3, 3), "AP": host["AP"]}))


if __name__ == "__main__":
    main()
