#!/usr/bin/env python
"""What the training augmentations cost on the host and on the device, and what the training step makes of the difference.

For B = 8 samples of 50 k synthetic events at 240 x 180 and 640 x 480, with and without frames:
  * the host chain (``Augmentations.transform_training`` sample by sample + collate), with one torch thread and with the
    thread count the process starts with (the loader runs in the training process);
  * the device call (``DeviceAugmentations`` on the collated batch): HIP events around 50 calls after 10 warm-up calls, and
    the host clock around the same calls (each call ends in its read of the surviving-event count);
then ``scripts/train_ncaltech101.py --max_iters N`` on the synthetic stream with and without ``--augment_on_device``, the two
variants alternating, each in a process of its own.  Writes a markdown report.

  python tools/augment_probe.py --out profiles/augment_device.md
"""
import argparse
import os
import platform
import re
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dagr_amd.data import Batch  # noqa: E402
from dagr_amd.data.augment import Augmentations, init_transforms  # noqa: E402
from dagr_amd.data.utils import to_data  # noqa: E402
from dagr_amd.utils import synthetic as syn  # noqa: E402

ARGS = types.SimpleNamespace(aug_p_flip=0.5, aug_zoom=1.5, aug_trans=0.1)
FOLLOW = ["bbox", "bbox0"]


def samples(B, n, W, H, frames):
    out = []
    for b in range(B):
        x, y, t, p = syn.uniform_window(n, W, H, seed=100 + b)
        box = np.array([[W / 4, H / 4, W / 3, H / 3, b % 2, 1]], np.float32)
        d = to_data(x=x, y=y, t=t, p=p, bbox=box, width=W, height=H, time_window=1000000)
        if frames:
            d.bbox0 = d.bbox.clone()
            d.image = torch.randint(0, 256, (1, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(b))
        out.append(d)
    return out


def host_ms(aug, data, reps, threads):
    was = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        times = []
        for r in range(reps + 2):
            t0 = time.perf_counter()
            Batch.from_data_list([aug.transform_training(d.clone()) for d in data], follow_batch=FOLLOW)
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times[2:]))
    finally:
        torch.set_num_threads(was)


def device_ms(dev_aug, batch, warmup=10, calls=50):
    for _ in range(warmup):
        dev_aug(batch)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        dev_aug(batch)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls, (time.perf_counter() - t0) * 1e3 / calls


def train_seconds(flag, iters, preset_args):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_ncaltech101.py"), "--max_iters", str(iters)] + preset_args
    if flag:
        cmd.append("--augment_on_device")
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    m = re.search(r"epoch 0: loss (\S+)\s+lr \S+\s+([0-9.]+) s", r.stdout)
    return float(m.group(2)), float(m.group(1))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_device.md"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--events", type=int, default=50000)
    ap.add_argument("--host_reps", type=int, default=5)
    ap.add_argument("--train_iters", type=int, default=200, help="0 skips the training runs")
    ap.add_argument("--train_rounds", type=int, default=2)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("augment_probe.py measures on the GPU; no device is visible")
    dev = torch.device("cuda", 0)
    threads = torch.get_num_threads()
    lines = ["# Training augmentations: host chain vs device chain", "",
             f"Box: {torch.cuda.get_device_name(0)}, {len(os.sched_getaffinity(0))} host cores available to the process "
             f"({platform.processor() or platform.machine()}), torch {torch.__version__}, {threads} torch threads by default.",
             "", f"B = {a.batch} samples x {a.events} events, `aug_p_flip=0.5 aug_zoom=1.5 aug_trans=0.1`.  Host: median of "
             f"{a.host_reps} batches (chain sample by sample + collate).  Device: 50 calls after 10 warm-up calls, HIP events "
             "(and the host clock around the same calls; every call ends in one read-back).", "",
             "| sensor | frames | host, 1 thread (ms) | host, default threads (ms) | device, HIP events (ms) | device, host clock (ms) |",
             "|---|---|---|---|---|---|"]
    for W, H in ((240, 180), (640, 480)):
        for frames in (False, True):
            aug = Augmentations(ARGS)
            init_transforms(aug.transform_training.transforms, H, W)
            dev_aug = aug.transform_training_device
            dev_aug.init(H, W)
            data = samples(a.batch, a.events, W, H, frames)
            h1, hn = host_ms(aug, data, a.host_reps, 1), host_ms(aug, data, a.host_reps, threads)
            batch = Batch.from_data_list(data, follow_batch=FOLLOW).to(dev)
            d_ev, d_host = device_ms(dev_aug, batch)
            lines.append(f"| {W} x {H} | {'uint8 [B, 3, H, W]' if frames else 'none'} | {h1:.2f} | {hn:.2f} | {d_ev:.3f} | "
                         f"{d_host:.3f} |")
            print(lines[-1], flush=True)
    if a.train_iters > 0:
        preset = ["--config", "config/dagr-l-ncaltech.yaml", "--batch_size", str(a.batch), "--n_nodes", str(a.events),
                  "--samples", str(a.batch * a.train_iters), "--aug_zoom", "1.5", "--output_directory",
                  os.path.join(os.environ.get("TMPDIR", "/tmp"), "augment_probe_logs")]
        rows = []
        for r in range(a.train_rounds):
            for flag in (False, True):
                secs, loss = train_seconds(flag, a.train_iters, preset)
                rows.append((r, flag, secs, loss))
                print(rows[-1], flush=True)
        lines += ["", f"`scripts/train_ncaltech101.py {' '.join(preset[:-2])} --max_iters {a.train_iters}` on the synthetic "
                  "stream (`SyntheticObjects`, at most 20 k events per sample), wall time of the training loop over its "
                  "iterations, first iterations included; the two variants alternate, one process each.", "",
                  "| round | augmentations | loop (s) | per step (ms) | mean loss |", "|---|---|---|---|---|"]
        for r, flag, secs, loss in rows:
            lines.append(f"| {r} | {'device (--augment_on_device)' if flag else 'host (loader)'} | {secs:.1f} | "
                         f"{secs / a.train_iters * 1e3:.1f} | {loss:.4f} |")
        host = np.mean([s for _, f, s, _ in rows if not f]) / a.train_iters * 1e3
        devm = np.mean([s for _, f, s, _ in rows if f]) / a.train_iters * 1e3
        spread = max(abs(rows[i][2] - rows[j][2]) for i in range(len(rows)) for j in range(len(rows))
                     if rows[i][1] == rows[j][1]) / a.train_iters * 1e3
        lines += ["", f"Mean per step: host {host:.1f} ms, device {devm:.1f} ms; the same variant differs by up to "
                  f"{spread:.1f} ms per step between rounds."
                  + ("  The step time does not move beyond that spread." if abs(host - devm) <= spread else "")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
