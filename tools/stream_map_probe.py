#!/usr/bin/env python
"""tools/stream_map_probe.py -- what detection mAP over every step costs on the device route (``EventStream(map=)``:
``dagr_stream_map_log`` per step, ``dagr_stream_map_plan`` + ``dagr_coco_match`` + ``dagr_coco_accumulate`` at the end) beside
the existing route on the same data (``DetectionBuffer(on_device=True, accumulate_on_device=True)``: ``update_device`` per
step, ``compute()`` with the job list built by numpy on the host), in one process.

``--part cost``: B = 1 and B = 8 lanes, 240 and 1200 images a lane, up to 64 ground-truth boxes and up to 100 detections an
image, two classes, synthetic boxes (detections are jittered ground truth plus false positives, scores in 64ths).  Per step:
``--launches`` calls back to back, wall clock with a device synchronisation on either side.  Per evaluation: wall clock around
the whole call, ``--rounds`` times; the existing route is refilled for every round (its ``compute()`` empties it).  The two
routes order the images differently (lane-major against step-major), which matters for ties in score only; both results
are printed.

``--part stream``: the step time of a B = 1 stream of the tiny test model with ``labels=``, with and without ``map_step()``
behind every step: ``--rounds`` rounds of ``--steps_timed`` steps each, alternating, no read-back inside a round; wall clock per
step, one device synchronisation at the end of the round.

Each part is one process; run them one at a time, each under a time limit of its own:

    timeout -k 10 400 python tools/stream_map_probe.py --part cost --commit <hash> --out profiles/stream_map.md && \\
    timeout -k 10 300 python tools/stream_map_probe.py --part stream --commit <hash> --out profiles/stream_map.md

``--out`` replaces the part's measured section of the file (between its two marker comments) and leaves the rest, which is
written by hand."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd import _lib                                                                  # noqa: E402
from dagr_amd import streaming as S                                                        # noqa: E402
from dagr_amd.utils import coco_eval as CE                                                 # noqa: E402
from dagr_amd.utils.buffers import DetectionBuffer                                         # noqa: E402

NAME = "tools/stream_map_probe.py"
G, A, CLASSES, POOL = 64, 100, ("car", "pedestrian"), 24


def markers(part):
    return (f"<!-- measured ({part}): written by {NAME} --part {part} --out, which replaces this section and nothing else -->",
            f"<!-- measured ({part}): end -->")


def write_section(path, part, text):
    begin, end = markers(part)
    old = open(path).read() if os.path.exists(path) else f"# {os.path.splitext(os.path.basename(path))[0]}\n"
    if begin in old and end in old:
        new = old[:old.index(begin)] + text.rstrip("\n") + old[old.index(end) + len(end):]
    else:
        new = old.rstrip("\n") + "\n\n" + text
    with open(path, "w") as f:
        f.write(new)


def cell(v, d=3):
    return f"{float(np.median(v)):.{d}f} ({min(v):.{d}f} .. {max(v):.{d}f})"


def step_pool(B, seed):
    """``POOL`` steps of B lanes: ``(det [B, A, 6], n_keep [B], gt_box [B, G, 4], gt_label [B, G], n_gt [B])`` as numpy."""
    rng, out = np.random.default_rng(seed), []
    for _ in range(POOL):
        n_gt = rng.integers(1, G + 1, B).astype(np.int32)
        xy, wh = rng.uniform(0, 500, (B, G, 2)), rng.uniform(8, 140, (B, G, 2))
        gt_box = np.concatenate([xy, xy + wh], -1).astype(np.float32)
        gt_label = rng.integers(0, 2, (B, G)).astype(np.int32)
        det, n_keep = np.zeros((B, A, 6), np.float32), np.zeros(B, np.int32)
        for b in range(B):
            hit = rng.random(n_gt[b]) < 0.8
            boxes = gt_box[b, :n_gt[b]][hit] + rng.normal(0, 3, (int(hit.sum()), 4))
            labels = gt_label[b, :n_gt[b]][hit]
            extra = int(rng.integers(0, A - len(boxes) + 1))
            fxy, fwh = rng.uniform(0, 500, (extra, 2)), rng.uniform(8, 140, (extra, 2))
            boxes = np.concatenate([boxes, np.concatenate([fxy, fxy + fwh], -1)])[:A]
            labels = np.concatenate([labels, rng.integers(0, 2, extra)])[:A]
            scores = rng.integers(1, 65, len(boxes)) / 64.0
            order = np.argsort(-scores, kind="stable")
            det[b, :len(boxes)] = np.concatenate([boxes, scores[:, None], labels[:, None]], 1)[order]
            n_keep[b] = len(boxes)
        out.append((det, n_keep, gt_box, gt_label, n_gt))
    return out


class Route:
    """Both routes on the same pool of steps, on the device."""

    def __init__(self, B, images):
        self.B, self.I, self.dev = B, images, torch.device("cuda:0")
        self.L, self.stream = _lib.lib(), _lib.cur_stream(torch.device("cuda:0"))
        host = step_pool(B, 100 + B)
        self.pool = [tuple(torch.from_numpy(v).to(self.dev) for v in s) for s in host]
        # the existing route's ground truth: one {boxes, labels} per image, device tensors cut by counts known on the host
        self.dicts = [[dict(boxes=d[2][b, :int(h[4][b])], labels=d[3][b, :int(h[4][b])].long()) for b in range(B)]
                      for d, h in zip(self.pool, host)]
        self.t_ref = [torch.full((B,), 1000 * k, dtype=torch.int64, device=self.dev) for k in range(POOL)]
        self.state = torch.empty(self.L.dagr_stream_map_bytes(B, images, G, A), dtype=torch.uint8, device=self.dev)
        self.plan = CE.StreamMapPlan(B, images, G, A, len(CLASSES), self.dev)
        self.buffer = DetectionBuffer(480, 640, CLASSES, on_device=True, accumulate_on_device=True)
        self.reset()

    def reset(self):
        _lib.check(self.L.dagr_stream_map_reset(_lib.ptr(self.state), self.state.numel(), self.B, self.I, G, A, self.stream), "reset")

    def log(self, k):
        P, (det, n_keep, box, label, n_gt) = _lib.ptr, self.pool[k % POOL]
        _lib.check(self.L.dagr_stream_map_log(P(self.state), self.state.numel(), self.B, self.I, G, A, P(det), P(n_keep), A, P(box),
                                              P(label), P(n_gt), P(self.t_ref[k % POOL]), self.stream), "dagr_stream_map_log")

    def update(self, k):
        det, n_keep = self.pool[k % POOL][:2]
        self.buffer.update_device(det, n_keep, self.dicts[k % POOL])

    def map(self):
        self.plan.run(self.state)
        tot, prec, _ = self.plan.precision()
        return CE.summarize(prec), tot


def wall(call, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(count):
        call(k)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / count


def part_cost(a):
    begin, end = markers("cost")
    steps, evals = [], []
    for B in (1, 8):
        for images in (240, 1200):
            r = Route(B, images)
            if images == 240:                               # per step: every timed call logs an image (the log is not full)
                count, ms_log, ms_upd = min(a.launches, images), [], []
                for _ in range(a.rounds):
                    r.reset()
                    ms_log.append(wall(r.log, count))
                    ms_upd.append(wall(r.update, count))
                    r.buffer._reset()
                steps.append((B, ms_log, ms_upd))
            ms_map, ms_compute, got, want, tot = [], [], None, None, None
            for _ in range(a.rounds):
                r.reset()
                for k in range(images):
                    r.log(k)
                    r.update(k)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got, tot = r.map()
                ms_map.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                want = r.buffer.compute(gather=False)
                ms_compute.append(1e3 * (time.perf_counter() - t0))
            evals.append((B, images, tot, ms_map, ms_compute, got["AP"], want["mAP"]))
            del r
            torch.cuda.empty_cache()
    lines = [begin, "", f"`{a.command}`, commit {a.commit}.", "",
             f"Per step, in one process: {a.launches} calls back to back, wall clock with a device synchronisation on either side, "
             f"{a.rounds} rounds; ms per call, median (min .. max) of the rounds.  B lanes, up to {G} ground-truth boxes and up to {A} "
             "detections an image.", "",
             "| B | `dagr_stream_map_log` (ms per step) | `DetectionBuffer.update_device` (ms per step) |", "|---|---|---|"]
    lines += [f"| {B} | {cell(x, 4)} | {cell(y, 4)} |" for B, x, y in steps]
    lines += ["", f"Per evaluation, same process and data: wall clock around the whole call, {a.rounds} rounds, ms, median (min .. max).  "
              "`map()`: `dagr_stream_map_plan`, the totals' read-back, `dagr_coco_match`, `score_order`, `dagr_coco_accumulate`, the "
              "precision array's read-back.  `compute()`: one copy of everything collected, `build_jobs` / `column_layout` / "
              "`accumulate_groups` in numpy, the upload, the same two kernels.  The AP columns differ only by the order of equal "
              "scores (lane-major against step-major images).", "",
              "| B | images a lane | jobs | columns | `map()` ms | `DetectionBuffer.compute()` ms | AP `map()` | AP `compute()` |",
              "|---|---|---|---|---|---|---|---|"]
    lines += [f"| {B} | {I} | {t['n_jobs']} | {t['n_out']} | {cell(x, 1)} | {cell(y, 1)} | {p:.6f} | {q:.6f} |"
              for B, I, t, x, y, p, q in evals]
    lines += ["", end]
    return "\n".join(lines) + "\n"


def part_stream(a):
    from tests.test_stream_rescue_gpu import _events, _step
    from tests.test_streaming_gpu import _model
    begin, end = markers("stream")
    model = _model(1)
    model.check_device_status = False
    rng = np.random.default_rng(5)
    R = 32
    xywh = np.concatenate([rng.uniform(0, 250, (R, 2)), rng.uniform(8, 40, (R, 2))], -1)
    events = [_events(k, lanes=1) for k in range(a.steps_timed + 20)]
    clock = int(np.asarray(events[0]["t_now"]).reshape(-1)[0])
    frames = [(clock - 1 + 50000 * f, xywh + 3.0 * f, rng.integers(0, 2, R).astype(np.int32), np.arange(1, R + 1, dtype=np.int64))
              for f in range(12)]
    stream = S.EventStream(model, window_us=20000, labels=dict(max_rows=R), map=dict(max_images=a.steps_timed + 20))
    per = {"step_device()": [], "step_device() + map_step()": []}
    with torch.no_grad():
        for _ in range(a.rounds + 1):                       # (the first round of either warms up and is not counted)
            for name in per:
                stream.reset()
                for t, x, lab, ids in frames:
                    stream.push_labels(np.array([t]), x[None], lab[None], ids[None])
                for k in range(20):
                    _step(stream, events[k])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(20, a.steps_timed + 20):
                    _step(stream, events[k])
                    if name != "step_device()":
                        stream.map_step()
                torch.cuda.synchronize()
                per[name].append(1e3 * (time.perf_counter() - t0) / a.steps_timed)
            counts = stream.map_counts()
        # map_step() with the device busy: the call returns while work enqueued in front of it is still running
        busy, host_ms, pending = torch.randn((8192, 8192), device=stream.device), [], 0
        stream.reset()
        for t, x, lab, ids in frames:
            stream.push_labels(np.array([t]), x[None], lab[None], ids[None])
        for k in range(a.rounds):
            _step(stream, events[k])
            for _ in range(12):
                busy @ busy
            marker = torch.cuda.Event()
            marker.record()
            t0 = time.perf_counter()
            stream.map_step()
            host_ms.append(1e3 * (time.perf_counter() - t0))
            pending += 0 if marker.query() else 1
            torch.cuda.synchronize()
    assert int(counts["images"][0]) == a.steps_timed, counts
    lines = [begin, "", f"`{a.command}`, commit {a.commit}.", "",
             f"B = 1, the tiny test model, `labels=dict(max_rows={R})`, `map=`: {a.rounds} rounds of {a.steps_timed} steps of 1 ms each "
             "after 20 warm-up steps, the two variants alternating on the same stream and events, nothing read back inside a "
             "round; wall clock per step with one device synchronisation at the end of the round; median (min .. max) of the "
             f"rounds.  Every timed `map_step()` logged an image ({int(counts['images'][0])} of them).", "",
             "| a step | ms per step |", "|---|---|"]
    lines += [f"| `{name}` | {cell(v[1:], 4)} |" for name, v in per.items()]
    lines += ["", f"`map_step()` with the device busy: a step, then twelve 8192 x 8192 fp32 matrix products and a marker event enqueued "
              f"in front of the call; host clock around `map_step()` alone, {a.rounds} rounds: {cell(host_ms, 4)} ms, and the marker "
              f"was still pending when the call returned in {pending} of {a.rounds} rounds."]
    lines += ["", end]
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("cost", "stream"), required=True)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps_timed", type=int, default=200)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    # the command as the sections print it: every flag that is not at its default, so that it reproduces the table
    given = [f" --{k} {getattr(a, k)}" for k in ("launches", "rounds", "steps_timed") if getattr(a, k) != ap.get_default(k)]
    a.command = f"python {NAME} --part {a.part}{''.join(given)} --commit {a.commit}"
    text = {"cost": part_cost, "stream": part_stream}[a.part](a)
    print(text)
    if a.out:
        write_section(a.out, a.part, text)


if __name__ == "__main__":
    main()
