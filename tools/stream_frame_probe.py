#!/usr/bin/env python
"""tools/stream_frame_probe.py -- what a step of an ``EventStream`` costs on a ``--use_image`` model when a frame arrives
every 50 ms and a detection is asked for every millisecond, and what preparing a raw frame costs on the device.

B = 1, 640x480, S-edges, resnet50 and resnet18 trunks; resident windows of about 25 k and 100 k events (``--window_us``
50 ms), steps of 1 ms, a new frame (``image=``) every 50 ms.  Two loops run in this one process on the same model in
alternating blocks of ``--block`` steps: ``stream`` gives the frame when it changes, ``every_step`` gives it on every step
(every step then runs the image branch).  Per block the p50 of the steps that ran the frame body and of those that ran the
held body are taken (by ``EventStream.frame_steps``; on a commit without that counter a step counts as a frame step when
it brought a frame, so its frame-less steps are listed on their own); the report gives the median of the blocks' p50s and
their spread.  The clock is the host's, around the call that ends in the detections' read-back.

The same file runs on the parent commit: ``--json`` writes the numbers, ``--parent_json`` of a later run puts them beside
its own.  ``dagr_stream_frame`` (a 1280x960 BGR frame, factor 2) is timed between two device events against the host
preparation it replaces (``DSEC.preprocess_image`` + ``run_stream._frame``: crop, bicubic shrink, channel flip, upload,
``/ 255``), the host's clock around it including the upload.

    python tools/stream_frame_probe.py --json parent.json                  # on the parent commit
    python tools/stream_frame_probe.py --parent_json parent.json --out profiles/stream_frame.md"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd.model.networks.dagr import DAGR                    # noqa: E402
from dagr_amd.streaming import EventStream                       # noqa: E402
from dagr_amd.utils import synthetic as syn                      # noqa: E402
from dagr_amd.utils.args import model_args                       # noqa: E402
from dagr_amd.utils.testing_weights import randomize_            # noqa: E402

W, H = 640, 480
T0 = 1 << 33
FRAME_US = 50000


class Loop:
    """One stream on the model; ``every_step``: the frame is given on every step."""

    def __init__(self, model, ev, window_us, images, every_step):
        self.stream, self.ev, self.images, self.every_step = EventStream(model, window_us=window_us), ev, images, every_step
        self.last = None

    def step(self, t_prev, t_now):
        """Returns (milliseconds, "frame" | "held" | "frameless")."""
        x, y, t, p = self.ev
        i0, i1 = np.searchsorted(t, [t_prev, t_now], side="right")
        i = int((t_now - T0) // FRAME_US)
        image = self.images[i % len(self.images)] if (self.every_step or i != self.last) else None
        self.last = i
        before = getattr(self.stream, "frame_steps", None)
        c0 = time.perf_counter()
        self.stream.step(np.stack([x[i0:i1], y[i0:i1]], -1), t[i0:i1], p[i0:i1], t_now=t_now, image=image)
        ms = (time.perf_counter() - c0) * 1e3
        if before is None:
            return ms, "frame" if image is not None else "frameless"
        return ms, "frame" if self.stream.frame_steps > before else "held"


def run_block(loop, t_start, step_us, steps):
    kinds = {}
    t_prev = t_start
    for _ in range(steps):
        ms, kind = loop.step(t_prev, t_prev + step_us)
        kinds.setdefault(kind, []).append(ms)
        t_prev += step_us
    return {k: float(np.median(v)) for k, v in kinds.items()}


def measure(model, n_resident, step_us, window_us, block, repeats):
    duration = window_us + (repeats * block + 2 * block) * step_us
    n = int(n_resident * duration / window_us)
    x, y, t, p = syn.edges_window(n, W, H, 5, window_us=duration, time_window=duration)
    ev = (x, y, t.astype(np.int64) + T0, p)
    images = [torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(s)).cuda() for s in (1, 2, 3)]
    loops = {"stream": Loop(model, ev, window_us, images, False), "every_step": Loop(model, ev, window_us, images, True)}
    t = T0 + window_us
    p50 = {name: {} for name in loops}
    with torch.no_grad():
        for loop in loops.values():                       # the first window in one push, then warmed until captured
            loop.step(T0, t)
            run_block(loop, t, step_us, block)
        for loop in loops.values():
            loop.stream.reset()
            loop.step(T0, t + block * step_us)
        t += block * step_us
        for r in range(repeats):
            for name in ("stream", "every_step") if r % 2 == 0 else ("every_step", "stream"):
                for kind, ms in run_block(loops[name], t, step_us, block).items():
                    p50[name].setdefault(kind, []).append(ms)
            t += block * step_us
    out = dict(n_resident=int(loops["stream"].stream.counts().sum()), step_us=step_us)
    for name, kinds in p50.items():
        for kind, v in kinds.items():
            out[f"{name}.{kind}"] = (float(np.median(v)), float(min(v)), float(max(v)))
    return out


def frame_preparation(repeats=50):
    """(ms of dagr_stream_frame between two device events, ms of the host preparation on the host's clock) for a
    1280x960 BGR frame, factor 2; None for the first on a commit without the kernel."""
    from dagr_amd.data.dsec_data import _resize_area_free
    raw = np.random.default_rng(0).integers(0, 256, (2 * H, 2 * W, 3), dtype=np.uint8)
    dev = torch.device("cuda:0")

    def host():
        small = _resize_area_free(raw[:2 * H], W, H)[0].permute(1, 2, 0).numpy()           # DSEC.preprocess_image
        img = np.ascontiguousarray(small[..., ::-1])                                       # run_stream._frame
        out = torch.from_numpy(img).to(dev).permute(2, 0, 1).unsqueeze(0).float() / 255.0
        torch.cuda.synchronize()
        return out
    host()
    ms_host = []
    for _ in range(max(3, repeats // 5)):
        c0 = time.perf_counter()
        host()
        ms_host.append((time.perf_counter() - c0) * 1e3)
    ms_dev = ms_upload = None
    try:
        from dagr_amd.engine import StreamState
        st = StreamState(1, FRAME_US, dev)
        lanes = torch.zeros((1,), dtype=torch.int32, device=dev)
        frames = torch.from_numpy(raw)[None].to(dev)
        st.write_frames(frames, lanes, 2, 2, W, H, True)
        torch.cuda.synchronize()
        ms_dev, ms_upload = [], []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.write_frames(frames, lanes, 2, 2, W, H, True)
            e1.record()
            e1.synchronize()
            ms_dev.append(e0.elapsed_time(e1))
            c0 = time.perf_counter()
            frames = torch.from_numpy(raw)[None].to(dev)
            st.write_frames(frames, lanes, 2, 2, W, H, True)
            torch.cuda.synchronize()
            ms_upload.append((time.perf_counter() - c0) * 1e3)
        ms_dev, ms_upload = float(np.median(ms_dev)), float(np.median(ms_upload))
    except (ImportError, AttributeError):
        pass
    return dict(kernel_ms=ms_dev, upload_and_kernel_ms=ms_upload, host_ms=float(np.median(ms_host)))


def _cell(v):
    return "-" if v is None else f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nets", nargs="+", default=["resnet50", "resnet18"])
    ap.add_argument("--resident", type=int, nargs="+", default=[25000, 100000])
    ap.add_argument("--step_us", type=int, default=1000)
    ap.add_argument("--window_us", type=int, default=50000)
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--json", default=None, help="write the numbers here (the parent commit's run)")
    ap.add_argument("--parent_json", default=None, help="the parent commit's numbers, listed beside this run's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    res = dict(device=torch.cuda.get_device_name(0), rows=[], frame=frame_preparation())
    for net in a.nets:
        torch.manual_seed(0)
        args = model_args("dagr-s", batch_size=1, use_image=True, img_net=net)
        model = randomize_(DAGR(args, height=H, width=W), seed=0).eval().cuda()
        model.cache_luts(width=W, height=H, radius=args.radius)
        model.check_device_status = False                     # no status read-back inside the timed call
        for n in a.resident:
            res["rows"].append(dict(net=net, **measure(model, n, a.step_us, a.window_us, a.block, a.repeats)))
            print(json.dumps(res["rows"][-1]), flush=True)
        del model
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    parent = None
    if a.parent_json:
        with open(a.parent_json) as f:
            parent = json.load(f)
    lines = ["# EventStream on a `--use_image` model: the image branch once per frame, raw frames on the device", "",
             f"`python tools/stream_frame_probe.py --parent_json <the parent commit's --json> --out profiles/stream_frame.md` on "
             f"{res['device']}: B = 1, {W}x{H}, S-edges, window {a.window_us} us, steps of {a.step_us} us, a new frame every "
             f"{FRAME_US} us, dagr-s, random weights.  Host clock around `EventStream.step` (ends in the detections' "
             f"read-back).  Two loops in one process in alternating blocks of {a.block} steps, {a.repeats} blocks each: "
             "`stream` gives the frame when it changes, `every step` gives it on every step.  ms per step: median of the "
             "blocks' p50 (min .. max of the blocks' p50).  The parent commit's columns are the same file run on the parent "
             "commit in the same session; its frame-less steps run the whole window, image branch included.", "",
             "| trunk | resident events | held step | frame step | frame on every step | parent: frame-less step | "
             "parent: frame step | held / parent frame-less |", "|---|---|---|---|---|---|---|---|"]
    for k, r in enumerate(res["rows"]):
        pr = parent["rows"][k] if parent else {}
        held, pless = r.get("stream.held"), pr.get("stream.frameless")
        ratio = f"{held[0] / pless[0]:.2f}" if held and pless else "-"
        lines.append(f"| {r['net']} | {r['n_resident']} | {_cell(held)} | {_cell(r.get('stream.frame'))} | "
                     f"{_cell(r.get('every_step.frame'))} | {_cell(pless)} | {_cell(pr.get('stream.frame'))} | {ratio} |")
    fr = res["frame"]
    lines += ["", "## Preparing a raw frame", "",
              f"A {2 * W}x{2 * H} BGR uint8 frame to the model's fp32 [3, {H}, {W}] (crop, bicubic 2x shrink, channel flip, "
              "`/ 255`), medians:", "",
              "| | ms |", "|---|---|",
              f"| `dagr_stream_frame` between two device events (frame already on the device) | "
              f"{'-' if fr['kernel_ms'] is None else format(fr['kernel_ms'], '.3f')} |",
              f"| upload of the raw frame + `dagr_stream_frame`, host clock to the end of the kernel | "
              f"{'-' if fr['upload_and_kernel_ms'] is None else format(fr['upload_and_kernel_ms'], '.3f')} |",
              f"| host preparation (`DSEC.preprocess_image` + `run_stream._frame`), host clock to the end of the `/ 255` | "
              f"{fr['host_ms']:.3f} |"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
