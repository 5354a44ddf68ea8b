#!/usr/bin/env python
"""tools/stream_probe.py -- milliseconds per detection on a sliding window: ``EventStream.step`` (the window slides on the
device, the host uploads the new events only) against the host-sliding loop a caller had to write before it (numpy cut of
a host-side stream, upload of the whole window, ``format_data``, ``model(x, reset=True)``).

B = 1, 640x480, S-edges; resident windows of about 25 k and 100 k events (``--window_us`` 50 ms), steps of 1 ms and 10 ms.
Both loops run in this one process on the same model, are warmed until the window is captured, and then run in
alternating blocks of ``--block`` steps; per loop the p50 of every block and the spread of the blocks' p50s are reported.
The clock is the host's, around the call that ends in the detections' read-back.

    python tools/stream_probe.py --out profiles/stream.md

The staging launches' own kernel time (k_stream_plan, k_stream_gather beside k_stage_window) comes from a separate
``rocprofv3 --kernel-trace --stats -- python tools/stream_probe.py --trace`` run: ``--trace`` plays a few steps of each
loop and nothing else."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd.data import Data                                   # noqa: E402
from dagr_amd.model.networks.dagr import DAGR                    # noqa: E402
from dagr_amd.streaming import EventStream                       # noqa: E402
from dagr_amd.utils import synthetic as syn                      # noqa: E402
from dagr_amd.utils.args import model_args                       # noqa: E402
from dagr_amd.utils.buffers import format_data                   # noqa: E402
from dagr_amd.utils.testing_weights import randomize_            # noqa: E402

W, H, TW = 640, 480, 1000000
T0 = 1 << 33


def make_stream(n_resident, window_us, duration_us, seed=5):
    """An S-edges stream of ``duration_us`` with ``n_resident`` events per ``window_us`` (absolute int64 timestamps)."""
    n = int(n_resident * duration_us / window_us)
    x, y, t, p = syn.edges_window(n, W, H, seed, window_us=duration_us, time_window=duration_us)
    return x, y, t.astype(np.int64) + T0, p


class HostLoop:
    """The loop written with the calls the engine had before the stream: the window lives on the host."""

    def __init__(self, model, ev, window_us):
        self.model, self.ev, self.window_us = model, ev, window_us
        self.dev = next(model.parameters()).device

    def step(self, t_prev, t_now):
        x, y, t, p = self.ev
        i0, i1 = np.searchsorted(t, [t_now - self.window_us, t_now], side="right")      # t_now - t < window_us, t <= t_now
        t_rel = (TW - (t_now - t[i0:i1])).astype(np.int32)
        d = Data(x=torch.from_numpy(p[i0:i1].reshape(-1, 1)), pos=torch.from_numpy(np.stack([x[i0:i1], y[i0:i1]], -1)),
                 t=torch.from_numpy(t_rel), width=W, height=H, time_window=TW).to(self.dev)
        d._geometry = (W, H, TW)
        return self.model(format_data(d), reset=True)[0]


class StreamLoop:
    def __init__(self, model, ev, window_us):
        self.stream, self.ev = EventStream(model, window_us=window_us), ev

    def step(self, t_prev, t_now):
        x, y, t, p = self.ev
        i0, i1 = np.searchsorted(t, [t_prev, t_now], side="right")                      # the events since the last step
        return self.stream.step(np.stack([x[i0:i1], y[i0:i1]], -1), t[i0:i1], p[i0:i1], t_now=t_now)


def run_block(loop, t_start, step_us, steps):
    out = np.empty(steps)
    t_prev = t_start
    for k in range(steps):
        t_now = t_prev + step_us
        c0 = time.perf_counter()
        loop.step(t_prev, t_now)
        out[k] = time.perf_counter() - c0
        t_prev = t_now
    return out * 1e3


def measure(model, n_resident, step_us, window_us, block, repeats):
    ev = make_stream(n_resident, window_us, window_us + (repeats * block + 8) * step_us)
    loops = {"stream": StreamLoop(model, ev, window_us), "host": HostLoop(model, ev, window_us)}
    t = T0 + window_us
    with torch.no_grad():
        loops["stream"].step(T0, t)                       # the first window in one push
        for loop in loops.values():                       # warmed until captured (two eager runs + the capture, each)
            run_block(loop, t, step_us, 8)
        loops["stream"].stream.reset()
        loops["stream"].step(T0, t)
        p50 = {k: [] for k in loops}
        for r in range(repeats):
            for name in ("stream", "host") if r % 2 == 0 else ("host", "stream"):
                if name == "host":
                    ms = run_block(loops["host"], t, step_us, block)
                else:
                    ms = run_block(loops["stream"], t, step_us, block)
                    t_stream_end = t + block * step_us
                p50[name].append(float(np.median(ms)))
            # both loops cover the same stretch of the stream in a repeat; the next repeat goes on from its end
            t = t_stream_end
    counts = int(loops["stream"].stream.counts().sum())
    return dict(n_resident=counts, step_us=step_us, new_per_step=int(n_resident * step_us / window_us),
                **{k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in p50.items()})


def trace(model, window_us=50000, n_resident=25000, step_us=1000, steps=12):
    ev = make_stream(n_resident, window_us, window_us + 2 * steps * step_us)
    with torch.no_grad():
        s = StreamLoop(model, ev, window_us)
        s.step(T0, T0 + window_us)
        run_block(s, T0 + window_us, step_us, steps)
        run_block(HostLoop(model, ev, window_us), T0 + window_us, step_us, steps)
    torch.cuda.synchronize()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resident", type=int, nargs="+", default=[25000, 100000])
    ap.add_argument("--step_us", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--window_us", type=int, default=50000)
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    args = model_args("dagr-s", batch_size=1)
    model = randomize_(DAGR(args, height=H, width=W), seed=0).eval().cuda()
    model.cache_luts(width=W, height=H, radius=args.radius)
    model.check_device_status = False                     # both loops: no status read-back inside the timed call
    if a.trace:
        trace(model, a.window_us)
        return
    rows = [measure(model, n, s, a.window_us, a.block, a.repeats) for n in a.resident for s in a.step_us]
    lines = ["# A detection per step on a sliding window: `EventStream.step` against the host-sliding loop", "",
             f"`python tools/stream_probe.py --out profiles/stream.md` on {torch.cuda.get_device_name(0)}: B = 1, {W}x{H}, "
             f"S-edges, window {a.window_us} us, dagr-s events-only, random weights.  Host clock around the call that ends "
             f"in the detections' read-back; both loops in one process, warmed until captured, alternating blocks of "
             f"{a.block} steps, {a.repeats} blocks each.  ms per step: median of the blocks' p50 (min .. max of the blocks' "
             "p50).", "",
             "| resident events | step | new events / step | `EventStream.step` | host loop (cut, upload, `format_data`, "
             "`model(x, reset=True)`) | stream / host |", "|---|---|---|---|---|---|"]
    for r in rows:
        s, h = r["stream"], r["host"]
        lines.append(f"| {r['n_resident']} | {r['step_us'] / 1000:g} ms | {r['new_per_step']} | {s[0]:.3f} ({s[1]:.3f} .. "
                     f"{s[2]:.3f}) | {h[0]:.3f} ({h[1]:.3f} .. {h[2]:.3f}) | {s[0] / h[0]:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
