#!/usr/bin/env python
"""tools/stream_cap_probe.py -- what a cap on the lanes' event count (``EventStream(max_lane_events=N)``) does to a stream
that is never read back: milliseconds per ``step_device``, calls of ``WindowEngine._alloc_events``, window-graph captures
and the final ``max_events``, for an uncapped stream and for one capped at ``--cap`` events.

B = 1, 640x480, S-edges, 1 ms steps, ``--steps`` ``step_device`` calls without a read-back, a resident window of about
``--resident`` events (``--window_us`` 50 ms), so the cap (32 768) is never reached: both streams compute the same windows,
and the difference is the bookkeeping -- the uncapped stream's bound is "every event pushed since the last read-back", the
capped stream's is ``B * N``.

Three streams run in this one process, each on a model (and engine) of its own with the same weights: uncapped, capped, and
a second capped one as the control that shows what two equal streams differ by.  After a warm-up that ends with the window
captured they advance in alternating blocks of ``--block`` steps over the same stretch of the stream.  Per step the host
clock around ``step_device`` is taken (host inputs: the packing and the upload of the new events are inside); a block ends
in a device synchronise -- no count or detection is read -- and its wall time per step is the second figure.  Reported per
stream: p50 and p99 of the per-step clock over all steps, the median and the min .. max of the blocks' p50s (the spread),
the same for the blocks' wall time per step.

    python tools/stream_cap_probe.py --out profiles/stream_cap.md"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd.model.networks.dagr import DAGR                    # noqa: E402
from dagr_amd.streaming import EventStream                       # noqa: E402
from dagr_amd.utils.args import model_args                       # noqa: E402
from dagr_amd.utils.testing_weights import randomize_            # noqa: E402
from tools.stream_probe import H, T0, W, make_stream             # noqa: E402


class Loop:
    """One stream on a model of its own; counts the engine's re-allocations and window captures after construction."""

    def __init__(self, ev, window_us, cap):
        torch.manual_seed(0)
        args = model_args("dagr-s", batch_size=1)
        self.model = randomize_(DAGR(args, height=H, width=W), seed=0).eval().cuda()
        self.model.cache_luts(width=W, height=H, radius=args.radius)
        self.model.check_device_status = False
        self.eng = self.model.engine()
        self.allocs, self.captures = [], 0
        alloc, capture = self.eng._alloc_events, self.eng._capture_window

        def counted_alloc(n):
            if n > self.eng.max_events:
                self.allocs.append(int(n))
            return alloc(n)

        def counted_capture(*a, **kw):
            self.captures += 1
            return capture(*a, **kw)
        self.eng._alloc_events, self.eng._capture_window = counted_alloc, counted_capture
        self.stream = EventStream(self.model, window_us=window_us, max_lane_events=cap)
        self.ev, self.ms, self.wall = ev, [], []

    def step(self, t_prev, t_now):
        x, y, t, p = self.ev
        i0, i1 = np.searchsorted(t, [t_prev, t_now], side="right")
        return self.stream.step_device(np.stack([x[i0:i1], y[i0:i1]], -1), t[i0:i1], p[i0:i1], t_now=t_now)

    def block(self, t_start, step_us, steps, keep=True):
        out = np.empty(steps)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        t_prev = t_start
        for k in range(steps):
            c0 = time.perf_counter()
            self.step(t_prev, t_prev + step_us)
            out[k] = time.perf_counter() - c0
            t_prev += step_us
        torch.cuda.synchronize()
        if keep:
            self.wall.append(1e3 * (time.perf_counter() - w0) / steps)
            self.ms.append(out * 1e3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resident", type=int, default=25000)
    ap.add_argument("--cap", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--step_us", type=int, default=1000)
    ap.add_argument("--window_us", type=int, default=50000)
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    blocks = a.steps // a.block
    ev = make_stream(a.resident, a.window_us, a.window_us + (a.warm + blocks * a.block + 8) * a.step_us)
    loops = {"uncapped": Loop(ev, a.window_us, None), f"capped at {a.cap}": Loop(ev, a.window_us, a.cap),
             f"capped at {a.cap} (control)": Loop(ev, a.window_us, a.cap)}
    names = list(loops)
    t = T0 + a.window_us
    with torch.no_grad():
        for loop in loops.values():                       # the first window in one push, then warmed until captured
            loop.step(T0, t)
            loop.block(t, a.step_us, a.warm, keep=False)
            assert loop.eng._wg is not None, "the window was not captured in the warm-up"
        t += a.warm * a.step_us
        warm = {k: (len(v.allocs), v.captures) for k, v in loops.items()}
        for r in range(blocks):
            for name in names[r % 3:] + names[:r % 3]:
                loops[name].block(t, a.step_us, a.block)
            t += a.block * a.step_us
    counts = {k: int(v.stream.counts().sum()) for k, v in loops.items()}
    lines = ["# A stream that is never read back: `EventStream(max_lane_events=N)` against the uncapped stream", "",
             f"`python tools/stream_cap_probe.py --out profiles/stream_cap.md` on {torch.cuda.get_device_name(0)}: B = 1, "
             f"{W}x{H}, S-edges, window {a.window_us} us, steps of {a.step_us} us ({int(a.resident * a.step_us / a.window_us)} "
             f"new events each), dagr-s events-only, random weights.  {blocks * a.block} `step_device` calls per stream "
             f"without a read-back, after a warm-up of 1 + {a.warm} steps that ends with the window captured; three streams "
             f"in one process, each on an engine of its own, in alternating blocks of {a.block} steps that end in a device "
             "synchronise.  Host clock around `step_device` (host inputs: packing and upload inside): p50 / p99 over all "
             "steps, and the median (min .. max) of the blocks' p50s; wall time per step of a block, synchronise included: "
             "median (min .. max) over the blocks.  `_alloc_events` calls and window-graph captures are counted after the "
             "warm-up (the warm-up's own: one capture each, no call).", "",
             "| stream | resident events at the end | p50 ms | p99 ms | blocks' p50 ms | block wall ms / step | "
             "`_alloc_events` calls | graph captures | final `max_events` |", "|---|---|---|---|---|---|---|---|---|"]
    for name, loop in loops.items():
        ms = np.concatenate(loop.ms)
        b50 = [float(np.median(m)) for m in loop.ms]
        lines.append(f"| {name} | {counts[name]} | {np.percentile(ms, 50):.3f} | {np.percentile(ms, 99):.3f} | "
                     f"{np.median(b50):.3f} ({min(b50):.3f} .. {max(b50):.3f}) | "
                     f"{np.median(loop.wall):.3f} ({min(loop.wall):.3f} .. {max(loop.wall):.3f}) | "
                     f"{len(loop.allocs) - warm[name][0]} | {loop.captures - warm[name][1]} | {loop.eng.max_events} |")
    un = loops["uncapped"]
    lines += ["", f"The uncapped stream's `_alloc_events` sizes: {un.allocs[warm['uncapped'][0]:]}; its slowest steps "
              f"(ms): {np.sort(np.concatenate(un.ms))[-4:].round(1).tolist()}; the capped stream's: "
              f"{np.sort(np.concatenate(loops[names[1]].ms))[-4:].round(1).tolist()}."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
