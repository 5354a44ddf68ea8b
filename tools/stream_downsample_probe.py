#!/usr/bin/env python
"""tools/stream_downsample_probe.py -- milliseconds per step of an event stream fed RAW sensor events, three ways:

  a  ``dagr.data.downsample.downsample_events`` per push (change map carried by the caller), the row cut, then
     ``EventStream.step`` on the survivors: the only route before the stream had a front;
  b  ``EventStream(downsample=2).step`` on the raw push: the front on the device, no host synchronisation before the
     detections' read-back;
  c  ``EventStream.step`` fed survivors computed beforehand: the floor, so b - c is the front's own cost.

B = 1, a 640x480 sensor over the 320x215 model, 1 ms steps on a 50 ms window, about ``--raw_per_step`` raw events per step.
The synthetic generators at sensor resolution hardly survive a 2x downsampling, so the raw stream is built from a
model-resolution S-edges stream: every event repeated 3 to 6 times at ``(2x + {0,1}, 2y + {0,1}, t + {0,1,2})`` with the
same polarity, sorted stably by ``t``.  All legs take host arrays (the upload is part of a step), run in this one process on
the same model, are warmed until the window is captured and then run in alternating blocks of ``--block`` steps over the
same stretch of the stream; the clock is the host's around the call that ends in the detections' read-back.

    python tools/stream_downsample_probe.py --commit <hash> --out profiles/stream_downsample.md

The front's launches by name come from ``rocprofv3 --kernel-trace --stats -- python tools/stream_downsample_probe.py
--trace`` (a few steps of leg b and nothing else)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd.data.downsample import downsample_events           # noqa: E402
from dagr_amd.model.networks.dagr import DAGR                    # noqa: E402
from dagr_amd.streaming import EventStream                       # noqa: E402
from dagr_amd.utils import synthetic as syn                      # noqa: E402
from dagr_amd.utils.args import model_args                       # noqa: E402
from dagr_amd.utils.testing_weights import randomize_            # noqa: E402

W, H, F = 320, 215, 2
W_IN, H_IN = 640, 480
CW, CH = W_IN // F, H_IN // F
T0 = 1 << 33


def make_raw_stream(raw_per_step, step_us, duration_us, seed=5):
    n_base = int(raw_per_step / 4.5 * duration_us / step_us)
    x, y, t, p = syn.edges_window(n_base, CW, CH, seed, window_us=duration_us, time_window=duration_us)
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    rep = rng.integers(3, 7, len(t))
    x, y, t, p = (np.repeat(np.asarray(v), rep) for v in (x, y, t, p))
    m = len(t)
    x = x.astype(np.int64) * 2 + rng.integers(0, 2, m)
    y = y.astype(np.int64) * 2 + rng.integers(0, 2, m)
    t = np.int64(T0) + t.astype(np.int64) + rng.integers(0, 3, m)
    o = np.argsort(t, kind="stable")
    return np.stack([x[o], y[o]], -1).astype(np.int16), t[o], p[o].astype(np.int8)


class Leg:
    def __init__(self, ev):
        self.xy, self.t, self.p = ev

    def cut(self, t_prev, t_now):
        i0, i1 = np.searchsorted(self.t, [t_prev, t_now], side="left")
        return self.xy[i0:i1], self.t[i0:i1], self.p[i0:i1]


class HostRoute(Leg):
    """a: downsample_events per push, the row cut, step on the survivors."""

    def __init__(self, model, ev, window_us):
        super().__init__(ev)
        self.stream = EventStream(model, window_us=window_us)
        self.dev = self.stream.device
        self.map = torch.zeros((CH, CW), dtype=torch.float32, device=self.dev)

    def survivors(self, t_prev, t_now):
        xy, t, p = self.cut(t_prev, t_now)
        d_xy = torch.from_numpy(xy).to(self.dev)
        ev = dict(x=d_xy[:, 0].contiguous(), y=d_xy[:, 1].contiguous(), t=torch.from_numpy(t).to(self.dev),
                  p=torch.from_numpy(p).to(self.dev))
        out, self.map = downsample_events(ev, H_IN, W_IN, CH, CW, change_map=self.map)
        m = (out["x"] < W) & (out["y"] < H)
        return torch.stack([out["x"][m], out["y"][m]], -1).to(torch.int16), out["t"][m], out["p"][m]

    def step(self, t_prev, t_now):
        xy, t, p = self.survivors(t_prev, t_now)
        return self.stream.step(xy, t, p, t_now=torch.tensor([t_now], dtype=torch.int64).to(self.dev))


class FrontRoute(Leg):
    """b: the raw push into a downsampling stream."""

    def __init__(self, model, ev, window_us):
        super().__init__(ev)
        self.stream = EventStream(model, window_us=window_us, downsample=F, sensor_size=(W_IN, H_IN))

    def step(self, t_prev, t_now):
        xy, t, p = self.cut(t_prev, t_now)
        return self.stream.step(xy, t, p, t_now=t_now)


class Floor(Leg):
    """c: survivors computed beforehand (host arrays, as the raw events are)."""

    def __init__(self, model, ev, window_us):
        super().__init__(ev)
        self.stream = EventStream(model, window_us=window_us)

    def step(self, t_prev, t_now):
        xy, t, p = self.cut(t_prev, t_now)
        return self.stream.step(xy, t, p, t_now=t_now)


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


def precompute_survivors(model, ev, window_us, step_us, t_end):
    """The survivors of the whole stream, through leg a's own code, as one host stream for leg c."""
    a = HostRoute(model, ev, window_us)
    parts = []
    for t_prev in range(T0, t_end, step_us):
        parts.append(a.survivors(t_prev, t_prev + step_us))
    return (torch.cat([q[0] for q in parts]).cpu().numpy(), torch.cat([q[1] for q in parts]).cpu().numpy(),
            torch.cat([q[2] for q in parts]).cpu().numpy())


def measure(model, raw_per_step, step_us, window_us, block, repeats):
    warm = 8
    t_end = T0 + window_us + (warm + repeats * block) * step_us
    ev = make_raw_stream(raw_per_step, step_us, t_end - T0 + step_us)
    with torch.no_grad():
        sv = precompute_survivors(model, ev, window_us, step_us, t_end)
        legs = {"a": HostRoute(model, ev, window_us), "b": FrontRoute(model, ev, window_us), "c": Floor(model, sv, window_us)}
        t = T0 + window_us
        for leg in legs.values():                          # the first window step by step, then warmed until captured
            run_block(leg, T0, step_us, window_us // step_us + warm)
        t += warm * step_us
        p50 = {k: [] for k in legs}
        order = ["a", "b", "c"]
        for r in range(repeats):
            for name in order[r % 3:] + order[:r % 3]:
                p50[name].append(float(np.median(run_block(legs[name], t, step_us, block))))
            t += block * step_us
        counts = {k: int(leg.stream.counts().sum()) for k, leg in legs.items()}
        for leg in legs.values():
            leg.stream.check_status()
    assert counts["a"] == counts["b"] == counts["c"], counts          # the three legs hold the same window
    n_raw = int(np.searchsorted(ev[1], t_end) - np.searchsorted(ev[1], T0 + window_us))
    n_sv = int(np.searchsorted(sv[1], t_end) - np.searchsorted(sv[1], T0 + window_us))
    steps = warm + repeats * block
    return dict(resident=counts["b"], raw_per_step=n_raw / steps, survivors_per_step=n_sv / steps,
                **{k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in p50.items()})


def trace(model, raw_per_step, step_us, window_us, steps=12):
    ev = make_raw_stream(raw_per_step, step_us, window_us + (steps + 1) * step_us)
    with torch.no_grad():
        b = FrontRoute(model, ev, window_us)
        run_block(b, T0, step_us, window_us // step_us + steps)
    torch.cuda.synchronize()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--raw_per_step", type=int, default=20000)
    ap.add_argument("--step_us", type=int, default=1000)
    ap.add_argument("--window_us", type=int, default=50000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    args = model_args("dagr-s", batch_size=1)
    model = randomize_(DAGR(args, height=H, width=W), seed=0).eval().cuda()
    model.cache_luts(width=W, height=H, radius=args.radius)
    model.check_device_status = False                     # no status read-back inside the timed call
    if a.trace:
        trace(model, a.raw_per_step, a.step_us, a.window_us)
        return
    r = measure(model, a.raw_per_step, a.step_us, a.window_us, a.block, a.repeats)
    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"                                    # noqa: E731
    lines = ["# Raw sensor events into the stream: the front on the device against `downsample_events` per push", "",
             f"`python tools/stream_downsample_probe.py --commit {a.commit} --out profiles/stream_downsample.md` on "
             f"{torch.cuda.get_device_name(0)}, commit {a.commit}: B = 1, a {W_IN}x{H_IN} sensor over the {W}x{H} model, "
             f"dagr-s events-only, random weights, {a.step_us} us steps on a {a.window_us} us window, "
             f"{r['raw_per_step']:.0f} raw events and {r['survivors_per_step']:.0f} survivors per step, "
             f"{r['resident']} resident events at the end.  Host clock around the call that ends in the detections' "
             f"read-back, host arrays in; the legs in one process, warmed until captured, alternating blocks of {a.block} "
             f"steps over the same stretch of the stream, {a.repeats} blocks each ({a.block * a.repeats} timed steps per "
             "leg).  ms per step: median of the blocks' p50 (min .. max of the blocks' p50).", "",
             "| leg | what runs | ms per step |", "|---|---|---|",
             f"| a | `downsample_events` per push, row cut, `step` on the survivors | {cell(r['a'])} |",
             f"| b | `EventStream(downsample=2).step` on the raw push | {cell(r['b'])} |",
             f"| c | `step` fed survivors computed beforehand (the floor) | {cell(r['c'])} |", "",
             f"b / a = {r['b'][0] / r['a'][0]:.2f}; the front's own cost b - c = {r['b'][0] - r['c'][0]:.3f} ms per step "
             f"(a - c = {r['a'][0] - r['c'][0]:.3f} ms)."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
