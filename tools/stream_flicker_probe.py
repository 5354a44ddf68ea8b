#!/usr/bin/env python
"""tools/stream_flicker_probe.py -- what the event stream's anti-flicker and trail filters cost, what they buy under a
cap, and what the worst case of the walk costs.

Scene: B = 1, a 640x480 sensor and model (dagr-s, events only, random weights, no downsampling), 1 ms steps on a 50 ms
window; S-edges events plus pixels lit at 100 Hz from ``dagr_amd.utils.synthetic.flicker_events`` (one ON and one OFF
event per period each).  2 % of the pixels lit emit 61 k events per window by themselves, so the leg with about 25 k
resident events lights 0.5 % of the pixels and the leg with about 100 k lights 2 %.

(a) ms per step of ``EventStream(flicker=True, trail_us=1000)`` against the same stream without the options -- which makes
the library calls of the parent commit's step, tests/test_stream_flicker_gpu.py holds it to that.  (c) the same pair under
``max_lane_events``, with the resident events and the share of the window that sits on lit pixels.  All legs take host
arrays (the upload is part of a step), run in this one process on the same model, are warmed until the window is captured
and the lights are blocked, and then run in alternating blocks of ``--block`` steps over the same stretch of the stream;
the clock is the host's around the call that ends in the detections' read-back.

(d) one push of ``--run`` events on ONE pixel through ``dagr_stream_flicker``, against a push of as many events on pixels of
their own and against ``dagr_stream_denoise`` on both: device events around the call, the median of ``--calls`` calls.

    python tools/stream_flicker_probe.py

``--only_off`` runs the two legs without the options alone: copied into ``tools/`` of a checkout of the parent commit, that
is the parent's ``step`` on the same pushes.

(b) the launches by name come from ``rocprofv3 --kernel-trace --stats -- python tools/stream_flicker_probe.py --trace``:
``dagr_stream_flicker`` and ``dagr_stream_denoise`` called through the binding on the same pushes, the steps of the larger
scene, and nothing else."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd import _lib                                        # noqa: E402
from dagr_amd.model.networks.dagr import DAGR                    # noqa: E402
from dagr_amd.streaming import EventStream                       # noqa: E402
from dagr_amd.utils import synthetic as syn                      # noqa: E402
from dagr_amd.utils.args import model_args                       # noqa: E402
from dagr_amd.utils.testing_weights import randomize_            # noqa: E402

W, H = 640, 480
T0 = 1 << 33
FILTER = dict(flicker=True, trail_us=1000)
RULE = (2000, 20000, 4, 1, 7, 1000)          # the defaults' periods and thresholds, trail_us
SCENES = ((0.005, 10000), (0.02, 39000))     # (share of the pixels lit, S-edges events per 50 ms)


def make_scene(lit_share, edges_per_window, duration_us, seed=5):
    """``(xy, t, p, lit map)``: S-edges over the sensor plus ``lit_share`` of the pixels lit at 100 Hz."""
    n = int(edges_per_window * duration_us / 50000)
    x, y, t, p = syn.edges_window(n, W, H, seed, window_us=duration_us, time_window=duration_us)
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    flat = rng.choice(W * H, int(lit_share * W * H), replace=False)
    fx, fy, ft, fp = syn.flicker_events(np.stack([flat % W, flat // W], -1), 100, duration_us, seed, events_per_half=1)
    x, y, t, p = (np.concatenate([np.asarray(u, np.int64), v]) for u, v in zip((x, y, t, p), (fx, fy, ft, fp)))
    o = np.argsort(t, kind="stable")
    lit = np.zeros((H, W), bool)
    lit[flat // W, flat % W] = True
    return np.stack([x[o], y[o]], -1).astype(np.int16), t[o] + T0, p[o].astype(np.int8), lit


class Leg:
    def __init__(self, model, ev, window_us, **kw):
        self.xy, self.t, self.p = ev
        self.stream = EventStream(model, window_us=window_us, **kw)

    def step(self, t_prev, t_now):
        i0, i1 = np.searchsorted(self.t, [t_prev, t_now], side="left")
        return self.stream.step(self.xy[i0:i1], self.t[i0:i1], self.p[i0:i1], t_now=t_now)


def run_block(leg, t_start, step_us, steps):
    out = np.empty(steps)
    t_prev = t_start
    for k in range(steps):
        t_now = t_prev + step_us
        c0 = time.perf_counter()
        leg.step(t_prev, t_now)
        out[k] = time.perf_counter() - c0
        t_prev = t_now
    return out * 1e3


def measure(model, scene, step_us, window_us, block, repeats, cap, only_off=False):
    warm = 60                                             # the window fills, the graph is captured, the lights are blocked
    t_end = T0 + window_us + (warm + repeats * block) * step_us
    xy, t, p, lit = make_scene(*scene, t_end - T0 + step_us)
    ev = (xy, t, p)
    with torch.no_grad():
        legs = {"off": Leg(model, ev, window_us), "cap-off": Leg(model, ev, window_us, max_lane_events=cap)}
        if not only_off:
            legs.update({"on": Leg(model, ev, window_us, **FILTER),
                         "cap-on": Leg(model, ev, window_us, max_lane_events=cap, **FILTER)})
        for leg in legs.values():
            run_block(leg, T0, step_us, window_us // step_us + warm)
        now = T0 + window_us + warm * step_us
        p50 = {k: [] for k in legs}
        order = list(legs)
        for r in range(repeats):
            for name in order[r % len(order):] + order[:r % len(order)]:
                p50[name].append(float(np.median(run_block(legs[name], now, step_us, block))))
            now += block * step_us
        out = {}
        for name, leg in legs.items():
            s = leg.stream
            flicker, trail = (int(v.sum()) for v in s.suppressed()) if hasattr(s, "suppressed") else (0, 0)
            out[name] = dict(ms=(float(np.median(p50[name])), float(min(p50[name])), float(max(p50[name]))),
                             resident=int(s.counts().sum()), dropped=int(s.dropped().sum()), flicker=flicker, trail=trail)
            s.check_status()
    i0, i1 = np.searchsorted(t, [now - window_us, now])
    out["pushed_per_step"] = (i1 - i0) / (window_us / step_us)
    out["lit_share_of_window"] = float(lit[xy[i0:i1, 1], xy[i0:i1, 0]].mean())
    return out


class Entry:
    """``dagr_stream_flicker`` and ``dagr_stream_denoise`` through the binding, on states of their own."""

    def __init__(self, max_push):
        self.L, self.dev, self.max_push = _lib.lib(), torch.device("cuda:0"), max_push
        self.state = {}
        for name in ("flicker", "denoise"):
            nbytes = getattr(self.L, f"dagr_stream_{name}_bytes")(1, W, H, max_push)
            self.state[name] = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            _lib.check(getattr(self.L, f"dagr_stream_{name}_reset")(_lib.ptr(self.state[name]), nbytes, 1, W, H, max_push,
                                                                  _lib.cur_stream(self.dev)), name)
        self.out = (torch.empty((max_push, 2), dtype=torch.int16, device=self.dev),
                    torch.empty((max_push,), dtype=torch.int64, device=self.dev),
                    torch.empty((max_push,), dtype=torch.int8, device=self.dev),
                    torch.empty((max_push,), dtype=torch.int32, device=self.dev), torch.zeros((1,), dtype=torch.int32, device=self.dev))
        self.count = torch.zeros((2, 1), dtype=torch.int64, device=self.dev)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.dev)

    def call(self, name, xy, t, p, batch):
        P, st = _lib.ptr, self.state[name]
        rule = RULE if name == "flicker" else (2000, 1)
        counters = (P(self.count[0]), P(self.count[1])) if name == "flicker" else (P(self.count[0]),)
        _lib.check(getattr(self.L, f"dagr_stream_{name}")(P(st), st.numel(), 1, self.max_push, W, H, *rule, P(xy), P(t), P(p),
                                                         P(batch), 0, int(t.shape[0]), *(P(o) for o in self.out), *counters,
                                                         P(self.status), _lib.cur_stream(self.dev)), name)


def on_device(xy, t, p):
    d = torch.device("cuda:0")
    return (torch.from_numpy(np.ascontiguousarray(xy)).to(d), torch.from_numpy(np.ascontiguousarray(t)).to(d),
            torch.from_numpy(np.ascontiguousarray(p)).to(d), torch.zeros((len(t),), dtype=torch.int32, device=d))


def worst_case(run, calls):
    """Milliseconds per call (median, min, max) of either filter on a push of ``run`` events on one pixel / on pixels of
    their own."""
    rng = np.random.Generator(np.random.PCG64(3))
    t = T0 + np.cumsum(rng.integers(1, 40, run)).astype(np.int64)
    p = rng.choice(np.array([-1, 1], np.int8), run)
    flat = rng.choice(W * H, run, replace=False)
    pushes = {"one pixel": on_device(np.full((run, 2), 100, np.int16), t, p),
              "pixels of their own": on_device(np.stack([flat % W, flat // W], -1).astype(np.int16), t, p)}
    e = Entry(run)
    out = {}
    for label, push in pushes.items():
        for name in ("flicker", "denoise"):
            ms = []
            for k in range(calls + 5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                e.call(name, *push)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            ms = ms[5:]
            out[(label, name)] = (float(np.median(ms)), float(min(ms)), float(max(ms)))
    return out


def trace(step_us, window_us, steps=40):
    """Both entries on the steps of the larger scene, from its 60th millisecond on (the lights are blocked by then)."""
    xy, t, p, _ = make_scene(*SCENES[-1], (60 + steps + 1) * step_us)
    e = Entry(1 << 15)
    for k in range(60 + steps):
        i0, i1 = np.searchsorted(t, [T0 + k * step_us, T0 + (k + 1) * step_us])
        push = on_device(xy[i0:i1], t[i0:i1], p[i0:i1])
        e.call("flicker", *push)
        if k >= 60:
            e.call("denoise", *push)
    torch.cuda.synchronize()
    print(f"traced {steps} pushes of about {i1 - i0} events; suppressed {e.count.cpu().numpy().ravel().tolist()}")


def build(width, height):
    args = model_args("dagr-s", batch_size=1)
    model = randomize_(DAGR(args, height=height, width=width), seed=0).eval().cuda()
    model.cache_luts(width=width, height=height, radius=args.radius)
    model.check_device_status = False                     # no status read-back inside the timed call
    return model


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step_us", type=int, default=1000)
    ap.add_argument("--window_us", type=int, default=50000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--cap", type=int, default=20000)
    ap.add_argument("--run", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--only_off", action="store_true", help="the legs without the options only: what a checkout of the "
                    "parent commit, with this file copied into its tools/, can run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    if a.trace:
        trace(a.step_us, a.window_us)
        return
    model = build(W, H)
    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"                                    # noqa: E731
    lines = [f"`python tools/stream_flicker_probe.py` on {torch.cuda.get_device_name(0)}: B = 1, {W}x{H}, dagr-s events-only, "
             f"random weights, {a.step_us} us steps on a {a.window_us} us window, `flicker=True, trail_us=1000`; "
             f"alternating blocks of {a.block} steps, {a.repeats} blocks per leg.  ms per step: median of the blocks' p50 "
             "(min .. max of the blocks' p50).", "",
             "| pixels lit | events per step | of the window on lit pixels | leg | resident | removed: flicker / trail "
             "| dropped by the cap | ms per step |", "|---|---|---|---|---|---|---|---|"]
    for scene in SCENES:
        r = measure(model, scene, a.step_us, a.window_us, a.block, a.repeats, a.cap, a.only_off)
        for name in ("off", "on", "cap-off", "cap-on"):
            if name not in r:
                continue
            v = r[name]
            lines.append(f"| {100 * scene[0]:.1f} % | {r['pushed_per_step']:.0f} | {100 * r['lit_share_of_window']:.1f} % | {name} | "
                         f"{v['resident']} | {v['flicker']} / {v['trail']} | {v['dropped']} | {cell(v['ms'])} |")
    if a.only_off:
        print("\n".join(lines))
        return
    w = worst_case(a.run, a.calls)
    lines += ["", f"One push of {a.run} events, ms per call by device events, median (min .. max) of {a.calls} calls:", "",
              "| push | `dagr_stream_flicker` | `dagr_stream_denoise` |", "|---|---|---|"]
    for label in ("one pixel", "pixels of their own"):
        lines.append(f"| {a.run} events on {label} | {cell(w[(label, 'flicker')])} | {cell(w[(label, 'denoise')])} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
