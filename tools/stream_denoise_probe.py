#!/usr/bin/env python
"""tools/stream_denoise_probe.py -- what the event stream's noise filter costs, and what it buys under a cap.

Cost: milliseconds per step of ``EventStream(downsample=2)`` fed RAW sensor events, without and with
``denoise_us`` / ``refractory_us``.  B = 1, a 1280x960 sensor over a 640x480 model (dagr-s, events only, random weights),
1 ms steps on a 50 ms window, at raw rates that leave about 25 k and 100 k resident events in the unfiltered window.  The raw
stream is built as tools/stream_downsample_probe.py builds its own: a model-resolution S-edges stream, every event repeated
3 to 6 times at ``(2x + {0,1}, 2y + {0,1}, t + {0,1,2})``.  Both legs take host arrays (the upload is part of a step), run
in this one process on the same model, are warmed until the window is captured and then run in alternating blocks of
``--block`` steps over the same stretch of the stream; the clock is the host's around the call that ends in the
detections' read-back.

Under a cap: a 320x215 stream without downsampling, 1 % of the pixels hot (one event every 500 us each) among S-edges
events, ``max_lane_events = 20000`` on a 50 ms window; the share of the capped window the hot pixels hold, without the
filter and with ``refractory_us = 1000``, from ``StreamDefinition`` -- whose counts the device stream is held to here.

    python tools/stream_denoise_probe.py --commit <hash> --out profiles/stream_denoise.md

The filter's launches by name come from ``rocprofv3 --kernel-trace --stats -- python tools/stream_denoise_probe.py --trace``
(the filtering leg at the larger rate and nothing else)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd.model.networks.dagr import DAGR                    # noqa: E402
from dagr_amd.streaming import EventStream, StreamDefinition     # noqa: E402
from dagr_amd.utils import synthetic as syn                      # noqa: E402
from dagr_amd.utils.args import model_args                       # noqa: E402
from dagr_amd.utils.testing_weights import randomize_            # noqa: E402

W, H, F = 640, 480, 2
W_IN, H_IN = F * W, F * H
T0 = 1 << 33
NOISE = dict(denoise_us=2000, refractory_us=1)
KEEP_ALL = dict(denoise_us=10 ** 9)      # removes next to nothing: the filter's launches in front of an unchanged window


def make_raw_stream(raw_per_step, step_us, duration_us, width=W, height=H, seed=5):
    n_base = int(raw_per_step / 4.5 * duration_us / step_us)
    x, y, t, p = syn.edges_window(n_base, width, height, seed, window_us=duration_us, time_window=duration_us)
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
    def __init__(self, model, ev, window_us, **noise):
        self.xy, self.t, self.p = ev
        self.stream = EventStream(model, window_us=window_us, downsample=F, sensor_size=(W_IN, H_IN), **noise)

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


def measure(model, raw_per_step, step_us, window_us, block, repeats):
    warm = 8
    t_end = T0 + window_us + (warm + repeats * block) * step_us
    ev = make_raw_stream(raw_per_step, step_us, t_end - T0 + step_us)
    with torch.no_grad():
        legs = {"off": Leg(model, ev, window_us), "on": Leg(model, ev, window_us, **NOISE),
                "all": Leg(model, ev, window_us, **KEEP_ALL)}
        for leg in legs.values():                          # the first window step by step, then warmed until captured
            run_block(leg, T0, step_us, window_us // step_us + warm)
        t = T0 + window_us + warm * step_us
        p50 = {k: [] for k in legs}
        order = ["off", "on", "all"]
        for r in range(repeats):
            for name in order[r % 3:] + order[:r % 3]:
                p50[name].append(float(np.median(run_block(legs[name], t, step_us, block))))
            t += block * step_us
        counts = {k: int(leg.stream.counts().sum()) for k, leg in legs.items()}
        filtered = int(legs["on"].stream.filtered().sum())
        for leg in legs.values():
            leg.stream.check_status()
    n_raw = int(np.searchsorted(ev[1], t_end) - np.searchsorted(ev[1], T0))
    steps = window_us // step_us + warm + repeats * block
    return dict(resident=counts, raw_per_step=n_raw / steps, filtered_share=filtered / max(1, n_raw),
                **{k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in p50.items()})


def trace(model, raw_per_step, step_us, window_us, steps=12):
    ev = make_raw_stream(raw_per_step, step_us, window_us + (steps + 1) * step_us)
    with torch.no_grad():
        run_block(Leg(model, ev, window_us, **NOISE), T0, step_us, window_us // step_us + steps)
    torch.cuda.synchronize()


def hot_pixels(model_small, steps=30, step_us=1000, window_us=50000, cap=20000, real_per_step=2000, period_us=500):
    """Share of the capped window that sits on hot pixels, without and with refractory_us = 1000 (the definition's window;
    the device stream's counts, dropped and filtered are held to the definition's)."""
    w, h = 320, 215
    xy, t, p = make_raw_stream(real_per_step, step_us, steps * step_us, width=w // 2, height=h // 2, seed=9)
    rng = np.random.Generator(np.random.PCG64(77))
    hot = rng.choice(w * h, (w * h) // 100, replace=False)
    phase = rng.integers(0, period_us, len(hot))
    ht = (T0 + phase[:, None] + period_us * np.arange(steps * step_us // period_us)[None, :]).reshape(-1)
    hx, hy = np.repeat(hot % w, steps * step_us // period_us), np.repeat(hot // w, steps * step_us // period_us)
    is_hot_map = np.zeros((h, w), bool)
    is_hot_map[hot // w, hot % w] = True
    x, y = np.concatenate([xy[:, 0], hx]), np.concatenate([xy[:, 1], hy])
    t, p = np.concatenate([t, ht]), np.concatenate([p, np.ones(len(ht), np.int8)])
    o = np.argsort(t, kind="stable")
    x, y, t, p = x[o].astype(np.int16), y[o].astype(np.int16), t[o], p[o]
    out = {}
    for name, noise in (("off", dict()), ("on", dict(refractory_us=1000))):
        d = StreamDefinition(1, w, h, window_us=window_us, max_lane_events=cap, **noise)
        stream = EventStream(model_small, window_us=window_us, max_lane_events=cap, **noise)
        with torch.no_grad():
            for k in range(steps):
                i0, i1 = np.searchsorted(t, [T0 + k * step_us, T0 + (k + 1) * step_us], side="left")
                d.push(x[i0:i1], y[i0:i1], t[i0:i1], p[i0:i1], t_now=T0 + (k + 1) * step_us)
                stream.step(np.stack([x[i0:i1], y[i0:i1]], -1), t[i0:i1], p[i0:i1], t_now=T0 + (k + 1) * step_us)
        assert stream.counts().tolist() == d.counts().tolist()
        assert np.array_equal(stream.dropped(), d.dropped) and np.array_equal(stream.filtered(), d.filtered)
        wx, wy = d.window()[:2]
        out[name] = dict(window=int(d.counts()[0]), hot=int(is_hot_map[wy, wx].sum()), dropped=int(d.dropped[0]),
                         filtered=int(d.filtered[0]))
    out["pushed"] = dict(total=len(t), hot=len(ht), pixels=len(hot))
    return out


def build(width, height):
    args = model_args("dagr-s", batch_size=1)
    model = randomize_(DAGR(args, height=height, width=width), seed=0).eval().cuda()
    model.cache_luts(width=width, height=height, radius=args.radius)
    model.check_device_status = False                     # no status read-back inside the timed call
    return model


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--raw_per_step", type=int, nargs="+", default=[3100, 13000])
    ap.add_argument("--step_us", type=int, default=1000)
    ap.add_argument("--window_us", type=int, default=50000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    model = build(W, H)
    if a.trace:
        trace(model, a.raw_per_step[-1], a.step_us, a.window_us)
        return
    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"                                    # noqa: E731
    lines = ["# The event stream's noise filter: what a step costs with it, and what it buys under a cap", "",
             f"`python tools/stream_denoise_probe.py --commit {a.commit} --out profiles/stream_denoise.md` on "
             f"{torch.cuda.get_device_name(0)}, commit {a.commit}: B = 1, a {W_IN}x{H_IN} sensor, `downsample=2` over the "
             f"{W}x{H} model, dagr-s events-only, random weights, {a.step_us} us steps on a {a.window_us} us window; the "
             f"filter is `denoise_us={NOISE['denoise_us']}, refractory_us={NOISE['refractory_us']}`.  Host clock around the "
             "call that ends in the detections' read-back, host arrays in; the legs in one process on the same stream, "
             f"warmed until captured, alternating blocks of {a.block} steps, {a.repeats} blocks each.  ms per step: median "
             "of the blocks' p50 (min .. max of the blocks' p50).", "",
             f"A third leg runs the filter with `denoise_us={KEEP_ALL['denoise_us']}` alone, which removes next to nothing: its "
             "window is the unfiltered one, so `all - off` is what the filter's launches add to a step (its deciding launch is "
             "then at its cheapest: a carried stamp that supports ends the search).", "",
             "| raw events per step | resident: off / on / all | removed by the filter (on) | off: ms per step "
             "| on: ms per step | all: ms per step | on - off | all - off |", "|---|---|---|---|---|---|---|---|"]
    for rate in a.raw_per_step:
        r = measure(model, rate, a.step_us, a.window_us, a.block, a.repeats)
        res = r["resident"]
        lines.append(f"| {r['raw_per_step']:.0f} | {res['off']} / {res['on']} / {res['all']} | "
                     f"{100 * r['filtered_share']:.1f} % | {cell(r['off'])} | {cell(r['on'])} | {cell(r['all'])} | "
                     f"{r['on'][0] - r['off'][0]:+.3f} | {r['all'][0] - r['off'][0]:+.3f} |")
    del model
    h = hot_pixels(build(320, 215))
    lines += ["", "## A 1 % hot-pixel population under a cap", "",
              f"320x215, no downsampling, {h['pushed']['pixels']} hot pixels firing every 500 us ({h['pushed']['hot']} of the "
              f"{h['pushed']['total']} events pushed in 30 steps of 1 ms), `max_lane_events=20000` on a 50 ms window.", "",
              "| | events in the window | of them on hot pixels | share | dropped by the cap | removed by the filter |",
              "|---|---|---|---|---|---|"]
    for name, label in (("off", "no filter"), ("on", "`refractory_us=1000`")):
        v = h[name]
        lines.append(f"| {label} | {v['window']} | {v['hot']} | {100 * v['hot'] / max(1, v['window']):.1f} % | {v['dropped']} | "
                     f"{v['filtered']} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
