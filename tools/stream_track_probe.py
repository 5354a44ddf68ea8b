#!/usr/bin/env python
"""tools/stream_track_probe.py -- what the event stream's tracker (``EventStream(track=)``) adds to a step.

Milliseconds per ``EventStream.step_device`` without and with ``track=``: B = 1, a 640x480 model (dagr-s, events only, random
weights), 1 ms steps on a 50 ms window at a rate that leaves about 25 k resident events.  The legs take device-resident
events, run in this one process on the same model and the same stream of events, are warmed until the window is captured
and then run in alternating blocks of ``--block`` steps; the clock is the host's around ``step_device`` plus the device
synchronisation that ends it.  Two tracking legs: ``track=True`` on everything the model detects (with random weights every
anchor survives the confidence threshold, so the first ``DAGR_TRACK_MAX_DETS`` rows take part against 64 slots -- the
tracker's worst case), and ``min_score`` set to the step's 50th score, which leaves about 50 boxes to track.

The launch's own duration: ``dagr_stream_track`` issued ``--launches`` times back to back on the last step's detections
between two device events, per launch.  Back-to-back launches of one small kernel are bounded below by the launch rate, so
this is the larger of the kernel's duration and one launch interval.

    python tools/stream_track_probe.py --commit <hash> --out profiles/stream_track.md

``--out`` replaces the measured section of the file (between its two marker comments) and leaves the rest, which is written
by hand.  The kernel's own duration comes from a kernel trace of a run of its own,
``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/stream_track_probe.py --trace all`` (or ``--trace 50``): that
tracking leg alone, nothing timed by the host."""
import argparse
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


class Leg:
    def __init__(self, model, ev, window_us, **kw):
        self.xy, self.t, self.p = ev
        self.t_host = self.t.cpu().numpy()
        self.stream = EventStream(model, window_us=window_us, **kw)

    def step(self, t_prev, t_now):
        i0, i1 = np.searchsorted(self.t_host, [t_prev, t_now], side="left")
        now = torch.full((1,), int(t_now), dtype=torch.int64, device=self.t.device)       # (on the device: no host path)
        return self.stream.step_device(self.xy[i0:i1], self.t[i0:i1], self.p[i0:i1], t_now=now)


def run_block(leg, t_start, step_us, steps):
    out = np.empty(steps)
    t_prev = t_start
    for k in range(steps):
        t_now = t_prev + step_us
        c0 = time.perf_counter()
        leg.step(t_prev, t_now)
        torch.cuda.synchronize()
        out[k] = time.perf_counter() - c0
        t_prev = t_now
    leg.stream.counts()         # (the host's bound on the window, which sizes the buffers, falls back to the count)
    return out * 1e3


def launch_alone(stream, det, n_keep, launches):
    """ms per dagr_stream_track launch, back to back on one step's detections (the state moves on: every call matches the
    same boxes again)."""
    st = stream.state
    for _ in range(10):
        st.run_track(det, n_keep)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        st.run_track(det, n_keep)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


BEGIN = "<!-- measured: written by tools/stream_track_probe.py --out, which replaces this section and nothing else -->"
END = "<!-- measured: end -->"


def write_section(path, text):
    """Put the measured section into ``path``: in place of the one it holds, or as a new file under a title.  Whatever else
    the file says -- the reading of the figures -- is written by hand and stays."""
    old = open(path).read() if os.path.exists(path) else ""
    if BEGIN in old and END in old:
        new = old[:old.index(BEGIN)] + text.rstrip("\n") + old[old.index(END) + len(END):]
    else:
        new = "# The event stream's tracker: what `track=` adds to a step\n\n" + text
    with open(path, "w") as f:
        f.write(new)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--per_step", type=int, default=500)
    ap.add_argument("--step_us", type=int, default=1000)
    ap.add_argument("--window_us", type=int, default=50000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", choices=["all", "50"], default=None, help="run that tracking leg alone for --trace_steps "
                    "steps behind a warmed window and nothing else: the run to put under a kernel trace")
    ap.add_argument("--trace_steps", type=int, default=200)
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    args = model_args("dagr-s", batch_size=1)
    model = randomize_(DAGR(args, height=H, width=W), seed=0).eval().cuda()
    model.cache_luts(width=W, height=H, radius=args.radius)
    model.check_device_status = False
    warm = 8
    n_steps = a.window_us // a.step_us + warm + a.repeats * a.block
    duration = (n_steps + 1) * a.step_us
    x, y, t, p = syn.edges_window(a.per_step * (n_steps + 1), W, H, 5, window_us=duration, time_window=duration)
    dev = torch.device("cuda:0")
    ev = (torch.from_numpy(np.stack([x, y], -1).astype(np.int16)).to(dev),
          torch.from_numpy(np.int64(T0) + t.astype(np.int64)).to(dev), torch.from_numpy(p.astype(np.int8)).to(dev))
    with torch.no_grad():
        # the 50th score of a settled window, for the leg that tracks about 50 boxes
        scout = Leg(model, ev, a.window_us)
        run_block(scout, T0, a.step_us, a.window_us // a.step_us)
        det, n_keep = scout.step(T0 + a.window_us, T0 + a.window_us + a.step_us)
        n_all, anchors = int(n_keep[0]), int(det.shape[1])
        scores = det[0, :n_all, 4].cpu().numpy()
        cut = float(scores[min(49, n_all - 1)]) if n_all else 0.0
        if a.trace:
            leg = Leg(model, ev, a.window_us, track=True if a.trace == "all" else dict(min_score=cut))
            run_block(leg, T0, a.step_us, a.window_us // a.step_us + warm + a.trace_steps)
            leg.stream.check_status()
            return
        legs = {"off": Leg(model, ev, a.window_us), "all": Leg(model, ev, a.window_us, track=True),
                "50": Leg(model, ev, a.window_us, track=dict(min_score=cut))}
        for leg in legs.values():
            run_block(leg, T0, a.step_us, a.window_us // a.step_us + warm)
        t_at = T0 + a.window_us + warm * a.step_us
        p50 = {k: [] for k in legs}
        order = list(legs)
        for r in range(a.repeats):
            for name in order[r % 3:] + order[:r % 3]:
                p50[name].append(float(np.median(run_block(legs[name], t_at, a.step_us, a.block))))
            t_at += a.block * a.step_us
        rows, alone = {}, {}
        for name in ("all", "50"):
            s = legs[name].stream
            det, n_keep = legs[name].step(t_at, t_at + a.step_us)
            det, n_keep = det.clone(), n_keep.clone()
            torch.cuda.synchronize()
            eligible = int((det[0, :int(n_keep[0]), 4] >= s.track["min_score"]).sum())
            rows[name] = (int(n_keep[0]), eligible, int((s.track_ids[0, :int(n_keep[0])] != 0).sum()), len(s.tracks()[0]))
            alone[name] = launch_alone(s, det, n_keep, a.launches)
        resident = {k: int(leg.stream.counts().sum()) for k, leg in legs.items()}
        for leg in legs.values():
            leg.stream.check_status()
    stat = {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in p50.items()}
    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"                                    # noqa: E731
    lines = [BEGIN, "",
             f"`python tools/stream_track_probe.py --commit {a.commit} --out profiles/stream_track.md`, commit {a.commit}: "
             f"B = 1, {W}x{H}, dagr-s events-only, random weights, "
             f"{a.step_us} us steps on a {a.window_us} us window, {a.per_step} events a step ({resident['off']} resident); "
             f"{anchors} anchors, of which {n_all} survive the confidence threshold.  Host clock around `step_device` and the "
             "device synchronisation behind it, device-resident events in; the legs in one process on the same events, warmed "
             f"until captured, alternating blocks of {a.block} steps, {a.repeats} blocks each ({a.block * a.repeats} timed "
             "steps per leg).  ms per step: median of the blocks' p50 (min .. max of the blocks' p50).  `dagr_stream_track` "
             f"alone: {a.launches} calls back to back between two device events, per call -- an upper bound of the kernel's "
             "duration that includes the host's call overhead.", "",
             "| leg | detections | eligible rows | rows with an id | live tracks | ms per step | minus `off` "
             "| `dagr_stream_track` alone, ms per call |", "|---|---|---|---|---|---|---|---|",
             f"| off (no `track=`) | {n_all} | | | | {cell(stat['off'])} | | |"]
    for name, label in (("all", "`track=True`"), ("50", f"`track=dict(min_score={cut:.6g})`")):
        r = rows[name]
        lines.append(f"| {label} | {r[0]} | {r[1]} | {r[2]} | {r[3]} | {cell(stat[name])} | "
                     f"{stat[name][0] - stat['off'][0]:+.4f} | {alone[name]:.4f} |")
    lines += ["", END]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        write_section(a.out, text)


if __name__ == "__main__":
    main()
