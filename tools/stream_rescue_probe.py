#!/usr/bin/env python
"""tools/stream_rescue_probe.py -- what the tracker's second association round (``EventStream(track=, rescue=)``) adds to a
step.

Milliseconds per ``EventStream.step_device`` without tracking, with ``track=``, with ``track=, motion=True`` and with each
of the two plus ``rescue=``, in the setting of ``tools/stream_motion_probe.py``: B = 1, a 640x480 model (dagr-s, events
only, random weights), 1 ms steps on a 50 ms window at a rate that leaves about 25 k resident events.  ``min_score`` is the
median score of a settled step, the same in every tracking leg, and ``low_score`` is 0, so that about half of the head's
rows are high and the other half low.  The legs take device-resident events, run in this one process on the same model and
the same stream of events, are warmed until the window is captured and then run in alternating blocks of ``--block`` steps;
the clock is the host's around ``step_device`` plus the device synchronisation that ends it.

The launches' own durations: the four entries, each on a state of its own that has been through the same steps, issued
``--launches`` times back to back on the SAME detections between two device events, in alternating rounds; per launch.  (The
state moves on with every call: from the second call on every row meets the track it matched in the call before.)

    python tools/stream_rescue_probe.py --commit <hash> --out profiles/stream_rescue.md

``--out`` replaces the measured section of the file (between its two marker comments) and leaves the rest, which is written
by hand."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd.model.networks.dagr import DAGR                    # noqa: E402
from dagr_amd.utils import synthetic as syn                      # noqa: E402
from dagr_amd.utils.args import model_args                       # noqa: E402
from dagr_amd.utils.testing_weights import randomize_            # noqa: E402
from tools.stream_motion_probe import launches                   # noqa: E402
from tools.stream_track_probe import H, T0, W, Leg, run_block    # noqa: E402

BEGIN = "<!-- measured: written by tools/stream_rescue_probe.py --out, which replaces this section and nothing else -->"
END = "<!-- measured: end -->"
LEGS = (("track", dict()), ("track + rescue", dict(rescue=dict(low_score=0.0))), ("motion", dict(motion=True)),
        ("motion + rescue", dict(motion=True, rescue=dict(low_score=0.0))))
ENTRY = {"track": "dagr_stream_track", "track + rescue": "dagr_stream_track_rescue", "motion": "dagr_stream_track_cv",
         "motion + rescue": "dagr_stream_track_cv_rescue"}


def write_section(path, text):
    """Put the measured section into ``path``: in place of the one it holds, or as a new file under a title."""
    old = open(path).read() if os.path.exists(path) else ""
    if BEGIN in old and END in old:
        new = old[:old.index(BEGIN)] + text.rstrip("\n") + old[old.index(END) + len(END):]
    else:
        new = "# The tracker's second association round: what `rescue=` adds to a step\n\n" + text
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
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
        scout = Leg(model, ev, a.window_us)                 # the median score of a settled window
        run_block(scout, T0, a.step_us, a.window_us // a.step_us)
        det, n_keep = scout.step(T0 + a.window_us, T0 + a.window_us + a.step_us)
        n_all, anchors = int(n_keep[0]), int(det.shape[1])
        cut = float(np.float32(np.median(det[0, :n_all, 4].cpu().numpy())))
        legs = {"off": Leg(model, ev, a.window_us)}
        for name, kw in LEGS:
            legs[name] = Leg(model, ev, a.window_us, track=dict(min_score=cut), **kw)
        for leg in legs.values():
            run_block(leg, T0, a.step_us, a.window_us // a.step_us + warm)
        t_at = T0 + a.window_us + warm * a.step_us
        p50 = {k: [] for k in legs}
        order = list(legs)
        for r in range(a.repeats):
            k = r % len(order)
            for name in order[k:] + order[:k]:
                p50[name].append(float(np.median(run_block(legs[name], t_at, a.step_us, a.block))))
            t_at += a.block * a.step_us
        # one more step of every leg: the rows of the rounds, then the launches alone on its detections
        before = {name: legs[name].stream.rescued().copy() for name, kw in LEGS if "rescue" in kw}
        det, n_keep = legs["track"].step(t_at, t_at + a.step_us)
        det, n_keep = det.clone(), n_keep.clone()
        for name, _ in LEGS[1:]:
            legs[name].step(t_at, t_at + a.step_us)
        torch.cuda.synchronize()
        n = int(n_keep[0])
        scores = det[0, :n, 4].cpu().numpy()
        high = int((scores >= np.float32(cut)).sum())
        low = int(((scores >= np.float32(0)) & ~(scores >= np.float32(cut))).sum())
        rows = {name: (int((legs[name].stream.track_ids[0, :n] != 0).sum()),
                       int((legs[name].stream.rescued() - before[name]).sum()) if name in before else 0) for name, _ in LEGS}
        for name, _ in LEGS:
            launches(legs[name].stream, det, n_keep, 10)
        per = {name: [] for name, _ in LEGS}
        for _ in range(a.rounds):
            for name, _kw in LEGS:
                per[name].append(launches(legs[name].stream, det, n_keep, a.launches))
        timed = {name: int((legs[name].stream.rescued() - before[name]).sum()) - rows[name][1] for name in before}
        # the same entries on the same detections with an EMPTY band (one fp32 value under min_score, which no row has):
        # what the instantiation costs before any low row is walked
        empty = {name: [] for name in before}
        under = float(np.nextafter(np.float32(cut), np.float32(-1)))
        for name in before:
            legs[name].stream.state.rescue["low_score"] = under
        for _ in range(a.rounds):
            for name in before:
                empty[name].append(launches(legs[name].stream, det, n_keep, a.launches))
        for name in before:
            legs[name].stream.state.rescue["low_score"] = 0.0
        resident = int(legs["off"].stream.counts().sum())
        for leg in legs.values():
            leg.stream.check_status()
    stat = {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in p50.items()}
    cell = lambda v, d=3: f"{v[0]:.{d}f} ({v[1]:.{d}f} .. {v[2]:.{d}f})"                           # noqa: E731
    lines = [BEGIN, "",
             f"`python tools/stream_rescue_probe.py --commit {a.commit} --out profiles/stream_rescue.md`, commit {a.commit}: "
             f"B = 1, {W}x{H}, dagr-s events-only, random weights, {a.step_us} us steps on a {a.window_us} us window, "
             f"{a.per_step} events a step ({resident} resident); {anchors} anchors, of which {n_all} survive the confidence "
             f"threshold.  `min_score = {cut:.6g}` (the median score of a settled step) in every tracking leg, `low_score = 0`: "
             f"in the step the rows are counted on, {high} rows are high and {low} low (each round takes 256 at most), 64 "
             "slots.  Host clock around `step_device` and the device synchronisation behind it, device-resident events in; the "
             f"legs in one process on the same events, warmed until captured, alternating blocks of {a.block} steps, "
             f"{a.repeats} blocks each ({a.block * a.repeats} timed steps per leg).  ms per step: median of the blocks' p50 "
             "(min .. max of the blocks' p50).", "",
             "| leg | ms per step | minus `off` | minus the leg without `rescue=` |", "|---|---|---|---|",
             f"| off (no `track=`) | {cell(stat['off'])} | | |"]
    for name, _ in LEGS:
        v = stat[name]
        base = stat[name.replace(" + rescue", "")][0] if "rescue" in name else None
        lines.append(f"| {name} | {cell(v)} | {v[0] - stat['off'][0]:+.4f} | {'' if base is None else f'{v[0] - base:+.4f}'} |")
    lines += ["", f"The launches alone, on the detections of that one step: {a.launches} calls back to back between two "
              f"device events, {a.rounds} rounds alternating between the four entries; ms per call, median (min .. max) of "
              "the rounds.  In these calls every track is matched again by the row that matched it in the call before.", "",
              "| entry | rows with an id in the step | of them rescued in the step | rescued per timed call | ms per call | "
              "minus the base entry | per low row, us | with an empty band, ms per call | minus the base entry | the low rows' "
              "share, per low row, us |", "|---|---|---|---|---|---|---|---|---|---|"]
    med = {name: float(np.median(v)) for name, v in per.items()}
    for name, _ in LEGS:
        v = (med[name], min(per[name]), max(per[name]))
        extra = ""
        if "rescue" in name:
            diff = med[name] - med[name.replace(" + rescue", "")]
            calls = a.rounds * a.launches + 10
            e = (float(np.median(empty[name])), min(empty[name]), max(empty[name]))
            extra = (f"{timed[name] / calls:.1f} | {cell(v, 4)} | {diff:+.4f} | {1e3 * diff / max(1, min(low, 256)):+.3f} | "
                     f"{cell(e, 4)} | {e[0] - med[name.replace(' + rescue', '')]:+.4f} | "
                     f"{1e3 * (med[name] - e[0]) / max(1, min(low, 256)):+.3f}")
        else:
            extra = f"| {cell(v, 4)} | | | | |"
        lines.append(f"| `{ENTRY[name]}` | {rows[name][0]} | {rows[name][1]} | {extra} |")
    lines += ["", END]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        write_section(a.out, text)


if __name__ == "__main__":
    main()
