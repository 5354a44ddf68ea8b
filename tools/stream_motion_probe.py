#!/usr/bin/env python
"""tools/stream_motion_probe.py -- what the tracker's motion model (``EventStream(track=, motion=)``) adds to a step.

Milliseconds per ``EventStream.step_device`` without tracking, with ``track=`` and with ``track=, motion=True``, in the setting
of ``tools/stream_track_probe.py``: B = 1, a 640x480 model (dagr-s, events only, random weights), 1 ms steps on a 50 ms
window at a rate that leaves about 25 k resident events.  With random weights every anchor survives the confidence
threshold, so the first ``DAGR_TRACK_MAX_DETS`` rows take part against 64 slots.  The legs take device-resident events,
run in this one process on the same model and the same stream of events, are warmed until the window is captured and then
run in alternating blocks of ``--block`` steps; the clock is the host's around ``step_device`` plus the device
synchronisation that ends it.  Two settings of ``min_score``: 0 (everything the model detects) and the step's 50th score.

The launches' own durations: ``dagr_stream_track`` and ``dagr_stream_track_cv``, each on a state of its own that has been
through the same warm-up steps, issued ``--launches`` times back to back on the SAME detections between two device events, in
alternating rounds; per launch.  The yardstick is the plain tracker's launch in the same run.  (The state moves on with
every call: from the second call on every row meets the track it made or matched in the call before, at ``dt = 0``.)

    python tools/stream_motion_probe.py --commit <hash> --out profiles/stream_motion.md

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
from tools.stream_track_probe import H, T0, W, Leg, run_block    # noqa: E402

BEGIN = "<!-- measured: written by tools/stream_motion_probe.py --out, which replaces this section and nothing else -->"
END = "<!-- measured: end -->"


def write_section(path, text):
    """Put the measured section into ``path``: in place of the one it holds, or as a new file under a title.  Whatever else
    the file says -- the reading of the figures -- is written by hand and stays."""
    old = open(path).read() if os.path.exists(path) else ""
    if BEGIN in old and END in old:
        new = old[:old.index(BEGIN)] + text.rstrip("\n") + old[old.index(END) + len(END):]
    else:
        new = "# The tracker's motion model: what `motion=` adds to a step\n\n" + text
    with open(path, "w") as f:
        f.write(new)


def launches(stream, det, n_keep, count):
    """ms per tracker launch of ``stream`` (plain or motion), ``count`` calls back to back on one step's detections."""
    st = stream.state
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(count):
        st.run_track(det, n_keep)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / count


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
        # the 50th score of a settled window, for the legs that track about 50 boxes
        scout = Leg(model, ev, a.window_us)
        run_block(scout, T0, a.step_us, a.window_us // a.step_us)
        det, n_keep = scout.step(T0 + a.window_us, T0 + a.window_us + a.step_us)
        n_all, anchors = int(n_keep[0]), int(det.shape[1])
        scores = det[0, :n_all, 4].cpu().numpy()
        cut = float(scores[min(49, n_all - 1)]) if n_all else 0.0
        legs = {"off": Leg(model, ev, a.window_us)}
        for name, score in (("all", 0.0), ("50", cut)):
            legs[f"track {name}"] = Leg(model, ev, a.window_us, track=dict(min_score=score))
            legs[f"motion {name}"] = Leg(model, ev, a.window_us, track=dict(min_score=score), motion=True)
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
        rows, alone = {}, {}
        for name in ("all", "50"):
            plain, moving = legs[f"track {name}"], legs[f"motion {name}"]
            det, n_keep = plain.step(t_at, t_at + a.step_us)
            det, n_keep = det.clone(), n_keep.clone()
            moving.step(t_at, t_at + a.step_us)
            torch.cuda.synchronize()
            n = int(n_keep[0])
            s, m = plain.stream, moving.stream
            eligible = int((det[0, :n, 4] >= s.track["min_score"]).sum())
            rows[name] = (n, eligible, int((s.track_ids[0, :n] != 0).sum()), int((m.track_ids[0, :n] != 0).sum()),
                          int((m.track_hits[0, :n] > 1).sum()), len(m.coasting()[0]))
            for stream in (s, m):                           # both states onto these detections, then alternating rounds
                launches(stream, det, n_keep, 10)
            per = {"track": [], "motion": []}
            for _ in range(a.rounds):
                per["track"].append(launches(s, det, n_keep, a.launches))
                per["motion"].append(launches(m, det, n_keep, a.launches))
            matched = int((m.track_hits[0, :n] > 1).sum())      # rows that match in the timed calls
            alone[name] = (per, matched)
        resident = {k: int(leg.stream.counts().sum()) for k, leg in legs.items()}
        for leg in legs.values():
            leg.stream.check_status()
    stat = {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in p50.items()}
    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"                                    # noqa: E731
    lines = [BEGIN, "",
             f"`python tools/stream_motion_probe.py --commit {a.commit} --out profiles/stream_motion.md`, commit {a.commit}: "
             f"B = 1, {W}x{H}, dagr-s events-only, random weights, "
             f"{a.step_us} us steps on a {a.window_us} us window, {a.per_step} events a step ({resident['off']} resident); "
             f"{anchors} anchors, of which {n_all} survive the confidence threshold.  Host clock around `step_device` and the "
             "device synchronisation behind it, device-resident events in; the legs in one process on the same events, warmed "
             f"until captured, alternating blocks of {a.block} steps, {a.repeats} blocks each ({a.block * a.repeats} timed "
             "steps per leg).  ms per step: median of the blocks' p50 (min .. max of the blocks' p50).", "",
             "| leg | ms per step | minus `off` | minus the `track=` leg |", "|---|---|---|---|",
             f"| off (no `track=`) | {cell(stat['off'])} | | |"]
    for name, label in (("all", "min_score=0"), ("50", f"min_score={cut:.6g}")):
        tr, mo = stat[f"track {name}"], stat[f"motion {name}"]
        lines.append(f"| `track=dict({label})` | {cell(tr)} | {tr[0] - stat['off'][0]:+.4f} | |")
        lines.append(f"| `track=dict({label}), motion=True` | {cell(mo)} | {mo[0] - stat['off'][0]:+.4f} | {mo[0] - tr[0]:+.4f} |")
    lines += ["", f"The launches alone, on the detections of one step: {a.launches} calls back to back between two device "
              f"events, {a.rounds} rounds alternating between the two entries; ms per call, median (min .. max) of the "
              "rounds.  In these calls every row that gets an id matches the track of the call before at `dt = 0`.", "",
              "| detections | eligible rows | rows with an id (`track=` / `motion=` step) | matched rows in the step / in the "
              "timed calls | coasting after the step | `dagr_stream_track` | `dagr_stream_track_cv` | difference | per "
              "eligible row, us | per matched row, us |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name in ("all", "50"):
        r, (per, matched) = rows[name], alone[name]
        tr = (float(np.median(per["track"])), min(per["track"]), max(per["track"]))
        mo = (float(np.median(per["motion"])), min(per["motion"]), max(per["motion"]))
        diff = mo[0] - tr[0]
        lines.append(f"| {r[0]} | {r[1]} | {r[2]} / {r[3]} | {r[4]} / {matched} | {r[5]} | {tr[0]:.4f} ({tr[1]:.4f} .. {tr[2]:.4f}) "
                     f"| {mo[0]:.4f} ({mo[1]:.4f} .. {mo[2]:.4f}) | {diff:+.4f} | {1e3 * diff / max(1, r[1]):+.3f} "
                     f"| {1e3 * diff / max(1, matched):+.3f} |")
    lines += ["", END]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        write_section(a.out, text)


if __name__ == "__main__":
    main()
