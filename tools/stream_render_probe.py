#!/usr/bin/env python
"""tools/stream_render_probe.py -- what the stream's picture (``EventStream(render=)``, ``render_step()``) costs, beside the
host path it replaces, and what its trail launch adds to a step.

``--part render``: a 640x480 model (dagr-s, events only, random weights), B = 1 and B = 8.  One step leaves 25 k or 100 k
resident events in the stream (spread over the lanes); the step's rows, ids and rings are then replaced by synthetic ones --
8 or 64 boxes a lane with ids, 0 or 64 live trails of 32 points a lane -- so that the picture's load is the stated one.
The new path: ``render_step()`` issued ``--launches`` times back to back between two device events, per call.  The host
path of the parent commit, in the same process right after it: ``counts()`` (the synchronisation), the read-back of the
window's events (t, xy, p: 13 bytes an event), of ``det``, ``n_keep`` and the ids, and ``render_frames`` on them with the
boxes as integer rows; the clock is the host's, and the path ends in ``render_frames``' own status read-back.  It draws no
ids and no trails: a lower bound of the host path.  ``--rounds`` rounds of each, alternating; median (min .. max).

``--part step``: milliseconds per ``step_device`` of a B = 1 tracking stream without and with ``render=`` (no
``render_step``), in the setting of ``tools/stream_track_probe.py``: alternating blocks of ``--block`` steps in one process.

``--part kernels --config K``: ``render_step()`` alone, 200 calls in configuration K of ``--part render`` (its order), for
``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/stream_render_probe.py --part kernels --config K``.

Each part is one process, run under a time limit of its own.  ``--out`` replaces the part's measured section of the file
(between its two marker comments) and leaves the rest, which is written by hand."""
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
from dagr_amd.visualization.frames import render_frames          # noqa: E402
from tools.stream_assign_probe import write_section              # noqa: E402
from tools.stream_track_probe import H, T0, W, Leg, run_block    # noqa: E402

WINDOW_US = 50000
CONFIGS = [(B, n, boxes, trails) for B in (1, 8) for n in (25000, 100000) for boxes, trails in ((8, 0), (64, 64))]
TRACK = dict(max_tracks=64)


def markers(part):
    return (f"<!-- measured ({part}): written by tools/stream_render_probe.py --part {part} --out, which replaces this section "
            "and nothing else -->", f"<!-- measured ({part}): end -->")


def model_for(B):
    torch.manual_seed(0)
    args = model_args("dagr-s", batch_size=B)
    model = randomize_(DAGR(args, height=H, width=W), seed=0).eval().cuda()
    model.cache_luts(width=W, height=H, radius=args.radius)
    model.check_device_status = False
    return model


def loaded_stream(model, B, n_events, boxes, trails, seed=3):
    """A drawing stream after one step that left ``n_events`` resident events, its rows / ids / rings replaced by the
    stated load; returns it with the pushed events (device tensors: what a host path reads back)."""
    dev = torch.device("cuda:0")
    rng = np.random.Generator(np.random.PCG64(seed))
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK, render=dict(trail=32, event_window_us=None))
    per = n_events // B
    parts = [syn.edges_window(per, W, H, seed + b, window_us=WINDOW_US - 1, time_window=WINDOW_US - 1) for b in range(B)]
    xy = np.concatenate([np.stack([p[0], p[1]], -1) for p in parts]).astype(np.int16)
    t = np.concatenate([np.int64(T0) + p[2].astype(np.int64) for p in parts])
    pol = np.concatenate([p[3] for p in parts]).astype(np.int8)
    batch = np.repeat(np.arange(B, dtype=np.int64), per)
    ev = tuple(torch.from_numpy(v).to(dev) for v in (xy, t, pol, batch))
    now = torch.full((B,), T0 + WINDOW_US - 1, dtype=torch.int64, device=dev)
    with torch.no_grad():
        det, n_keep = stream.step_device(*ev[:3], batch=ev[3], t_now=now)
    assert int(stream.counts().sum()) == per * B, "the window does not hold the stated events"
    st, A, M = stream.state, int(det.shape[1]), TRACK["max_tracks"]
    assert boxes <= A
    rows = np.zeros((B, A, 6), np.float32)
    xy0 = rng.uniform(0, [W - 80, H - 80], (B, boxes, 2))
    rows[:, :boxes, :2], rows[:, :boxes, 2:4] = xy0, xy0 + rng.uniform(20, 80, (B, boxes, 2))
    rows[:, :boxes, 4] = 0.9
    det.copy_(torch.from_numpy(rows).to(dev))
    n_keep.fill_(boxes)
    st.track_ids[:, :boxes] = torch.arange(1, boxes + 1, device=dev) * 37
    if trails:                                  # 32 steps of `trails` slots walking: dagr_stream_trail on a written state
        n = B * M
        ids = np.where(np.arange(M) < trails, 1 + np.arange(M), 0).astype(np.int64)
        c = rng.uniform(40, [W - 40, H - 40], (B, M, 2))
        v = rng.uniform(-4, 4, (B, M, 2))
        t_ref_where = st._t_ref_where()
        for k in range(32):
            box = np.concatenate([c + k * v - 10, c + k * v + 10], 2).astype(np.float32)
            t_last = np.full((B, M), T0 + WINDOW_US - 1, np.int64)
            raw = b"".join([np.tile(ids, (B, 1)).tobytes(), t_last.tobytes(), box.tobytes(), bytes(8 * n), bytes(8 * B)])
            st.track_state.copy_(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev))
            st.run_trail()
        assert t_ref_where is not None
        assert all(len(lane) == trails and all(len(p) == 32 for p in lane.values()) for lane in stream.trails())
    return stream, ev, (det, n_keep)


def new_path(stream, launches):
    for _ in range(5):
        stream.render_step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        stream.render_step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def host_path(stream, ev, det_n_keep, B):
    """The parent commit's way to a picture, once: milliseconds by the host's clock."""
    det, n_keep = det_n_keep
    black = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=det.device)       # (a base already on the device: not timed)
    torch.cuda.synchronize()
    c0 = time.perf_counter()
    counts = stream.counts()                                                    # the synchronisation
    xy, t, p, _ = (v.cpu().numpy() for v in ev)                                 # 13 bytes an event
    det_h, nk_h, ids_h = det.cpu().numpy(), n_keep.cpu().numpy(), stream.track_ids.cpu().numpy()
    rows, ptr = [], [0]
    for b in range(B):
        d = det_h[b, :int(nk_h[b])]
        rows.append(np.concatenate([np.floor(d[:, :4]), np.zeros((len(d), 1))], 1).astype(np.int64))
        ptr.append(ptr[-1] + len(d))
    out = render_frames(black, np.arange(B), xy[:, 0], xy[:, 1], p, np.concatenate([[0], np.cumsum(counts)]), alpha=0.5,
                        boxes=np.concatenate(rows), box_ptr=np.array(ptr), linewidth=1)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - c0) * 1e3
    assert tuple(out.shape) == (B, H, W, 3) and len(t) == int(counts.sum()) and ids_h.shape == det_h.shape[:2]
    return ms


def cell(v, d=3):
    return f"{float(np.median(v)):.{d}f} ({min(v):.{d}f} .. {max(v):.{d}f})"


def part_render(a):
    begin, end = markers("render")
    lines = [begin, "", f"`python tools/stream_render_probe.py --part render --launches {a.launches} --rounds {a.rounds}` at "
             f"commit {a.commit}, {torch.cuda.get_device_name(0)}, one process; ms, median (min .. max) over {a.rounds} rounds.",
             "", "| B | resident events | boxes a lane | live trails a lane | render_step(), device events, per call | host path "
             "(counts, read-back, render_frames), host clock | host path / render_step |", "|---|---|---|---|---|---|---|"]
    models = {}
    for B, n, boxes, trails in CONFIGS:
        model = models.setdefault(B, model_for(B))
        stream, ev, det = loaded_stream(model, B, n, boxes, trails)
        host_path(stream, ev, det, B)                                           # (warm: code objects, allocations)
        new, old = [], []
        for _ in range(a.rounds):
            new.append(new_path(stream, a.launches))
            old.append(host_path(stream, ev, det, B))
        assert stream.render_status() == []
        lines.append(f"| {B} | {n} | {boxes} | {trails} | {cell(new)} | {cell(old)} | {np.median(old) / np.median(new):.0f}x |")
        print(lines[-1], flush=True)
    lines += ["", end]
    if a.out:
        write_section(a.out, "render", "\n".join(lines) + "\n")


def part_step(a):
    begin, end = markers("step")
    model = model_for(1)
    warm = 8
    n_steps = WINDOW_US // a.step_us + warm + a.repeats * a.block
    duration = (n_steps + 1) * a.step_us
    x, y, t, p = syn.edges_window(a.per_step * (n_steps + 1), W, H, 5, window_us=duration, time_window=duration)
    d = torch.device("cuda:0")
    ev = (torch.from_numpy(np.stack([x, y], -1).astype(np.int16)).to(d),
          torch.from_numpy(np.int64(T0) + t.astype(np.int64)).to(d), torch.from_numpy(p.astype(np.int8)).to(d))
    with torch.no_grad():
        legs = {"track=": Leg(model, ev, WINDOW_US, track=True),
                "track=, render= (no render_step)": Leg(model, ev, WINDOW_US, track=True, render=True)}
        for leg in legs.values():
            run_block(leg, T0, a.step_us, WINDOW_US // a.step_us + warm)
        t_at = T0 + WINDOW_US + warm * a.step_us
        p50, order = {k: [] for k in legs}, list(legs)
        for r in range(a.repeats):
            k = r % len(order)
            for name in order[k:] + order[:k]:
                p50[name].append(float(np.median(run_block(legs[name], t_at, a.step_us, a.block))))
            t_at += a.block * a.step_us
    lines = [begin, "", f"`python tools/stream_render_probe.py --part step --block {a.block} --repeats {a.repeats}` at commit "
             f"{a.commit}, {torch.cuda.get_device_name(0)}, one process, alternating blocks; ms per step_device, the median of "
             f"the blocks' medians (min .. max over {a.repeats} blocks).", "", "| stream | ms per step |", "|---|---|"]
    lines += [f"| {name} | {cell(v)} |" for name, v in p50.items()] + ["", end]
    print("\n".join(lines), flush=True)
    if a.out:
        write_section(a.out, "step", "\n".join(lines) + "\n")


def part_kernels(a):
    B, n, boxes, trails = CONFIGS[a.config]
    stream, _, _ = loaded_stream(model_for(B), B, n, boxes, trails)
    for _ in range(200):
        stream.render_step()
    torch.cuda.synchronize()
    print(f"config {a.config}: B={B} events={n} boxes={boxes} trails={trails}: 200 render_step calls")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("render", "step", "kernels"), required=True)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--step_us", type=int, default=1000)
    ap.add_argument("--per_step", type=int, default=500, help="events a step: 500 leaves about 25 k in a 50 ms window")
    ap.add_argument("--config", type=int, default=0)
    ap.add_argument("--commit", default="(working tree)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_render_probe.py measures on the GPU; no device is available")
    {"render": part_render, "step": part_step, "kernels": part_kernels}[a.part](a)


if __name__ == "__main__":
    main()
