#!/usr/bin/env python
"""tools/stream_assign_probe.py -- what an optimal assignment in the tracker's match (``EventStream(track=,
assign="optimal")``, ``dagr_stream_track_optimal``) buys on labelled synthetic scenes, and what it costs beside the greedy
entries.

``--part scene``: the committed scene of ``tools/stream_score_probe.py`` and the crowded scene (``CROWD`` below) through all
four tracker variants, greedy beside optimal: the C entry followed by ``dagr_stream_score`` and ``dagr_stream_identity`` on
the ids it left on the device, beside ``TrackDefinition`` under ``ScoreDefinition`` / ``IdentityDefinition`` on the host.  The
two must be equal, counter for counter; the probe stops on a difference.  Id switches, misses, MOTA, IDF1, and the
definition's ``conflicts`` and ``reassigned`` rounds.

``--part cost``: ``dagr_stream_track`` against ``dagr_stream_track_optimal`` (flags 0) in one process, ``--launches`` calls
back to back between two device events, ``--rounds`` rounds, on a state that is put back in front of every round: 32 rows on
64 tracks without conflicts; the crowded scene's busiest step (the step and lane whose round one takes the definition the
most path steps); 256 rows on 256 tracks, every box reaching its neighbour's; and milliseconds per
``EventStream.step_device`` of a B = 1 stream in the setting of ``tools/stream_score_probe.py`` with ``track=``, without and
with ``assign="optimal"``.

Each part is one process; run them one at a time, each under a time limit of its own:

    timeout -k 10 300 python tools/stream_assign_probe.py --part scene --commit <hash> --out profiles/stream_assign.md && \\
    timeout -k 10 600 python tools/stream_assign_probe.py --part cost --commit <hash> --out profiles/stream_assign.md

``--out`` replaces the part's measured section of the file (between its two marker comments) and leaves the rest, which is
written by hand."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd import _lib                                                                  # noqa: E402
from dagr_amd import streaming as S                                                        # noqa: E402
from dagr_amd.utils import synthetic as syn                                                # noqa: E402
from tools import stream_score_probe as sp                                                 # noqa: E402
from tools.stream_score_probe import SCENE, SCENE_TRACK, VARIANTS, dev                     # noqa: E402

CROWD = dict(seed=4, B=2, objects=24, steps=120, A=48, width=160, height=120, labels=1)
SCENES = (("committed", SCENE), ("crowded", CROWD))


def markers(part):
    return (f"<!-- measured ({part}): written by tools/stream_assign_probe.py --part {part} --out, which replaces this section "
            "and nothing else -->", f"<!-- measured ({part}): end -->")


def write_section(path, part, text):
    begin, end = markers(part)
    old = open(path).read() if os.path.exists(path) else f"# {os.path.splitext(os.path.basename(path))[0]}\n"
    if begin in old and end in old:
        new = old[:old.index(begin)] + text.rstrip("\n") + old[old.index(end) + len(end):]
    else:
        new = old.rstrip("\n") + "\n\n" + text
    with open(path, "w") as f:
        f.write(new)


class OptimalChain(sp.DeviceChain):
    """``DeviceChain`` whose tracker entry is ``dagr_stream_track_optimal``, on the same state, with a workspace."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.assign_ws = torch.empty(self.L.dagr_stream_track_optimal_bytes(self.B, self.o["max_tracks"]), dtype=torch.uint8,
                                     device=self.tracks.device)

    def track(self, det, n_keep, t_ref):
        P, o, D = _lib.ptr, self.o, _lib.DEFINES
        flags, gains, outputs, second = 0, [0.0, 0.0], [None] * 7, [0.0, 0.0, None]
        if self.m is not None:
            flags, gains, outputs = flags | D["DAGR_TRACK_OPTIMAL_MOTION"], [self.m["alpha"], self.m["beta"]], [P(t) for t in self.motion_out]
        if self.r is not None:
            flags, second = flags | D["DAGR_TRACK_OPTIMAL_RESCUE"], [self.r["low_score"], self.r["iou"], P(self.rescued)]
        _lib.check(self.L.dagr_stream_track_optimal(P(self.tracks), self.tracks.numel(), self.B, o["max_tracks"], o["iou"],
                                                    o["max_age_us"], o["min_score"], *gains, P(det), P(n_keep), self.A, P(t_ref),
                                                    P(self.ids), P(self.hits), *outputs, P(self.untracked), *second, flags,
                                                    P(self.assign_ws), self.assign_ws.numel(), self.stream),
                   "dagr_stream_track_optimal")

    def step(self, s):
        det, n_keep, t_ref = dev(s["det"]), dev(s["n_keep"]), dev(s["t_ref"])
        self.track(det, n_keep, t_ref)
        labels = (dev(s["gt_box"]), dev(s["gt_label"]), dev(s["gt_id"]), dev(s["n_gt"]))
        self.score(det, n_keep, *labels)
        self.identity(det, n_keep, *labels)
        torch.cuda.synchronize()                    # (the inputs above live until here)


def run_scene(scene, B, A, motion, rescue, assign):
    """One variant through the device chain and through the definitions -> (score totals, identity totals, events)."""
    chain = (OptimalChain if assign else sp.DeviceChain)(B, A, SCENE_TRACK, motion, rescue, True, identity=True)
    d = S.TrackDefinition(B, SCENE_TRACK, motion=motion, rescue=rescue, assign=assign)
    sc, idd = S.ScoreDefinition(B, True), S.IdentityDefinition(B, True, True)
    for k, s in enumerate(scene):
        chain.step(s)
        ids, _ = d.step(s["det"], s["n_keep"], s["t_ref"])
        got = chain.ids.cpu().numpy()
        if any(not np.array_equal(got[b, :n], ids[b, :n]) for b, n in enumerate(s["n_keep"])):
            raise SystemExit(f"step {k}: the device's track ids are not the definition's")
        match, _ = sc.step(s["det"], s["n_keep"], ids, s["gt_box"], s["gt_label"], s["gt_id"], s["n_gt"])
        idd.step(s["det"], s["n_keep"], ids, s["gt_box"], s["gt_label"], s["gt_id"], s["n_gt"], match, sc.id)
    solved, want = chain.solve(), idd.solve()
    for k in S.IDENTITY_RESULT:
        if not np.array_equal(solved[k], want[k]):
            raise SystemExit(f"the device's {k} = {solved[k]} is not the definition's {want[k]}")
    counters, objects = chain.read()
    for k in S.SCORE_COUNTERS:
        if not np.array_equal(counters[k], sc.counters[k]):
            raise SystemExit(f"the device's {k} = {counters[k]} is not the definition's {sc.counters[k]}")
    if any(g.tobytes() != w.tobytes() for g, w in zip(objects, sc.objects())):
        raise SystemExit("the device's object tables are not the definition's")
    return S.score_summary(counters, objects)["total"], S.identity_summary(solved)["total"], d.events


def part_scene(a):
    begin, end = markers("scene")
    lines = [begin, "",
             f"`python tools/stream_assign_probe.py --part scene --commit {a.commit}`, commit {a.commit}.  The committed scene is "
             f"`track_scene({', '.join(f'{k}={v}' for k, v in SCENE.items())})` (12 places in 320 x 240, two labels), the crowded "
             f"scene `track_scene({', '.join(f'{k}={v}' for k, v in CROWD.items())})`; both {SCENE['steps']} steps of 1000 us at "
             f"the generator's default rates, through the tracker with `min_score = {SCENE_TRACK['min_score']}`, `max_age_us = "
             f"{SCENE_TRACK['max_age_us']}`, the other options at their defaults, scored at IoU 0.5 (`dagr_stream_score`, "
             "`dagr_stream_identity`, one `dagr_stream_identity_solve`).  Every row is the DEVICE's figures -- the greedy entry of "
             "the variant, or `dagr_stream_track_optimal` with the variant's flags -- and they equal `TrackDefinition` under "
             "`ScoreDefinition` / `IdentityDefinition` on the host: the track ids at every step, every counter, every table word "
             "and every integer of the solve (the probe stops otherwise).  Totals over the lanes.  `conflicts` / `reassigned`: "
             "the definition's rounds (one lane, one step, one round) in which a row or a track had two admissible partners / "
             "whose pairing is not what greedy gives on the same state, of `rounds`.", "",
             "| scene | tracker | match | gt | match | miss | false pos | id switches | frag | MOTA | IDF1 | IDP | IDR | tracks | "
             "conflicts | reassigned | rounds |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for scene_name, kw in SCENES:
        scene = syn.track_scene(**kw)
        for name, motion, rescue in VARIANTS:
            for assign in (None, "optimal"):
                m, i, ev = run_scene(scene, kw["B"], kw["A"], motion, rescue, assign)
                rounds = kw["B"] * kw["steps"] * (2 if rescue else 1)
                lines.append(f"| {scene_name} | {name} | {assign or 'greedy'} | {m['gt']} | {m['match']} | {m['miss']} | "
                             f"{m['false_pos']} | {m['switch']} | {m['frag']} | {m['mota']:.3f} | {i['idf1']:.3f} | {i['idp']:.3f} | "
                             f"{i['idr']:.3f} | {i['tracks']} | {ev.get('conflicts', '')} | {ev.get('reassigned', '')} | "
                             f"{rounds if assign else ''} |")
    lines += ["", end]
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------------------------------------ cost
def grid_step(n, width, t):
    """``n`` rows on a grid of boxes 20 px apart, ``width`` wide and 10 high: 10 is disjoint, 26 reaches the next box."""
    det = np.zeros((1, n, 6), np.float32)
    for i in range(n):
        x, y = 20.0 * (i % 20), 20.0 * (i // 20)
        det[0, i] = (x, y, x + width, y + 10, 0.9, 0)
    return dict(det=det, n_keep=np.array([n], np.int32), t_ref=np.array([t], np.int64))


def busiest_step():
    """The crowded scene's step and lane whose round one takes the definition's assignment the most path steps: (the state
    in front of it as the definition leaves it, the step cut to that lane, rows, live tracks, path steps)."""
    scene = syn.track_scene(**CROWD)
    d = S.TrackDefinition(CROWD["B"], SCENE_TRACK, assign="optimal")
    best = None
    for k, s in enumerate(scene):
        before = (d.id.copy(), d.t_last.copy(), d.box.copy(), d.label.copy(), d.hits.copy(), d.next_id.copy())
        d.step(s["det"], s["n_keep"], s["t_ref"])
        for r in d.rounds:
            if not (r["w"] > 0).any():      # (no live track yet: nothing to assign)
                continue
            stats = {}
            S.assign_max_weight_definition(r["w"], stats)
            if best is None or stats["steps"] > best[0]:
                b = r["lane"]
                best = (stats["steps"], k, b, [x[b:b + 1].copy() for x in before], len(r["rows"]), int((r["w"] > 0).any(0).sum()),
                        dict(det=s["det"][b:b + 1], n_keep=s["n_keep"][b:b + 1], t_ref=s["t_ref"][b:b + 1]))
    return best


def plain_state(fields, M):
    """dagr_stream_track's state of one lane from the definition's arrays, as include/dagr_hip.h lays it out."""
    ids, t_last, box, label, hits, next_id = fields
    return torch.from_numpy(np.concatenate([ids.reshape(-1).view(np.uint8), t_last.reshape(-1).view(np.uint8),
                                            np.ascontiguousarray(box).reshape(-1).view(np.uint8),
                                            label.reshape(-1).view(np.uint8), hits.reshape(-1).view(np.uint8),
                                            next_id.reshape(-1).view(np.uint8)])).cuda()


def time_entries(state, step, M, track, count, rounds):
    """ms per call of dagr_stream_track and of dagr_stream_track_optimal (flags 0) on ``step``, every round from ``state``:
    the first call of a round meets the tracks as they were, the calls behind it the tracks the call before left."""
    L, P, d = _lib.lib(), _lib.ptr, torch.device("cuda:0")
    o = S._track_options(track, "probe")
    det, n_keep, t_ref = dev(step["det"]), dev(step["n_keep"]), dev(step["t_ref"])
    A = int(det.shape[1])
    ids, hits = torch.zeros((1, A), dtype=torch.int64, device=d), torch.zeros((1, A), dtype=torch.int32, device=d)
    ws = torch.empty(L.dagr_stream_track_optimal_bytes(1, M), dtype=torch.uint8, device=d)
    work, stream = state.clone(), _lib.cur_stream(d)
    assert state.numel() == L.dagr_stream_track_bytes(1, M)

    def greedy():
        return L.dagr_stream_track(P(work), work.numel(), 1, M, o["iou"], o["max_age_us"], o["min_score"], P(det), P(n_keep), A,
                                   P(t_ref), P(ids), P(hits), None, stream)

    def optimal():
        return L.dagr_stream_track_optimal(P(work), work.numel(), 1, M, o["iou"], o["max_age_us"], o["min_score"], 0.0, 0.0, P(det),
                                           P(n_keep), A, P(t_ref), P(ids), P(hits), *[None] * 7, None, 0.0, 0.0, None, 0, P(ws),
                                           ws.numel(), stream)

    out, first = {}, {}
    for name, call in (("dagr_stream_track", greedy), ("dagr_stream_track_optimal", optimal)):
        out[name] = []
        for r in range(rounds + 1):
            work.copy_(state)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(count):
                _lib.check(call(), name)
            b.record()
            torch.cuda.synchronize()
            if r:                           # (the first round is the warm-up)
                out[name].append(a.elapsed_time(b) / count)
        work.copy_(state)                   # and the first call alone, the one that meets the step as the scene has it
        alone = []
        for _ in range(rounds):
            work.copy_(state)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            _lib.check(call(), name)
            b.record()
            torch.cuda.synchronize()
            alone.append(a.elapsed_time(b))
        first[name] = alone
    return out, first


def part_cost(a):
    from dagr_amd.model.networks.dagr import DAGR
    from dagr_amd.utils.args import model_args
    from dagr_amd.utils.testing_weights import randomize_
    from tools.stream_track_probe import H, T0, W, Leg, run_block
    begin, end = markers("cost")
    cell = lambda v, d=4: f"{float(np.median(v)):.{d}f} ({min(v):.{d}f} .. {max(v):.{d}f})"                  # noqa: E731
    L, P, d0 = _lib.lib(), _lib.ptr, torch.device("cuda:0")
    T = (1 << 33) + 5000

    def after(step, M, track):
        """The state one greedy step on an empty state leaves: every row a track."""
        o = S._track_options(track, "probe")
        st = torch.empty(L.dagr_stream_track_bytes(1, M), dtype=torch.uint8, device=d0)
        _lib.check(L.dagr_stream_track_reset(P(st), st.numel(), 1, M, _lib.cur_stream(d0)), "reset")
        det, nk, tr = dev(step["det"]), dev(step["n_keep"]), dev(step["t_ref"])
        A = int(det.shape[1])
        ids, hits = torch.zeros((1, A), dtype=torch.int64, device=d0), torch.zeros((1, A), dtype=torch.int32, device=d0)
        _lib.check(L.dagr_stream_track(P(st), st.numel(), 1, M, o["iou"], o["max_age_us"], o["min_score"], P(det), P(nk), A,
                                       P(tr), P(ids), P(hits), None, _lib.cur_stream(d0)), "dagr_stream_track")
        torch.cuda.synchronize()
        return st

    rows = []
    track = dict(max_tracks=64)
    rows.append(("32 rows x 64 tracks (32 live), disjoint boxes: no conflict, the solve is skipped",
                 time_entries(after(grid_step(32, 10, T), 64, track), grid_step(32, 10, T + 1000), 64, track, a.launches, a.rounds)))
    steps, k, b, fields, n_rows, n_tracks, step = busiest_step()
    rows.append((f"the crowded scene's busiest step (step {k}, lane {b}: {n_rows} rows, {n_tracks} tracks with an admissible row, {steps} path "
                 "steps in the definition), 64 slots",
                 time_entries(plain_state(fields, 64), step, 64, SCENE_TRACK, a.launches, a.rounds)))
    track = dict(max_tracks=256, iou=0.1)
    rows.append(("256 rows x 256 tracks, every box reaches its neighbour's (IoU 0.2 at a threshold of 0.1): one 256 x 256 solve",
                 time_entries(after(grid_step(256, 10, T), 256, track), grid_step(256, 26, T + 1000), 256, track,
                              max(1, a.launches // 10), a.rounds)))

    torch.manual_seed(0)
    args = model_args("dagr-s", batch_size=1)
    model = randomize_(DAGR(args, height=H, width=W), seed=0).eval().cuda()
    model.cache_luts(width=W, height=H, radius=args.radius)
    model.check_device_status = False
    warm = 8
    n_steps = a.window_us // a.step_us + warm + a.repeats * a.block
    duration = (n_steps + 1) * a.step_us
    x, y, t, p = syn.edges_window(a.per_step * (n_steps + 1), W, H, 5, window_us=duration, time_window=duration)
    ev = (torch.from_numpy(np.stack([x, y], -1).astype(np.int16)).to(d0),
          torch.from_numpy(np.int64(T0) + t.astype(np.int64)).to(d0), torch.from_numpy(p.astype(np.int8)).to(d0))
    with torch.no_grad():
        legs = {"off": Leg(model, ev, a.window_us), "track": Leg(model, ev, a.window_us, track=True),
                "track, assign=\"optimal\"": Leg(model, ev, a.window_us, track=True, assign="optimal")}
        for leg in legs.values():
            run_block(leg, T0, a.step_us, a.window_us // a.step_us + warm)
        t_at = T0 + a.window_us + warm * a.step_us
        p50, order = {k_: [] for k_ in legs}, list(legs)
        for r in range(a.repeats):
            k_ = r % len(order)
            for name in order[k_:] + order[:k_]:
                p50[name].append(float(np.median(run_block(legs[name], t_at, a.step_us, a.block))))
            t_at += a.block * a.step_us
        for leg in legs.values():
            leg.stream.check_status()
    lines = [begin, "",
             f"`python tools/stream_assign_probe.py --part cost --commit {a.commit}`, commit {a.commit}.", "",
             f"`dagr_stream_track` and `dagr_stream_track_optimal` (flags 0) alone, B = 1, in one process on the same state and "
             f"step: {a.launches} calls back to back between two device events ({max(1, a.launches // 10)} at 256 x 256), "
             f"{a.rounds} rounds after a warm-up, the state put back in front of every round; ms per call, median (min .. max) of "
             "the rounds.  The first call of a round meets the step as described, every later call the tracks the call before "
             "left (the same boxes again, at age 0).  `first call`: that one call alone between two events, which includes the "
             "launch.", "",
             "| step | `dagr_stream_track` | `dagr_stream_track_optimal` | ratio | first call, greedy | first call, optimal |",
             "|---|---|---|---|---|---|"]
    for name, (per, first) in rows:
        g, o = per["dagr_stream_track"], per["dagr_stream_track_optimal"]
        lines.append(f"| {name} | {cell(g)} | {cell(o)} | {float(np.median(o)) / float(np.median(g)):.2f} | "
                     f"{cell(first['dagr_stream_track'])} | {cell(first['dagr_stream_track_optimal'])} |")
    base = float(np.median(p50["track"]))
    lines += ["", f"`EventStream.step_device`, B = 1, {W}x{H}, dagr-s events-only, random weights, {a.step_us} us steps on a "
              f"{a.window_us} us window, {a.per_step} events a step; host clock around `step_device` and the device "
              "synchronisation behind it; the legs in one process on the same events, warmed until captured, alternating blocks "
              f"of {a.block} steps, {a.repeats} blocks each.  ms per step: median of the blocks' p50 (min .. max).", "",
              "| leg | ms per step | minus `track` |", "|---|---|---|"]
    lines += [f"| {name} | {cell(v, 3)} | {float(np.median(v)) - base:+.4f} |" for name, v in p50.items()]
    lines += ["", end]
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("scene", "cost"), required=True)
    ap.add_argument("--per_step", type=int, default=500)
    ap.add_argument("--step_us", type=int, default=1000)
    ap.add_argument("--window_us", type=int, default=50000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    text = {"scene": part_scene, "cost": part_cost}[a.part](a)
    print(text)
    if a.out:
        write_section(a.out, a.part, text)


if __name__ == "__main__":
    main()
