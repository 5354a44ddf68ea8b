#!/usr/bin/env python
"""tools/stream_score_probe.py -- what the stream's scorer (``EventStream(track=, score=)``, ``dagr_stream_score``) says about
the trackers on a labelled synthetic scene, and what it costs.

``--part scene``: the committed scene (``dagr_amd.utils.synthetic.track_scene``, the settings of ``SCENE`` below) through the
four tracker entries, each followed by ``dagr_stream_score`` on the track ids it left on the device: id switches,
fragmentations, MOTA, MOTP, mostly tracked / mostly lost per variant, beside the figures of ``TrackDefinition`` under
``ScoreDefinition`` on the host.  The two must be equal, counter for counter; the probe fails if they are not.  Every scored
step is followed by ``dagr_stream_identity`` and the scene by ``dagr_stream_identity_solve``: IDF1, IDP and IDR beside MOTA,
again device against definition (``IdentityDefinition``; the integers must be equal).

``--part identity``: (1) ``dagr_stream_score`` alone and ``dagr_stream_identity`` alone, ``--launches`` calls back to back
between two device events, ``--rounds`` rounds, at 32 labelled boxes against 64 hypotheses and at 256 against 256 (B = 1,
every box lies on a hypothesis).  (2) ``dagr_assign_max_weight`` on three large matrices, B = 1, ``--rounds`` calls each, beside
the path steps ``assign_max_weight_definition`` counts on the same matrix (the totals must be equal).

``--part cost``: (1) ``dagr_stream_score`` alone, ``--launches`` calls back to back between two device events, ``--rounds``
rounds, at G = 8 / 32 / 256 labelled boxes against 64 hypotheses (B = 1; the first ``min(G, 64)`` boxes lie on a hypothesis,
the rest are missed; every call after the first walks the keep round).  (2) Milliseconds per ``EventStream.step_device`` of a
B = 1 stream in the setting of ``tools/stream_rescue_probe.py`` (640x480 dagr-s, events only, random weights, 1 ms steps on a
50 ms window): without tracking, with ``track=``, with ``track=, score=`` and no ``score_step`` at all, and with a
``score_step`` of 32 labelled boxes behind every 50th step.  The legs alternate in one process, as that probe's do.

Each part is one process; run them one at a time, each under a time limit of its own:

    timeout -k 10 300 python tools/stream_score_probe.py --part scene --commit <hash> --out profiles/stream_score.md && \\
    timeout -k 10 600 python tools/stream_score_probe.py --part cost --commit <hash> --out profiles/stream_score.md
    timeout -k 10 300 python tools/stream_score_probe.py --part identity --commit <hash> --out profiles/stream_identity.md

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

SCENE = dict(seed=4, B=2, objects=12, steps=120, A=32)
SCENE_TRACK = dict(min_score=0.5, max_age_us=6000)
VARIANTS = (("plain", None, None), ("motion", True, None), ("rescue", None, True), ("both", True, True))
ENTRY = {"plain": "dagr_stream_track", "motion": "dagr_stream_track_cv", "rescue": "dagr_stream_track_rescue",
         "both": "dagr_stream_track_cv_rescue"}


def markers(part):
    return (f"<!-- measured ({part}): written by tools/stream_score_probe.py --part {part} --out, which replaces this section "
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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class DeviceChain:
    """One tracker entry on a state of its own, followed by the scorer on the ids it leaves: the C entries, called as a C
    caller calls them."""

    def __init__(self, B, A, track, motion, rescue, score, identity=None):
        self.L, P = _lib.lib(), _lib.ptr
        self.B, self.A = B, A
        self.o = S._track_options(track, "probe")
        self.m = S._motion_options(motion, self.o, "probe")
        self.r = S._rescue_options(rescue, self.o, "probe")
        self.s = S._score_options(score, self.o, self.m, "probe")
        self.family = "dagr_stream_track" + ("" if self.m is None else "_cv")
        M, d = self.o["max_tracks"], torch.device("cuda:0")
        self.stream = _lib.cur_stream(d)
        self.tracks = torch.empty(getattr(self.L, self.family + "_bytes")(B, M), dtype=torch.uint8, device=d)
        _lib.check(getattr(self.L, self.family + "_reset")(P(self.tracks), self.tracks.numel(), B, M, self.stream), "reset")
        z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=d)                  # noqa: E731
        self.ids, self.hits = z((B, A), torch.int64), z((B, A), torch.int32)
        self.motion_out = [z((B, A, 4), torch.float32), z((B, A, 4), torch.float32), z((B, M), torch.int64),
                           z((B, M, 4), torch.float32), z((B, M), torch.int32), z((B, M), torch.int64), z((B,), torch.int32)]
        self.untracked, self.rescued = z((B,), torch.int64), z((B,), torch.int64)
        self.state = torch.empty(self.L.dagr_stream_score_bytes(B, self.s["max_objects"]), dtype=torch.uint8, device=d)
        _lib.check(self.L.dagr_stream_score_reset(P(self.state), self.state.numel(), B, self.s["max_objects"], self.stream),
                   "score reset")
        self.i = S._identity_options(identity, self.s, "probe")
        if self.i is not None:          # the identity state behind the scorer's, and what the scorer has to leave for it
            M_, T = self.s["max_objects"], self.i["max_tracks"]
            self.identity_state = torch.empty(self.L.dagr_stream_identity_bytes(B, M_, T), dtype=torch.uint8, device=d)
            _lib.check(self.L.dagr_stream_identity_reset(P(self.identity_state), self.identity_state.numel(), B, M_, T,
                                                         self.stream), "identity reset")
            self.ws = torch.empty(self.L.dagr_assign_workspace_bytes(B, M_, T), dtype=torch.uint8, device=d)
            self.outcomes = {}          # G -> (gt_match [B, G], gt_flags [B, G])
            self.obj_track, self.result = z((B, M_), torch.int64), z((B, len(S.IDENTITY_RESULT)), torch.int64)

    def step(self, s):
        P, o = _lib.ptr, self.o
        det, n_keep, t_ref = dev(s["det"]), dev(s["n_keep"]), dev(s["t_ref"])
        gains = [] if self.m is None else [self.m["alpha"], self.m["beta"]]
        outputs = [] if self.m is None else [P(t) for t in self.motion_out]
        second = [] if self.r is None else [self.r["low_score"], self.r["iou"], P(self.rescued)]
        entry = self.family + ("" if self.r is None else "_rescue")
        _lib.check(getattr(self.L, entry)(P(self.tracks), self.tracks.numel(), self.B, o["max_tracks"], o["iou"], o["max_age_us"],
                                          o["min_score"], *gains, P(det), P(n_keep), self.A, P(t_ref), P(self.ids), P(self.hits),
                                          *outputs, P(self.untracked), *second, self.stream), entry)
        labels = (dev(s["gt_box"]), dev(s["gt_label"]), dev(s["gt_id"]), dev(s["n_gt"]))
        self.score(det, n_keep, *labels)
        if self.i is not None:
            self.identity(det, n_keep, *labels)
        torch.cuda.synchronize()                    # (the inputs above live until here)

    def score(self, det, n_keep, gt_box, gt_label, gt_id, n_gt):
        P = _lib.ptr
        box = P(self.motion_out[0]) if self.s["boxes"] == "track" else None
        _lib.check(self.L.dagr_stream_score(P(self.state), self.state.numel(), self.B, self.s["max_objects"], self.s["iou"], P(det),
                                            P(n_keep), self.A, P(self.ids), box, P(gt_box), P(gt_label), P(gt_id), P(n_gt),
                                            int(gt_box.shape[1]), *self.outcome(int(gt_box.shape[1])), self.stream),
                   "dagr_stream_score")

    def outcome(self, G):
        """``(gt_match, gt_flags)`` for ``G`` rows a lane: NULL without the identity state, which is what reads them."""
        if self.i is None:
            return None, None
        if G not in self.outcomes:
            d = self.state.device
            self.outcomes[G] = (torch.zeros((self.B, G), dtype=torch.int64, device=d),
                                torch.zeros((self.B, G), dtype=torch.int32, device=d))
        return tuple(_lib.ptr(t) for t in self.outcomes[G])

    def identity(self, det, n_keep, gt_box, gt_label, gt_id, n_gt):
        P = _lib.ptr
        box = P(self.motion_out[0]) if self.s["boxes"] == "track" else None
        G = int(gt_box.shape[1])
        _lib.check(self.L.dagr_stream_identity(P(self.identity_state), self.identity_state.numel(), self.B, self.s["max_objects"],
                                               self.i["max_tracks"], self.s["iou"], P(self.state), self.state.numel(), P(det),
                                               P(n_keep), self.A, P(self.ids), box, P(gt_box), P(gt_label), P(gt_id), P(n_gt), G,
                                               self.outcome(G)[0], self.stream), "dagr_stream_identity")

    def solve(self):
        """``dagr_stream_identity_solve`` -> the dict ``EventStream.identity()`` returns, without ``obj_track``."""
        P = _lib.ptr
        _lib.check(self.L.dagr_stream_identity_solve(P(self.identity_state), self.identity_state.numel(), self.B,
                                                     self.s["max_objects"], self.i["max_tracks"], P(self.obj_track),
                                                     P(self.result), P(self.ws), self.ws.numel(), self.stream),
                   "dagr_stream_identity_solve")
        result = self.result.cpu().numpy()
        return {name: result[:, i].copy() for i, name in enumerate(S.IDENTITY_RESULT)}

    def read(self):
        """``(counters, objects)`` as ``EventStream.track_score()`` / ``scored_objects()`` return them."""
        n, M = self.B * self.s["max_objects"], self.s["max_objects"]
        raw = self.state.view(torch.int64).cpu().numpy()
        table, words = raw[:8 * n].reshape(8, self.B, M), raw[8 * n:].reshape(self.B, 16)
        return ({name: words[:, 1 + i].copy() for i, name in enumerate(S.SCORE_COUNTERS)},
                [S.objects_from_arrays(int(words[b, 0]), *table[:, b]) for b in range(self.B)])


def part_scene(a):
    scene = syn.track_scene(**SCENE)
    begin, end = markers("scene")
    lines = [begin, "",
             f"`python tools/stream_score_probe.py --part scene --commit {a.commit}`, commit {a.commit}: "
             f"`track_scene({', '.join(f'{k}={v}' for k, v in SCENE.items())})` -- {SCENE['B']} lanes x {SCENE['objects']} places x "
             f"{SCENE['steps']} steps of 1000 us, the generator's default rates (4 % of steps start a 1..5 step gap, 5 % a 1..4 step "
             "score dip to 0.15..0.45, about 3 clutter rows a step, 1 px jitter, 1 % deaths, 1 % labels without an identity) -- "
             f"through the tracker with `min_score = {SCENE_TRACK['min_score']}`, `max_age_us = {SCENE_TRACK['max_age_us']}`, the "
             "other options at their defaults, scored at IoU 0.5.  `device`: the C entry followed by `dagr_stream_score` on the ids "
             "it left on the device; `definition`: `TrackDefinition` under `ScoreDefinition` on the host.  Totals over the lanes.  "
             "IDF1, IDP, IDR: `dagr_stream_identity` behind every scored step and one `dagr_stream_identity_solve` (`max_tracks = "
             "256`), against `IdentityDefinition`; `path steps`: what the definition's assignment took, both lanes.",
             "", "| tracker | where | gt | match | miss | false pos | id switches | frag | MOTA | MOTP | mostly tracked | mostly lost "
             "| objects | IDF1 | IDP | IDR | IDTP | labelled frames | tracked frames | tracks | path steps |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, motion, rescue in VARIANTS:
        chain = DeviceChain(SCENE["B"], SCENE["A"], SCENE_TRACK, motion, rescue, True, identity=True)
        d, sc = S.TrackDefinition(SCENE["B"], SCENE_TRACK, motion=motion, rescue=rescue), S.ScoreDefinition(SCENE["B"], True)
        idd = S.IdentityDefinition(SCENE["B"], True, True)
        for s in scene:
            chain.step(s)
            ids, _ = d.step(s["det"], s["n_keep"], s["t_ref"])
            match, _ = sc.step(s["det"], s["n_keep"], ids, s["gt_box"], s["gt_label"], s["gt_id"], s["n_gt"])
            idd.step(s["det"], s["n_keep"], ids, s["gt_box"], s["gt_label"], s["gt_id"], s["n_gt"], match, sc.id)
        stats = []
        solved, want = chain.solve(), idd.solve(stats)
        for k in S.IDENTITY_RESULT:
            if not np.array_equal(solved[k], want[k]):
                raise SystemExit(f"{name}: the device's {k} = {solved[k]} is not the definition's {want[k]}")
        path_steps = sum(st["steps"] for st in stats)
        counters, objects = chain.read()
        for k in S.SCORE_COUNTERS:
            if not np.array_equal(counters[k], sc.counters[k]):
                raise SystemExit(f"{name}: the device's {k} = {counters[k]} is not the definition's {sc.counters[k]}")
        if any(g.tobytes() != w.tobytes() for g, w in zip(objects, sc.objects())):
            raise SystemExit(f"{name}: the device's object tables are not the definition's")
        for where, m, i in (("device", S.score_summary(counters, objects)["total"], S.identity_summary(solved)["total"]),
                            ("definition", S.score_summary(sc.counters, sc.objects())["total"],
                             S.identity_summary(want)["total"])):
            lines.append(f"| {name} (`{ENTRY[name]}`) | {where} | {m['gt']} | {m['match']} | {m['miss']} | {m['false_pos']} | "
                         f"{m['switch']} | {m['frag']} | {m['mota']:.3f} | {m['motp']:.3f} | {m['mostly_tracked']} | "
                         f"{m['mostly_lost']} | {m['objects']} | {i['idf1']:.3f} | {i['idp']:.3f} | {i['idr']:.3f} | {i['idtp']} | "
                         f"{i['gt_frames']} | {i['hyp_frames']} | {i['tracks']} | {path_steps} |")
    lines += ["", "Device and definition are equal in every counter, every table word and every integer of the solve (the probe "
              "stops otherwise).", "", end]
    return "\n".join(lines) + "\n"


def launch_case(G, hyps=64):
    """``hyps`` hypotheses on a grid of disjoint boxes, G labelled boxes of which the first min(G, hyps) lie on one."""
    grid = lambda i: (20.0 * (i % 20), 20.0 * (i // 20), 20.0 * (i % 20) + 10, 20.0 * (i // 20) + 10)      # noqa: E731
    det = np.zeros((1, hyps, 6), np.float32)
    for i in range(hyps):
        det[0, i] = grid(i) + (0.9, i % 2)
    gt_box = np.array([[grid(g) for g in range(G)]], np.float32)
    return dict(det=det, n_keep=np.array([hyps], np.int32), ids=np.arange(1, hyps + 1, dtype=np.int64)[None],
                gt_box=gt_box, gt_label=(np.arange(G, dtype=np.int32) % 2)[None], gt_id=np.arange(1, G + 1, dtype=np.int64)[None],
                n_gt=np.array([G], np.int32))


def time_launches(G, count, rounds):
    c = launch_case(G)
    chain = DeviceChain(1, 64, True, None, None, dict(max_objects=256))
    chain.ids.copy_(dev(c["ids"]))
    t = [dev(c[k]) for k in ("det", "n_keep", "gt_box", "gt_label", "gt_id", "n_gt")]
    for _ in range(10):
        chain.score(*t)
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(count):
            chain.score(*t)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / count)
    counters, _ = chain.read()
    calls = 10 + rounds * count
    assert counters["steps"][0] == calls and counters["match"][0] == calls * min(G, 64) and counters["kept"][0] == (calls - 1) * min(G, 64)
    return out


def part_cost(a):
    from dagr_amd.model.networks.dagr import DAGR
    from dagr_amd.utils.args import model_args
    from dagr_amd.utils.testing_weights import randomize_
    from tools.stream_track_probe import H, T0, W, Leg, run_block
    begin, end = markers("cost")
    cell = lambda v, d=4: f"{float(np.median(v)):.{d}f} ({min(v):.{d}f} .. {max(v):.{d}f})"                  # noqa: E731
    per = {G: time_launches(G, a.launches, a.rounds) for G in (8, 32, 256)}
    torch.manual_seed(0)
    args = model_args("dagr-s", batch_size=1)
    model = randomize_(DAGR(args, height=H, width=W), seed=0).eval().cuda()
    model.cache_luts(width=W, height=H, radius=args.radius)
    model.check_device_status = False
    warm = 8
    n_steps = a.window_us // a.step_us + warm + a.repeats * a.block
    duration = (n_steps + 1) * a.step_us
    x, y, t, p = syn.edges_window(a.per_step * (n_steps + 1), W, H, 5, window_us=duration, time_window=duration)
    d = torch.device("cuda:0")
    ev = (torch.from_numpy(np.stack([x, y], -1).astype(np.int16)).to(d),
          torch.from_numpy(np.int64(T0) + t.astype(np.int64)).to(d), torch.from_numpy(p.astype(np.int8)).to(d))
    c = launch_case(32)
    labels = tuple(dev(c[k]) for k in ("gt_box", "gt_label", "gt_id", "n_gt"))

    class ScoredLeg(Leg):
        """A leg whose every ``every``-th step is followed by a score_step of 32 labelled boxes (device tensors)."""
        every, made = 50, 0

        def step(self, t_prev, t_now):
            out = super().step(t_prev, t_now)
            self.made += 1
            if self.made % self.every == 0:
                self.stream.score_step(*labels)
            return out

    with torch.no_grad():
        legs = {"off": Leg(model, ev, a.window_us), "track": Leg(model, ev, a.window_us, track=True),
                "track, score= (no score_step)": Leg(model, ev, a.window_us, track=True, score=True),
                "track, score=, a score_step every 50th step": ScoredLeg(model, ev, a.window_us, track=True, score=True)}
        for leg in legs.values():
            run_block(leg, T0, a.step_us, a.window_us // a.step_us + warm)
        t_at = T0 + a.window_us + warm * a.step_us
        p50, order = {k: [] for k in legs}, list(legs)
        for r in range(a.repeats):
            k = r % len(order)
            for name in order[k:] + order[:k]:
                p50[name].append(float(np.median(run_block(legs[name], t_at, a.step_us, a.block))))
            t_at += a.block * a.step_us
        scored = int(legs[order[-1]].stream.track_score()["steps"][0])
        for leg in legs.values():
            leg.stream.check_status()
    lines = [begin, "",
             f"`python tools/stream_score_probe.py --part cost --commit {a.commit}`, commit {a.commit}.", "",
             f"`dagr_stream_score` alone: B = 1, 64 hypotheses with ids, `max_objects = 256`, G labelled boxes of which the first "
             f"min(G, 64) lie on a hypothesis; {a.launches} calls back to back between two device events, {a.rounds} rounds; ms per "
             "call, median (min .. max) of the rounds.  Every timed call keeps every pair of the call before.", "",
             "| G | ms per call |", "|---|---|"]
    lines += [f"| {G} | {cell(v)} |" for G, v in per.items()]
    base = float(np.median(p50["track"]))
    lines += ["", f"`EventStream.step_device`, B = 1, {W}x{H}, dagr-s events-only, random weights, {a.step_us} us steps on a "
              f"{a.window_us} us window, {a.per_step} events a step; host clock around `step_device` (and the `score_step` behind "
              "it, in the last leg) and the device synchronisation behind it; the legs in one process on the same events, warmed "
              f"until captured, alternating blocks of {a.block} steps, {a.repeats} blocks each.  ms per step: median of the "
              f"blocks' p50 (min .. max).  The last leg made {scored} score_steps of 32 labelled boxes.", "",
              "| leg | ms per step | minus `track` |", "|---|---|---|"]
    lines += [f"| {name} | {cell(v, 3)} | {float(np.median(v)) - base:+.4f} |" for name, v in p50.items()]
    lines += ["", end]
    return "\n".join(lines) + "\n"


def time_pair(G, hyps, count, rounds):
    """ms per call of ``dagr_stream_score`` alone and of ``dagr_stream_identity`` alone on the same arrays, per round."""
    c = launch_case(G, hyps)
    chain = DeviceChain(1, hyps, True, None, None, dict(max_objects=256), identity=True)
    chain.ids.copy_(dev(c["ids"]))
    t = [dev(c[k]) for k in ("det", "n_keep", "gt_box", "gt_label", "gt_id", "n_gt")]
    out = {"dagr_stream_score": [], "dagr_stream_identity": []}
    for _ in range(10):
        chain.score(*t)                 # (the identity step reads what the last of these left: every row scored and matched)
    for name, call in (("dagr_stream_score", chain.score), ("dagr_stream_identity", chain.identity)):
        for _ in range(10):
            call(*t)
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(count):
                call(*t)
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / count)
    solved, calls = chain.solve(), 10 + rounds * count
    assert solved["gt_frames"][0] == calls * G and solved["hyp_frames"][0] == calls * hyps, solved
    assert solved["idtp"][0] == calls * min(G, hyps), solved
    return out


# the large matrices of tests/test_assign_gpu.py (tests/stream_identity_cases.py), by the same seeds
ASSIGN = (("256 x 300, weights 0..2", 6, 256, 300, 2, None), ("1024 x 1024, weights 0..1000", 7, 1024, 1024, 1000, None),
          ("1000 x 1024, weights 0..100 at 0.4 %", 8, 1000, 1024, 100, 0.004))


def time_assign(seed, n, m, high, density, rounds):
    rng = np.random.Generator(np.random.PCG64(seed))
    w = rng.integers(0, high + 1, (n, m)).astype(np.int32)
    if density is not None:
        w *= (rng.random((n, m)) < density).astype(np.int32)
    stats = {}
    total, _ = S.assign_max_weight_definition(w, stats)
    L, P, d = _lib.lib(), _lib.ptr, torch.device("cuda:0")
    wd, nr, nc = dev(w), dev(np.array([n], np.int32)), dev(np.array([m], np.int32))
    ws = torch.empty(L.dagr_assign_workspace_bytes(1, n, m), dtype=torch.uint8, device=d)
    row_col, out = torch.zeros((1, n), dtype=torch.int32, device=d), torch.zeros((1,), dtype=torch.int64, device=d)
    ms = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        _lib.check(L.dagr_assign_max_weight(P(wd), 1, n, m, P(nr), P(nc), n, m, P(row_col), P(out), P(ws), ws.numel(),
                                            _lib.cur_stream(d)), "dagr_assign_max_weight")
        b.record()
        torch.cuda.synchronize()
        if r:                           # (the first call is the warm-up)
            ms.append(a.elapsed_time(b))
    if int(out[0]) != total or S.check_assignment(w, total, row_col[0].cpu().numpy()) is not None:
        raise SystemExit(f"{n} x {m}: the device's total {int(out[0])} or its pairing is not right (definition: {total})")
    return ms, stats["steps"], total


def part_identity(a):
    begin, end = markers("identity")
    cell = lambda v, d=4: f"{float(np.median(v)):.{d}f} ({min(v):.{d}f} .. {max(v):.{d}f})"                  # noqa: E731
    lines = [begin, "",
             f"`python tools/stream_score_probe.py --part identity --commit {a.commit}`, commit {a.commit}.", "",
             "`dagr_stream_score` alone and `dagr_stream_identity` alone in one process: B = 1, `max_objects = 256`, `max_tracks = "
             f"256`, every labelled box lies on a hypothesis with an id; {a.launches} calls back to back between two device events, "
             f"{a.rounds} rounds; ms per call, median (min .. max) of the rounds.", "",
             "| labelled boxes x hypotheses | `dagr_stream_score` | `dagr_stream_identity` |", "|---|---|---|"]
    for G, hyps in ((32, 64), (256, 256)):
        per = time_pair(G, hyps, a.launches, a.rounds)
        lines.append(f"| {G} x {hyps} | {cell(per['dagr_stream_score'])} | {cell(per['dagr_stream_identity'])} |")
    lines += ["", f"`dagr_assign_max_weight`, B = 1 (one wave), one call between two device events, {a.rounds} calls after a warm-up; "
              "`path steps`: what `assign_max_weight_definition` counts on the same matrix (the kernel repeats them one for one; "
              "the totals are equal and the pairing is a right one, or the probe stops).", "",
              "| matrix | total | path steps | ms per call | us per path step |", "|---|---|---|---|---|"]
    for name, seed, n, m, high, density in ASSIGN:
        ms, steps, total = time_assign(seed, n, m, high, density, a.rounds)
        lines.append(f"| {name} | {total} | {steps} | {cell(ms, 2)} | {1e3 * float(np.median(ms)) / steps:.2f} |")
    lines += ["", end]
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("scene", "cost", "identity"), required=True)
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
    text = {"scene": part_scene, "cost": part_cost, "identity": part_identity}[a.part](a)
    print(text)
    if a.out:
        write_section(a.out, a.part, text)


if __name__ == "__main__":
    main()
