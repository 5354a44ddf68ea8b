#!/usr/bin/env python
"""tools/stream_hota_probe.py -- what HOTA on the device (``EventStream(track=, score=, identity=, hota=)``,
``dagr_stream_hota``, ``dagr_stream_hota_solve``) says about the trackers on the labelled synthetic scenes, and what it costs.

``--part scene``: the two scenes of ``tools/stream_assign_probe.py`` (the committed scene of ``profiles/stream_score.md`` and
the crowded one) through the four greedy tracker entries and through ``dagr_stream_track_optimal`` (plain, and motion +
rescue), each followed by ``dagr_stream_score``, ``dagr_stream_identity`` and ``dagr_stream_hota`` on what it left on the
device, then one ``dagr_stream_hota_solve``: HOTA, DetA, AssA, LocA beside MOTA and IDF1.  The same chain runs through the
definitions on the host (``TrackDefinition``, ``ScoreDefinition``, ``IdentityDefinition``, ``HotaDefinition``); every integer
of the solve must be equal and the fp64 sums within ``(pairs + 2) * 2**-52``, or the probe stops.

``--part cost``: (1) ``dagr_stream_identity`` alone and ``dagr_stream_hota`` alone in one process, ``--launches`` calls back to
back between two device events, ``--rounds`` rounds, at 32 labelled boxes against 64 hypotheses and at 256 against 256 (B = 1,
a log large enough for every call).  (2) ``dagr_stream_hota_solve`` between two device events, ``--rounds`` calls after a
warm-up: on the log of the committed scene (plain tracker, B = 2, 120 instants a lane) and on a full log of 1200 instants of
256 rows x 256 columns whose boxes reach their neighbours' (B = 1).  (3) On the host, for comparison, on the committed scene's
log: ``HotaDefinition.solve`` and the float restatement ``tests/stream_hota_cases.hota_float`` (numpy + scipy), wall clock.

Each part is one process; run them one at a time, each under a time limit of its own:

    timeout -k 10 300 python tools/stream_hota_probe.py --part scene --commit <hash> --out profiles/stream_hota.md && \\
    timeout -k 10 300 python tools/stream_hota_probe.py --part cost --commit <hash> --out profiles/stream_hota.md

``--out`` replaces the part's measured section of the file (between its two marker comments) and leaves the rest, which is
written by hand."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd import _lib                                                                  # noqa: E402
from dagr_amd import streaming as S                                                        # noqa: E402
from dagr_amd.utils import synthetic as syn                                                # noqa: E402
from tools import stream_assign_probe as ap_                                               # noqa: E402
from tools import stream_score_probe as sp                                                 # noqa: E402
from tools.stream_score_probe import SCENE, SCENE_TRACK, dev                               # noqa: E402

K = _lib.DEFINES["DAGR_HOTA_THRESHOLDS"]
VARIANTS = (("plain", None, None, None), ("motion", True, None, None), ("rescue", None, True, None), ("both", True, True, None),
            ("plain, assign=optimal", None, None, "optimal"), ("both, assign=optimal", True, True, "optimal"))


def markers(part):
    return (f"<!-- measured ({part}): written by tools/stream_hota_probe.py --part {part} --out, which replaces this section "
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


class Hota:
    """HOTA's state behind a ``DeviceChain`` with an identity state: the C entries, called as a C caller calls them."""

    def __init__(self, chain, max_instants):
        self.c, self.L, self.I = chain, chain.L, int(max_instants)
        self.B, self.M, self.T = chain.B, chain.s["max_objects"], chain.i["max_tracks"]
        d = chain.state.device
        self.state = torch.empty(self.L.dagr_stream_hota_bytes(self.B, self.M, self.T, self.I), dtype=torch.uint8, device=d)
        self.ws = torch.empty(self.L.dagr_stream_hota_workspace_bytes(self.B, self.M, self.T, self.I), dtype=torch.uint8, device=d)
        _lib.check(self.L.dagr_stream_hota_reset(_lib.ptr(self.state), self.state.numel(), self.B, self.M, self.T, self.I,
                                                 chain.stream), "dagr_stream_hota_reset")

    def step(self, det, n_keep, gt_box, gt_label, gt_id, n_gt):
        P, c = _lib.ptr, self.c
        box = P(c.motion_out[0]) if c.s["boxes"] == "track" else None
        G = int(gt_box.shape[1])
        _lib.check(self.L.dagr_stream_hota(P(self.state), self.state.numel(), self.B, self.M, self.T, self.I, P(c.identity_state),
                                           c.identity_state.numel(), P(c.state), c.state.numel(), P(det), P(n_keep), c.A, P(c.ids),
                                           box, P(gt_box), P(gt_label), P(gt_id), P(n_gt), G, c.outcome(G)[0], c.stream),
                   "dagr_stream_hota")

    def launch_solve(self):
        P = _lib.ptr
        _lib.check(self.L.dagr_stream_hota_solve(P(self.state), self.state.numel(), self.B, self.M, self.T, self.I, P(self.ws),
                                                 self.ws.numel(), self.c.stream), "dagr_stream_hota_solve")

    def solve(self):
        """``dagr_stream_hota_solve`` -> the dict ``EventStream.hota()`` returns."""
        self.launch_solve()
        B, at = self.B, 0
        sizes = (8 * B * self.M * self.T, 8 * B * self.M, 8 * B * self.T, 32 * B, 32 * K * B, 24 * K * B)
        offsets = []
        for n in sizes:                 # (include/dagr_hip.h: every array at the next multiple of 16 bytes)
            offsets.append(at)
            at += -(-n // 16) * 16
        raw = self.state[:at].cpu().numpy()
        words = raw[offsets[3]:offsets[3] + sizes[3]].view(np.int64).reshape(B, 4)
        count = raw[offsets[4]:offsets[4] + sizes[4]].view(np.int64).reshape(B, K, 4)
        sums = raw[offsets[5]:offsets[5] + sizes[5]].view(np.float64).reshape(B, K, 3)
        out = {name: count[:, :, i].copy() for i, name in enumerate(S.HOTA_COUNTERS)}
        out.update({name: sums[:, :, i].copy() for i, name in enumerate(S.HOTA_SUMS)})
        out.update({name: words[:, i].copy() for i, name in enumerate(S.HOTA_WORDS)})
        return out


def run_scene(scene, B, A, motion, rescue, assign, definition=True):
    """One variant through the device chain (and the definitions) -> (score totals, identity totals, HOTA totals, the
    HOTA definition or None)."""
    chain = (ap_.OptimalChain if assign else sp.DeviceChain)(B, A, SCENE_TRACK, motion, rescue, True, identity=True)
    hota = Hota(chain, S.HOTA_DEFAULTS["max_instants"])
    d = S.TrackDefinition(B, SCENE_TRACK, motion=motion, rescue=rescue, assign=assign)
    sc, idd, hd = S.ScoreDefinition(B, True), S.IdentityDefinition(B, True, True), S.HotaDefinition(B, True, True, True)
    for s in scene:
        chain.step(s)
        hota.step(*(dev(s[k]) for k in ("det", "n_keep", "gt_box", "gt_label", "gt_id", "n_gt")))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        if definition:
            ids, _ = d.step(s["det"], s["n_keep"], s["t_ref"])
            match, _ = sc.step(s["det"], s["n_keep"], ids, s["gt_box"], s["gt_label"], s["gt_id"], s["n_gt"])
            idd.step(s["det"], s["n_keep"], ids, s["gt_box"], s["gt_label"], s["gt_id"], s["n_gt"], match, sc.id)
            hd.step(s["det"], s["n_keep"], ids, s["gt_box"], s["gt_label"], s["gt_id"], s["n_gt"], match, sc.id, idd.track_id)
    solved = hota.solve()
    if definition:
        want = hd.solve()
        for k in S.HOTA_COUNTERS + S.HOTA_WORDS:
            if not np.array_equal(solved[k], want[k]):
                raise SystemExit(f"the device's {k} = {solved[k]} is not the definition's {want[k]}")
        pairs = (want["mc"] > 0).sum((2, 3))
        for k in S.HOTA_SUMS:
            if not np.all(np.abs(solved[k] - want[k]) <= (pairs + 2) * 2.0 ** -52 * want[k]):
                raise SystemExit(f"the device's {k} = {solved[k]} is not the definition's {want[k]}")
    counters, objects = chain.read()
    return (S.score_summary(counters, objects)["total"], S.identity_summary(chain.solve())["total"],
            S.hota_summary(solved)["total"], hd if definition else None, hota)


def part_scene(a):
    begin, end = markers("scene")
    lines = [begin, "",
             f"`python tools/stream_hota_probe.py --part scene --commit {a.commit}`, commit {a.commit}: the two labelled scenes of "
             "`profiles/stream_assign.md` -- `committed`: `track_scene(" + ", ".join(f"{k}={v}" for k, v in SCENE.items()) + ")`, "
             "`crowded`: `track_scene(" + ", ".join(f"{k}={v}" for k, v in ap_.CROWD.items()) + ")` -- through the tracker with "
             f"`min_score = {SCENE_TRACK['min_score']}`, `max_age_us = {SCENE_TRACK['max_age_us']}`, scored at IoU 0.5, "
             "`max_objects = max_tracks = 256`, `max_instants = 1200`.  Every row is the DEVICE's figures: the tracker's C entry, "
             "then `dagr_stream_score`, `dagr_stream_identity`, `dagr_stream_hota` at every step and one `dagr_stream_hota_solve`; "
             "they equal the definitions' chain on the host in every integer (the probe stops otherwise).  Totals over the lanes; "
             "HOTA, DetA, AssA: means over the 19 thresholds; LocA: over the thresholds with a TP.", "",
             "| scene | tracker | MOTA | IDF1 | HOTA | DetA | AssA | LocA | HOTA at 0.5 | TP at 0.5 | instants | alignment decides |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for scene_name, cfg in ap_.SCENES:
        scene = syn.track_scene(**cfg)
        for name, motion, rescue, assign in VARIANTS:
            m, i, h, hd, _ = run_scene(scene, cfg["B"], cfg["A"], motion, rescue, assign)
            lines.append(f"| {scene_name} | {name} | {m['mota']:.3f} | {i['idf1']:.3f} | {h['hota']:.3f} | {h['deta']:.3f} | "
                         f"{h['assa']:.3f} | {h['loca']:.3f} | {h['alphas']['hota'][9]:.3f} | {h['tp'][9]} | {h['instants']} | "
                         f"{hd.events['alignment_decides']} |")
    lines += ["", "`alignment decides`: the logged instants at which the pairing on alignment x similarity is not the pairing on "
              "the similarity alone (counted by the definition).", "", end]
    return "\n".join(lines) + "\n"


def overlapping_case(n):
    """``n`` labelled 8 x 8 boxes every 6 pixels on a 16-wide grid (a neighbour's IoU is 1 / 7) and ``n`` hypotheses with ids
    on them, one pixel to the right: every box reaches its neighbours'."""
    x, y = 6.0 * (np.arange(n) % 16), 6.0 * (np.arange(n) // 16)
    box = np.stack([x, y, x + 8, y + 8], -1).astype(np.float32)
    det = np.zeros((1, n, 6), np.float32)
    det[0, :, :4], det[0, :, 4] = box + np.array([1, 0, 1, 0], np.float32), 0.9
    return dict(det=det, n_keep=np.array([n], np.int32), ids=np.arange(1, n + 1, dtype=np.int64)[None], gt_box=box[None],
                gt_label=np.zeros((1, n), np.int32), gt_id=np.arange(1, n + 1, dtype=np.int64)[None], n_gt=np.array([n], np.int32))


def time_pair(G, hyps, count, rounds):
    """ms per call of ``dagr_stream_identity`` alone and of ``dagr_stream_hota`` alone on the same arrays, per round."""
    c = sp.launch_case(G, hyps)
    chain = sp.DeviceChain(1, hyps, True, None, None, dict(max_objects=256), identity=True)
    calls = 10 + rounds * count
    hota = Hota(chain, calls)
    chain.ids.copy_(dev(c["ids"]))
    t = [dev(c[k]) for k in ("det", "n_keep", "gt_box", "gt_label", "gt_id", "n_gt")]
    out = {"dagr_stream_identity": [], "dagr_stream_hota": []}
    chain.score(*t)                     # (both read what this left: every row scored and matched)
    for name, call in (("dagr_stream_identity", chain.identity), ("dagr_stream_hota", hota.step)):
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
    solved = hota.solve()
    assert solved["instants"][0] == calls and solved["dropped_instants"][0] == 0 and solved["rows"][0] == calls * G, solved
    assert solved["tp"][0, 0] == calls * min(G, hyps), solved
    return out


def time_solve(hota, rounds):
    ms = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        hota.launch_solve()
        b.record()
        torch.cuda.synchronize()
        if r:                           # (the first call is the warm-up)
            ms.append(a.elapsed_time(b))
    return ms


def part_cost(a):
    from tests.stream_hota_cases import hota_float
    begin, end = markers("cost")
    cell = lambda v, d=4: f"{float(np.median(v)):.{d}f} ({min(v):.{d}f} .. {max(v):.{d}f})"                  # noqa: E731
    lines = [begin, "",
             f"`python tools/stream_hota_probe.py --part cost --commit {a.commit}`, commit {a.commit}.", "",
             "`dagr_stream_identity` alone and `dagr_stream_hota` alone in one process: B = 1, `max_objects = 256`, `max_tracks = "
             f"256`, a log that holds every call, every labelled box lies on a hypothesis with an id; {a.launches} calls back to "
             f"back between two device events, {a.rounds} rounds; ms per call, median (min .. max) of the rounds.", "",
             "| labelled boxes x hypotheses | `dagr_stream_identity` | `dagr_stream_hota` |", "|---|---|---|"]
    for G, hyps in ((32, 64), (256, 256)):
        per = time_pair(G, hyps, a.launches, a.rounds)
        lines.append(f"| {G} x {hyps} | {cell(per['dagr_stream_identity'])} | {cell(per['dagr_stream_hota'])} |")
    # the committed scene's log, on the device and on the host
    scene = syn.track_scene(**SCENE)
    _, _, h, hd, hota = run_scene(scene, SCENE["B"], SCENE["A"], None, None, None)
    ms_scene = time_solve(hota, a.rounds)
    host = {}
    for name, call in (("`HotaDefinition.solve` (numpy integers)", hd.solve),
                       ("`hota_float` (numpy fp64 + scipy `linear_sum_assignment`)", lambda: hota_float(hd.log, 256, 256))):
        t0 = time.perf_counter()
        call()
        host[name] = 1e3 * (time.perf_counter() - t0)
    # a full log: 1200 instants of 256 x 256 whose boxes reach their neighbours'
    c = overlapping_case(256)
    chain = sp.DeviceChain(1, 256, True, None, None, dict(max_objects=256), identity=True)
    full = Hota(chain, 1200)
    chain.ids.copy_(dev(c["ids"]))
    t = [dev(c[k]) for k in ("det", "n_keep", "gt_box", "gt_label", "gt_id", "n_gt")]
    chain.score(*t)
    chain.identity(*t)
    for _ in range(1200):
        full.step(*t)
    ms_full = time_solve(full, a.rounds)
    solved = full.solve()
    assert solved["instants"][0] == 1200 and solved["rows"][0] == solved["columns"][0] == 1200 * 256, solved
    lines += ["", f"`dagr_stream_hota_solve` (the two memsets, the replay and the reduce) between two device events, {a.rounds} calls "
              "after a warm-up; ms per call, median (min .. max).", "", "| log | ms per solve |", "|---|---|",
              f"| the committed scene, plain tracker: B = 2, {h['instants']} instants, {h['tp'][0] + h['fn'][0]} rows "
              f"and {h['tp'][0] + h['fp'][0]} columns in all | {cell(ms_scene, 3)} |",
              f"| a full log: B = 1, 1200 instants of 256 x 256, boxes every 6 px (a neighbour's IoU is 1 / 7); "
              f"{int(solved['tp'][0, 0])} TPs at 0.05, HOTA {S.hota_summary(solved)['total']['hota']:.3f} | {cell(ms_full, 3)} |",
              "", "On the host, for comparison, the same log of the committed scene (one call each, wall clock, the probe's CPU):",
              "", "| what | ms |", "|---|---|"]
    lines += [f"| {name} | {v:.1f} |" for name, v in host.items()]
    lines += ["", end]
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("scene", "cost"), required=True)
    ap.add_argument("--launches", type=int, default=500)
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
