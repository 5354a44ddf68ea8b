#!/usr/bin/env python
"""tools/stream_labels_probe.py -- what scoring every step against interpolated keyframes (``EventStream(labels=)``,
``dagr_stream_labels_push`` / ``dagr_stream_labels_at``) says that scoring the keyframes alone does not, and what it costs.

``--part scene``: the labelled scene of ``profiles/stream_score.md`` (``dagr_amd.utils.synthetic.track_scene``, ``SCENE`` below,
run on to ``--steps`` steps of 1000 us so that it holds several keyframes) through the tracker entries, scored three ways on the
device -- at the keyframes alone (every ``--every``-th step, the scene's true boxes), at every step against the keyframes
interpolated by ``dagr_stream_labels_at`` at the step's own ``t_ref``, and at every step against the scene's true boxes --
for the plain tracker and with ``motion=`` + ``rescue=``: MOTA, id switches, IDF1, HOTA.  A report, not a pass criterion.

``--part cost``: (1) ``dagr_stream_labels_at`` and a one-keyframe ``dagr_stream_labels_push`` at 32 and at 256 rows beside
``dagr_stream_score`` at 32 boxes against 64 hypotheses, in one process: ``--launches`` calls back to back between two device
events, ``--rounds`` rounds.  (2) Wall time of ``score_step()`` on a B = 1 stream of the tiny test model against the host path
in the same process: read ``t_ref`` back, interpolate in numpy (``LabelDefinition``), upload, ``score_step(arrays)``.

Each part is one process; run them one at a time, each under a time limit of its own:

    timeout -k 10 300 python tools/stream_labels_probe.py --part scene --commit <hash> --out profiles/stream_labels.md && \\
    timeout -k 10 300 python tools/stream_labels_probe.py --part cost --commit <hash> --out profiles/stream_labels.md

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
from tools.stream_score_probe import SCENE, SCENE_TRACK, DeviceChain, dev, launch_case                # noqa: E402

NAME = "tools/stream_labels_probe.py"
TRACKERS = (("plain", None, None), ("motion= + rescue=", True, True))
HOTA = dict(max_instants=1200)


def markers(part):
    return (f"<!-- measured ({part}): written by {NAME} --part {part} --out, which replaces this section and nothing else -->",
            f"<!-- measured ({part}): end -->")


def write_section(path, part, text):
    begin, end = markers(part)
    old = open(path).read() if os.path.exists(path) else f"# {os.path.splitext(os.path.basename(path))[0]}\n"
    if begin in old and end in old:
        new = old[:old.index(begin)] + text.rstrip("\n") + old[old.index(end) + len(end):]
    else:
        new = old.rstrip("\n") + "\n\n" + text
    with open(path, "w") as f:
        f.write(new)


class Store:
    """The label store's two entries on a state of their own, called as a C caller calls them."""

    def __init__(self, B, labels):
        self.L, self.B, self.o = _lib.lib(), B, S._label_options(labels, "probe")
        d = torch.device("cuda:0")
        self.stream, K, R = _lib.cur_stream(d), self.o["max_keyframes"], self.o["max_rows"]
        self.state = torch.empty(self.L.dagr_stream_labels_bytes(B, K, R), dtype=torch.uint8, device=d)
        _lib.check(self.L.dagr_stream_labels_reset(_lib.ptr(self.state), self.state.numel(), B, K, R, self.stream), "labels reset")
        self.out = (torch.zeros((B, R, 4), dtype=torch.float32, device=d), torch.zeros((B, R), dtype=torch.int32, device=d),
                    torch.zeros((B, R), dtype=torch.int64, device=d), torch.zeros((B,), dtype=torch.int32, device=d))

    def push(self, t, n, xywh, label, ident):
        P = _lib.ptr
        _lib.check(self.L.dagr_stream_labels_push(P(self.state), self.state.numel(), self.B, self.o["max_keyframes"],
                                                  self.o["max_rows"], int(t.shape[1]), P(t), P(n), P(xywh), P(label), P(ident),
                                                  self.stream), "dagr_stream_labels_push")

    def at(self, t_ref):
        P, nan = _lib.ptr, float("nan")
        _lib.check(self.L.dagr_stream_labels_at(P(self.state), self.state.numel(), self.B, self.o["max_keyframes"],
                                                self.o["max_rows"], P(t_ref), self.o["max_gap_us"] or 0, nan, nan,
                                                *(P(v) for v in self.out), self.stream), "dagr_stream_labels_at")
        return self.out


class Chain(DeviceChain):
    """``DeviceChain`` with HOTA's state behind the identity state, and the ground truth handed in as device tensors."""

    def __init__(self, B, A, motion, rescue):
        super().__init__(B, A, SCENE_TRACK, motion, rescue, True, identity=True)
        self.h = S._hota_options(HOTA, self.i, "probe")
        M, T, I, P = self.s["max_objects"], self.i["max_tracks"], self.h["max_instants"], _lib.ptr
        d = self.state.device
        self.hota_state = torch.empty(self.L.dagr_stream_hota_bytes(B, M, T, I), dtype=torch.uint8, device=d)
        self.hota_ws = torch.empty(self.L.dagr_stream_hota_workspace_bytes(B, M, T, I), dtype=torch.uint8, device=d)
        _lib.check(self.L.dagr_stream_hota_reset(P(self.hota_state), self.hota_state.numel(), B, M, T, I, self.stream), "hota reset")

    def track(self, s):
        """The tracker entry alone; returns the step's ``(det, n_keep)`` on the device."""
        P, o = _lib.ptr, self.o
        det, n_keep, t_ref = dev(s["det"]), dev(s["n_keep"]), dev(s["t_ref"])
        gains = [] if self.m is None else [self.m["alpha"], self.m["beta"]]
        outputs = [] if self.m is None else [P(t) for t in self.motion_out]
        second = [] if self.r is None else [self.r["low_score"], self.r["iou"], P(self.rescued)]
        entry = self.family + ("" if self.r is None else "_rescue")
        _lib.check(getattr(self.L, entry)(P(self.tracks), self.tracks.numel(), self.B, o["max_tracks"], o["iou"], o["max_age_us"],
                                          o["min_score"], *gains, P(det), P(n_keep), self.A, P(t_ref), P(self.ids), P(self.hits),
                                          *outputs, P(self.untracked), *second, self.stream), entry)
        return det, n_keep, t_ref

    def labelled(self, det, n_keep, gt):
        """The scorer chain -- score, identity, HOTA's pass 1 -- on ``gt = (gt_box, gt_label, gt_id, n_gt)``."""
        P, G = _lib.ptr, int(gt[0].shape[1])
        self.score(det, n_keep, *gt)
        self.identity(det, n_keep, *gt)
        _lib.check(self.L.dagr_stream_hota(P(self.hota_state), self.hota_state.numel(), self.B, self.s["max_objects"],
                                           self.i["max_tracks"], self.h["max_instants"], P(self.identity_state),
                                           self.identity_state.numel(), P(self.state), self.state.numel(), P(det), P(n_keep), self.A,
                                           P(self.ids), None, *(P(v) for v in gt), G, self.outcome(G)[0], self.stream),
                   "dagr_stream_hota")
        torch.cuda.synchronize()

    def hota(self):
        """``dagr_stream_hota_solve`` -> the dict ``EventStream.hota()`` returns, through the documented layout."""
        P, B = _lib.ptr, self.B
        M, T, I = self.s["max_objects"], self.i["max_tracks"], self.h["max_instants"]
        _lib.check(self.L.dagr_stream_hota_solve(P(self.hota_state), self.hota_state.numel(), B, M, T, I, P(self.hota_ws),
                                                 self.hota_ws.numel(), self.stream), "dagr_stream_hota_solve")
        K, at, out = _lib.DEFINES["DAGR_HOTA_THRESHOLDS"], 0, {}
        for name, dtype, shape in (("pmc", np.int64, (B, M, T)), ("gc", np.int64, (B, M)), ("tc", np.int64, (B, T)),
                                   ("words", np.int64, (B, 4)), ("count", np.int64, (B, K, 4)), ("sums", np.float64, (B, K, 3))):
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            out[name] = self.hota_state[at:at + nbytes].cpu().numpy().view(dtype).reshape(shape)
            at += -(-nbytes // 16) * 16
        res = {name: out["count"][:, :, i] for i, name in enumerate(S.HOTA_COUNTERS)}
        res.update({name: out["sums"][:, :, i] for i, name in enumerate(S.HOTA_SUMS)})
        res.update({name: out["words"][:, i] for i, name in enumerate(S.HOTA_WORDS)})
        return res


def part_scene(a):
    scene = syn.track_scene(**dict(SCENE, steps=a.steps))
    B, G = SCENE["B"], SCENE["objects"]
    begin, end = markers("scene")
    lines = [begin, "",
             f"`python {NAME} --part scene --commit {a.commit}`, commit {a.commit}: "
             f"`track_scene({', '.join(f'{k}={v}' for k, v in dict(SCENE, steps=a.steps).items())})` -- the scene of "
             f"`profiles/stream_score.md` run on to {a.steps} steps of 1000 us so that it holds {1 + (a.steps - 1) // a.every} "
             f"keyframes, one every {a.every}th step -- through the tracker (`min_score = {SCENE_TRACK['min_score']}`, `max_age_us = "
             f"{SCENE_TRACK['max_age_us']}`), scored at IoU 0.5 on the device three ways.  `keyframes alone`: `dagr_stream_score` "
             "(+ identity, HOTA) at the keyframe steps only, on the scene's true boxes.  `interpolated`: at every step, on what "
             "`dagr_stream_labels_at` makes of the keyframes at the step's own `t_ref` (the store is fed one keyframe ahead).  "
             "`true boxes`: at every step, on the scene's true boxes of that step.  Totals over the lanes.", "",
             "| tracker | scored | steps scored | gt | miss | false pos | id switches | MOTA | IDF1 | HOTA | DetA | AssA |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    keys = list(range(0, a.steps, a.every))
    for name, motion, rescue in TRACKERS:
        for how in ("keyframes alone", "interpolated", "true boxes"):
            chain, store, pushed = Chain(B, SCENE["A"], motion, rescue), Store(B, dict(max_keyframes=64, max_rows=G)), 0
            for k, s in enumerate(scene):
                det, n_keep, t_ref = chain.track(s)
                if how == "interpolated":
                    while pushed < len(keys) and (pushed == 0 or keys[pushed - 1] <= k):       # one keyframe ahead of the step
                        q = scene[keys[pushed]]
                        box = q["gt_box"].astype(np.float64)
                        xywh = np.concatenate([box[..., :2], box[..., 2:] - box[..., :2]], -1)
                        store.push(dev(q["t_ref"][:, None]), dev(q["n_gt"][:, None]), dev(xywh[:, None]),
                                   dev(q["gt_label"][:, None]), dev(q["gt_id"][:, None]))
                        pushed += 1
                    chain.labelled(det, n_keep, store.at(t_ref))
                elif how == "true boxes" or k % a.every == 0:
                    chain.labelled(det, n_keep, tuple(dev(s[v]) for v in ("gt_box", "gt_label", "gt_id", "n_gt")))
                torch.cuda.synchronize()
            counters, objects = chain.read()
            m, i = S.score_summary(counters, objects)["total"], S.identity_summary(chain.solve())["total"]
            h = S.hota_summary(chain.hota())["total"]
            lines.append(f"| {name} | {how} | {int(counters['steps'].sum())} | {m['gt']} | {m['miss']} | {m['false_pos']} | "
                         f"{m['switch']} | {m['mota']:.3f} | {i['idf1']:.3f} | {h['hota']:.3f} | {h['deta']:.3f} | {h['assa']:.3f} |")
    lines += ["", end]
    return "\n".join(lines) + "\n"


def time_calls(call, count, rounds):
    for _ in range(10):
        call()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(count):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / count)
    return out


def part_cost(a):
    begin, end = markers("cost")
    cell = lambda v, d=4: f"{float(np.median(v)):.{d}f} ({min(v):.{d}f} .. {max(v):.{d}f})"                  # noqa: E731
    rng = np.random.default_rng(3)
    rows = {}
    for R in (32, 256):
        store = Store(1, dict(max_keyframes=8, max_rows=R))
        frames = []
        for f in range(2):
            xywh = np.concatenate([rng.uniform(0, 300, (1, 1, R, 2)), rng.uniform(5, 40, (1, 1, R, 2))], -1)
            frames.append((dev(np.array([[1000 + 50000 * f]], np.int64)), dev(np.array([[R]], np.int32)), dev(xywh),
                           dev(np.zeros((1, 1, R), np.int32)), dev(rng.permutation(R).astype(np.int64)[None, None] + 1)))
            store.push(*frames[-1])
        t_ref = dev(np.array([1000 + 12345], np.int64))
        ms_at = time_calls(lambda: store.at(t_ref), a.launches, a.rounds)
        assert int(store.out[3][0]) == R
        # a one-keyframe push: the instants have to rise, so every call pushes the next one, from device arrays prepared in
        # front of the clock
        calls = 10 + a.launches * a.rounds
        later = [dev(np.array([[200000 + i]], np.int64)) for i in range(calls)]
        it = iter(later)
        ms_push = time_calls(lambda: store.push(next(it), *frames[0][1:]), a.launches, a.rounds)
        words = store.state[:64].view(torch.int64).cpu().numpy()
        assert words[0] == 8 and words[2] == 0 and words[4] == calls + 2 - 8, words
        rows[R] = (ms_at, ms_push)
    c = launch_case(32)
    chain = DeviceChain(1, 64, True, None, None, dict(max_objects=256))
    chain.ids.copy_(dev(c["ids"]))
    t = [dev(c[k]) for k in ("det", "n_keep", "gt_box", "gt_label", "gt_id", "n_gt")]
    ms_score = time_calls(lambda: chain.score(*t), a.launches, a.rounds)
    lines = [begin, "", f"`python {NAME} --part cost --commit {a.commit}`, commit {a.commit}.", "",
             f"The entries alone, B = 1, in one process: {a.launches} calls back to back between two device events, {a.rounds} "
             "rounds; ms per call, median (min .. max) of the rounds.  `dagr_stream_labels_at`: two resident keyframes of R rows "
             "with the same R identities in shuffled order, `t_ref` inside them, every row written.  `dagr_stream_labels_push`: one "
             "keyframe of R rows a call onto a full ring of 8.  `dagr_stream_score`: 32 labelled boxes against 64 hypotheses, "
             "`max_objects = 256`.", "", "| entry | rows | ms per call |", "|---|---|---|"]
    for R, (ms_at, ms_push) in rows.items():
        lines += [f"| `dagr_stream_labels_at` | {R} | {cell(ms_at)} |", f"| `dagr_stream_labels_push` | {R} | {cell(ms_push)} |"]
    lines.append(f"| `dagr_stream_score` | 32 x 64 | {cell(ms_score)} |")

    # ---- score_step() against the host path, on a stream of the tiny test model
    from tests.test_stream_rescue_gpu import _events, _step
    from tests.test_streaming_gpu import _model
    model = _model(1)
    model.check_device_status = False
    G, per = 32, {"score_step()": [], "host path": []}
    xywh0 = np.concatenate([rng.uniform(0, 250, (G, 2)), rng.uniform(8, 40, (G, 2))], -1)
    clock = int(np.asarray(_events(0, lanes=1)["t_now"]).reshape(-1)[0])      # the instant of the stream's first step
    frames = [(clock + 50000 * f, xywh0 + 3.0 * f, np.zeros(G, np.int32), np.arange(1, G + 1, dtype=np.int64)) for f in range(6)]
    streams = {}
    for name in per:
        st = S.EventStream(model, window_us=20000, track=True, score=True, labels=dict(max_rows=G) if name == "score_step()" else None)
        d = S.LabelDefinition(1, dict(max_rows=G))
        for t, x, lab, ids in frames:
            d.push(0, t, x, lab, ids)
            if st.labels is not None:
                st.push_labels(np.array([t]), x[None], lab[None], ids[None])
        streams[name] = (st, d)
    where = {}
    with torch.no_grad():
        for k in range(a.steps_timed + 20):
            for name, (st, d) in streams.items():
                _step(st, _events(k, lanes=1))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "score_step()":
                    st.score_step()
                else:
                    if name not in where:
                        base = _lib.lib().dagr_stream_t_ref(_lib.ptr(st.state.state), 1, st.state.cap) - st.state.state.data_ptr()
                        where[name] = st.state.state[base:base + 8].view(torch.int64)
                    t_ref = where[name].cpu().numpy()                     # the read-back: one synchronisation a step
                    st.score_step(*d.at(t_ref))
                torch.cuda.synchronize()
                if k >= 20:
                    per[name].append(1e3 * (time.perf_counter() - t0))
    lines += ["", f"`score_step()` against the host path in one process: B = 1, the tiny test model, {a.steps_timed} timed steps of 1 ms "
              f"after 20 warm-up steps, {G} labelled rows, the two streams stepped alternately on the same events; host clock around "
              "the call with a device synchronisation on either side.  `host path`: read `t_ref` back, `LabelDefinition.at` in "
              "numpy, upload, `score_step(arrays)`.  ms per call: median (min .. max) of the steps.", "",
              "| path | ms per call |", "|---|---|"]
    lines += [f"| {name} | {cell(v, 3)} |" for name, v in per.items()]
    lines += ["", end]
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("scene", "cost"), required=True)
    ap.add_argument("--steps", type=int, default=501)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps_timed", type=int, default=200)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    text = {"scene": part_scene, "cost": part_cost}[a.part](a)
    print(text)
    if a.out:
        write_section(a.out, a.part, text)


if __name__ == "__main__":
    main()
