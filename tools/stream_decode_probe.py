#!/usr/bin/env python
"""tools/stream_decode_probe.py -- what decoding the camera's words on the device costs against today's path.

B = 1, a 640x480 sensor (no downsampling; dagr-s, events only, random weights), 1 ms steps on a 50 ms window, the synthetic
S-edges stream at rates that leave about 25 k and 100 k resident events, encoded step by step as EVT 3.0 before any clock
starts (``dagr_amd.data.evt.encode_events``: the encoding is the camera's work).  Legs, all on host inputs (the upload is
part of a step), in this one process on the same model, warmed until the window is captured, run in alternating blocks of
``--block`` steps over the same stretch of the stream; the clock is the host's around the call that ends in the detections'
read-back:

* ``step``: ``EventStream.step`` on the pre-decoded arrays -- today's path, the yardstick;
* ``host+step``: a numpy-vectorised host decode of the step's words (``host_decode_evt3`` below) and then ``step``;
* ``words``: ``EventStream(decode="evt3").step_words``, ``max_decoded=None`` (the worst case: 12 rows per word);
* ``words tight``: the same with ``max_decoded`` = twice the largest push's events;
* the last three again with the noise filter on (``denoise_us=2000, refractory_us=1``), which sorts every row it is handed.

    python tools/stream_decode_probe.py --commit <hash> --out profiles/stream_decode.md

The decoder's launches by name come from ``rocprofv3 --kernel-trace --stats -- python tools/stream_decode_probe.py --trace``
(the ``words tight`` leg at the larger rate and nothing else)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagr_amd.data.evt import encode_events                      # noqa: E402
from dagr_amd.model.networks.dagr import DAGR                    # noqa: E402
from dagr_amd.streaming import DecodeDefinition, EventStream     # noqa: E402
from dagr_amd.utils import synthetic as syn                      # noqa: E402
from dagr_amd.utils.args import model_args                       # noqa: E402
from dagr_amd.utils.testing_weights import randomize_            # noqa: E402

W, H = 640, 480
T0 = 1 << 33
NOISE = dict(denoise_us=2000, refractory_us=1)


def host_decode_evt3(words, st):
    """EVT 3.0 words -> (xy int16[n,2], t int64, p int8) with numpy array operations, no loop over words: last-writer-wins by
    ``maximum.accumulate`` of positions, wraps and vector bases by ``cumsum``.  ``st``: the state carried between pushes
    (high, low, loops, y, base, pol).  For a synced stream inside the sensor, which is what the probe pushes."""
    w = words.astype(np.int64)
    n = len(w)
    if n == 0:
        return np.zeros((0, 2), np.int16), np.zeros(0, np.int64), np.zeros(0, np.int8)
    typ, idx = w >> 12, np.arange(n)

    def last(mask, vals, init):
        pos = np.maximum.accumulate(np.where(mask, idx, -1))
        return np.where(pos >= 0, vals[np.maximum(pos, 0)], init), pos

    y, _ = last(typ == 0, w & 0x7FF, st["y"])
    low, _ = last(typ == 6, w & 0xFFF, st["low"])
    is_h, hv = typ == 8, w & 0xFFF
    high, _ = last(is_h, hv, st["high"])
    loops = st["loops"] + np.cumsum(is_h & (np.concatenate([[st["high"]], high[:-1]]) - hv >= 2048))
    t = (loops << 24) + (high << 12) + low
    inc = np.where(typ == 4, 12, np.where(typ == 5, 8, 0))
    c = np.cumsum(inc)
    base_set, bpos = last(typ == 3, w & 0x7FF, st["base"])
    base = base_set + c - np.where(bpos >= 0, c[np.maximum(bpos, 0)], 0)       # behind the word
    pol, _ = last(typ == 3, (w >> 11) & 1, st["pol"])
    single = typ == 2
    mask = np.where(typ == 4, w & 0xFFF, np.where(typ == 5, w & 0xFF, 0))
    mask[single] = 1
    wi, bi = np.nonzero((mask[:, None] >> np.arange(12)) & 1)
    x = np.where(single[wi], w[wi] & 0x7FF, base[wi] - inc[wi] + bi)
    p = np.where(single[wi], (w[wi] >> 11) & 1, pol[wi]) * 2 - 1
    st.update(high=int(high[-1]), low=int(low[-1]), loops=int(loops[-1]), y=int(y[-1]), base=int(base[-1]), pol=int(pol[-1]))
    return np.stack([x, y[wi]], -1).astype(np.int16), t[wi] + T0, p.astype(np.int8)


def make_steps(events_per_step, step_us, n_steps, seed=5):
    """Per step: (xy, t, p) and its EVT 3.0 words; times on the wire are relative to T0."""
    x, y, t, p = syn.edges_window(events_per_step * n_steps, W, H, seed, window_us=n_steps * step_us,
                                  time_window=n_steps * step_us)
    t = t.astype(np.int64)
    o = np.lexsort((x, y, t))                   # (one instant: row by row, ascending x -- what lets the encoder vectorise)
    x, y, t, p = x[o], y[o], t[o], p[o]
    steps, prev = [], None
    for k in range(n_steps):
        i0, i1 = np.searchsorted(t, [k * step_us, (k + 1) * step_us], side="left")
        words = encode_events(x[i0:i1], y[i0:i1], t[i0:i1], p[i0:i1], "evt3", t_prev=prev)
        if i1 > i0:
            prev = int(t[i1 - 1])
        steps.append((np.stack([x[i0:i1], y[i0:i1]], -1).astype(np.int16), t[i0:i1] + T0, p[i0:i1].astype(np.int8), words))
    return steps


class Leg:
    def __init__(self, model, kind, window_us, max_decoded=None, **noise):
        self.kind = kind
        kw = dict(decode="evt3", max_decoded=max_decoded, t_base=T0) if kind == "words" else {}
        self.stream = EventStream(model, window_us=window_us, **kw, **noise)
        self.host = dict(high=0, low=0, loops=0, y=0, base=0, pol=0)

    def step(self, k, s, step_us):
        t_now = T0 + (k + 1) * step_us
        if self.kind == "words":
            return self.stream.step_words(s[3], t_now=t_now)
        if self.kind == "host":
            return self.stream.step(*host_decode_evt3(s[3], self.host), t_now=t_now)
        return self.stream.step(s[0], s[1], s[2], t_now=t_now)


def run_block(leg, steps, k0, n, step_us):
    out = np.empty(n)
    for j in range(n):
        c0 = time.perf_counter()
        leg.step(k0 + j, steps[k0 + j], step_us)
        out[j] = time.perf_counter() - c0
    return out * 1e3


def legs_for(model, window_us, tight):
    return {"step": Leg(model, "events", window_us), "host+step": Leg(model, "host", window_us),
            "words": Leg(model, "words", window_us), "words tight": Leg(model, "words", window_us, max_decoded=tight),
            "step, filter": Leg(model, "events", window_us, **NOISE), "words, filter": Leg(model, "words", window_us, **NOISE),
            "words tight, filter": Leg(model, "words", window_us, max_decoded=tight, **NOISE)}


def measure(model, events_per_step, step_us, window_us, block, repeats):
    warm = window_us // step_us + 8
    steps = make_steps(events_per_step, step_us, warm + repeats * block)
    tight = 2 * max(len(s[1]) for s in steps)
    check = DecodeDefinition(1, "evt3", W, H, t_base=T0)
    host = dict(high=0, low=0, loops=0, y=0, base=0, pol=0)
    for s in steps[:60]:                                       # the words are the events, for both decoders
        x, y, t, p, _ = check.push(s[3])
        hxy, ht, hp = host_decode_evt3(s[3], host)
        assert np.array_equal(np.stack([x, y], -1), s[0]) and np.array_equal(t, s[1]) and np.array_equal(p, s[2])
        assert np.array_equal(hxy, s[0]) and np.array_equal(ht, s[1]) and np.array_equal(hp, s[2])
    with torch.no_grad():
        legs = legs_for(model, window_us, tight)
        for leg in legs.values():
            run_block(leg, steps, 0, warm, step_us)
        p50 = {k: [] for k in legs}
        order = list(legs)
        for r in range(repeats):
            for name in order[r % len(order):] + order[:r % len(order)]:
                p50[name].append(float(np.median(run_block(legs[name], steps, warm + r * block, block, step_us))))
        counts = {k: int(leg.stream.counts().sum()) for k, leg in legs.items()}
        for leg in legs.values():
            leg.stream.check_status()
    assert counts["step"] == counts["host+step"] == counts["words"] == counts["words tight"], counts
    assert counts["step, filter"] == counts["words, filter"] == counts["words tight, filter"], counts
    n_ev = np.array([len(s[1]) for s in steps[warm:]])
    n_w = np.array([len(s[3]) for s in steps[warm:]])
    return dict(resident=counts["step"], resident_filter=counts["step, filter"], events=float(n_ev.mean()),
                n_words=float(n_w.mean()), bytes_events=float(17 * n_ev.mean() + 8), bytes_words=float(2 * n_w.mean() + 16),
                tight=tight, **{k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in p50.items()})


def trace(model, events_per_step, step_us, window_us, n=12):
    warm = window_us // step_us
    steps = make_steps(events_per_step, step_us, warm + n)
    with torch.no_grad():
        run_block(Leg(model, "words", window_us, max_decoded=2 * max(len(s[1]) for s in steps)), steps, 0, warm + n, step_us)
    torch.cuda.synchronize()


def build(width, height):
    args = model_args("dagr-s", batch_size=1)
    model = randomize_(DAGR(args, height=height, width=width), seed=0).eval().cuda()
    model.cache_luts(width=width, height=height, radius=args.radius)
    model.check_device_status = False                     # no status read-back inside the timed call
    return model


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events_per_step", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--step_us", type=int, default=1000)
    ap.add_argument("--window_us", type=int, default=50000)
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    model = build(W, H)
    if a.trace:
        trace(model, a.events_per_step[-1], a.step_us, a.window_us)
        return
    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"                                    # noqa: E731
    names = ["step", "host+step", "words", "words tight", "step, filter", "words, filter", "words tight, filter"]
    lines = [f"`python tools/stream_decode_probe.py --commit {a.commit}` on {torch.cuda.get_device_name(0)}: B = 1, "
             f"{W}x{H}, dagr-s events-only, random weights, {a.step_us} us steps on a {a.window_us} us window, S-edges "
             f"encoded as EVT 3.0.  Host clock around the call that ends in the detections' read-back, host inputs; the "
             f"legs in one process, warmed until captured, alternating blocks of {a.block} steps, {a.repeats} blocks each.  "
             "ms per step: median of the blocks' p50 (min .. max of the blocks' p50).", "",
             "| events per step | words per step | resident (filter on) | bytes up: events / words | tight max_decoded | "
             + " | ".join(names) + " |", "|" + "---|" * (5 + len(names))]
    for rate in a.events_per_step:
        r = measure(model, rate, a.step_us, a.window_us, a.block, a.repeats)
        lines.append(f"| {r['events']:.0f} | {r['n_words']:.0f} | {r['resident']} ({r['resident_filter']}) | "
                     f"{r['bytes_events']:.0f} / {r['bytes_words']:.0f} | {r['tight']} | "
                     + " | ".join(cell(r[k]) for k in names) + " |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
