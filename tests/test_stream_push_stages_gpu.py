"""The stages a push of an event stream passes through -- the word decoder, the flicker / trail filters, the noise filter
and the downsampling front -- as a chain: every subset of the four, capped and not, calls the library entries the chain
rule names and equals StreamDefinition push by push; and a push that outgrows a stage's scratch carries the stage's maps
(stamp maps, flicker maps, decoder states) into the larger state."""
import copy

import numpy as np
import pytest
import torch

from dagr_amd.data.evt import encode_events
from dagr_amd.streaming import (DecodeDefinition, EventStream, StreamDefinition, denoise_definition, flicker_definition,
                                flicker_state)
from dagr_amd.utils import synthetic as syn
from tests import stream_flicker_cases as fc
from tests.test_stream_denoise_gpu import _dense, _record_stream_calls
from tests.test_stream_flicker_gpu import FLICKER_STEP_ENTRIES, STEP_US, T_BASE, TW, WINDOW_US, _same_maps
from tests.test_stream_flicker_gpu import _sequence as _flicker_sequence
from tests.test_streaming_gpu import H, W, _assert_same_detections, _dev, _model

pytestmark = pytest.mark.gpu

FLICKER = dict(flicker=True, trail_us=1000)
NOISE = dict(denoise_us=2000, refractory_us=1)


class _Words:
    """The project's encoder's words of a sequence's pushes, lane by lane, and the decoder's definition of them."""

    def __init__(self, B, fmt, w, h):
        self.B, self.fmt, self.last = B, fmt, [None] * B
        self.dec = DecodeDefinition(B, fmt, w, h, t_base=T_BASE)

    def encode(self, s):
        words, lane_words = [], []
        for b in range(self.B):
            m = s["batch"] == b
            words.append(encode_events(s["x"][m], s["y"][m], s["t"][m], s["p"][m], self.fmt, t_prev=self.last[b]))
            lane_words.append(len(words[-1]))
            if m.any():
                self.last[b] = int(s["t"][m][-1])
        return np.concatenate(words), lane_words


def _step(stream, d, words, s):
    """One push into the stream and into its definition ``d`` (through ``words``, a ``_Words``, if the stream decodes);
    returns the step's ``(det, n_keep)``."""
    t_now = None if s["t_now"] is None else s["t_now"] + T_BASE
    if words is None:
        d.push(s["x"], s["y"], s["t"] + T_BASE, s["p"], s["batch"], t_now=t_now)
        return stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"] + T_BASE, s["p"], batch=s["batch"], t_now=t_now)
    w, lane_words = words.encode(s)
    x, y, t, p, batch = words.dec.push(w, lane_words)
    assert np.array_equal(t, s["t"] + T_BASE) and np.array_equal(x, s["x"]), "the decoder changed the events"
    d.push(x, y, t, p, batch, t_now=t_now)
    return stream.step_words_device(w, lane_words, t_now=t_now)


def _assert_window(stream, d, eng, det, lanes, where):
    """The step's detections and outputs equal the engine's on the definition's window, bit for bit."""
    got, out = (det[0].clone(), det[1].clone()), stream.outputs.clone()
    window = tuple(_dev(v) for v in d.formatted())
    _assert_same_detections(got, eng.forward_detections(*window), lanes, where)
    assert torch.equal(out, eng.forward_raw(*window)), where
    return int(got[1].sum())


def _assert_counters(stream, d, where):
    assert stream.counts().tolist() == d.counts().tolist(), where
    assert np.array_equal(stream.filtered(), d.filtered) and np.array_equal(stream.dropped(), d.dropped), where
    assert all(np.array_equal(u, v) for u, v in zip(stream.suppressed(), d.suppressed)), where


# ------------------------------------------------------------------------------------------------ growth carries the state
GROW_B, BIG = 2, 4


def _growth_sequence():
    """Six pushes of 10 ms, B = 2, on the model's own sensor, as tests/test_stream_flicker_gpu.py's: moving edges with spatial
    support and 30 lit pixels per lane, which are blocked from 24 / 60 ms on.  Pushes 0..3 and 5 hold some hundred events
    a lane, push 4 (``BIG``) more than 4096 in all: it outgrows the scratch a stage starts with.  It opens with an echo of
    the last millisecond of push 3, one pixel to the right: events whose only support are stamps of the push before."""
    rng = np.random.Generator(np.random.PCG64(78))
    lights = []
    for b in range(GROW_B):
        flat = rng.choice(W * H, 30, replace=False)
        hz = np.where(np.arange(30) % 4 == 3, 100, 250)
        lights.append(syn.flicker_events(np.stack([flat % W, flat // W], -1), hz, 6 * STEP_US, seed=310 + b, t0=1000))
    seq, parts = [], None
    for k in range(6):
        lo, hi = 1000 + k * STEP_US, 1000 + (k + 1) * STEP_US
        before, parts = parts, []
        for b in range(GROW_B):
            m = (lights[b][2] >= lo) & (lights[b][2] < hi)
            sources = [tuple(v[m] for v in lights[b]),
                       _dense(syn.edges_window, 600 if k == BIG else 80, 500 + 3 * k + b, lo, hi - 3, W, H)]
            if k == BIG:
                x, y, t, _ = before[b]
                m = (t >= lo - 1000) & (x + 1 < W)
                sources.append((x[m] + 1, y[m], np.full(int(m.sum()), lo), np.ones(int(m.sum()), np.int64)))
            parts.append(fc._merge(*sources))
        s = {key: np.concatenate([part[i] for part in parts]) for i, key in enumerate("xytp")}
        s["batch"] = np.concatenate([np.full(len(part[2]), b, np.int64) for b, part in enumerate(parts)])
        s["t_now"] = None
        seq.append(s)
    return seq


@pytest.mark.parametrize("fmt", [None, "evt3"], ids=["events", "evt3"])
def test_a_push_that_outgrows_the_scratch_carries_the_stages_state(fmt, monkeypatch):
    """Flicker / trail and noise filters, B = 2; with ``evt3`` behind the decoder.  The large push makes the filter states
    (the decoder's state, with ``evt3``) grow -- their ``_reset`` entries are called during that step -- and after it and
    after the small push behind it the stamp maps, the flicker maps, the decoder's state and counters, the stream's
    counters and the detections equal the definitions'.  The large push must see the carried state: replayed on the CPU
    through a definition whose flicker maps (stamp maps, decoder state) were reset just before it, it keeps (decodes)
    something else -- so a growth that lost the maps could not pass."""
    kw = dict(**FLICKER, **NOISE)
    seq = _growth_sequence()
    model = _model(GROW_B)
    eng = model.engine().set_low_latency(True)
    calls = _record_stream_calls(monkeypatch)
    stream = EventStream(model, window_us=WINDOW_US, **kw, **(dict(decode=fmt, t_base=T_BASE) if fmt else {}))
    d = StreamDefinition(GROW_B, W, H, time_window=TW, window_us=WINDOW_US, **kw)
    words = _Words(GROW_B, fmt, W, H) if fmt else None
    total = 0
    with torch.no_grad():
        for k, s in enumerate(seq):
            if k == BIG:            # the condition, on the definitions alone
                assert len(s["t"]) > 4096
                x, y, p = s["x"].astype(np.int16), s["y"].astype(np.int16), s["p"].astype(np.int8)
                t, batch = s["t"] + T_BASE, s["batch"]
                carried = flicker_definition(copy.deepcopy(d.flicker_state), x, y, t, p, batch, d.flicker, d.trail_us)
                fresh = flicker_definition(flicker_state(GROW_B, W, H), x, y, t, p, batch, d.flicker, d.trail_us)
                assert not np.array_equal(carried, fresh), "the large push does not depend on the carried flicker maps"
                m = carried == 0
                never = np.full_like(d.last_t, np.iinfo(np.int64).min)
                carried = denoise_definition(d.last_t.copy(), x[m], y[m], t[m], batch[m], d.denoise_us, d.refractory_us)
                fresh = denoise_definition(never, x[m], y[m], t[m], batch[m], d.denoise_us, d.refractory_us)
                assert not np.array_equal(carried, fresh), "the large push does not depend on the carried stamp maps"
                if fmt:
                    probe, again = copy.deepcopy(words), DecodeDefinition(GROW_B, fmt, W, H, t_base=T_BASE)
                    w, lane_words = probe.encode(s)
                    assert len(w) > 4096
                    assert not np.array_equal(probe.dec.push(w, lane_words)[2], again.push(w, lane_words)[2]), \
                        "the large push does not depend on the carried decoder state"
                del calls[:]
            det = _step(stream, d, words, s)
            if k == BIG:
                grown = ["dagr_stream_decode_reset"] if fmt else ["dagr_stream_flicker_reset", "dagr_stream_denoise_reset"]
                assert all(name in calls for name in grown), calls
            total += _assert_window(stream, d, eng, det, GROW_B, k)
            if k >= BIG:
                _assert_counters(stream, d, k)
                assert np.array_equal(stream.last_stamps(), d.last_t), k
                assert _same_maps(stream.flicker_state(), d.flicker_state), k
                if fmt:
                    assert all(np.array_equal(v, words.dec.state[name]) for name, v in stream.decode_state().items()), k
                    assert all(np.array_equal(v, words.dec.counts[name]) for name, v in stream.decode_counts().items()), k
    stream.check_status()
    assert d.filtered.min() > 0 and min(v.min() for v in d.suppressed) > 0 and d.counts().sum() > 0
    assert total > 0, "no step kept a detection: the comparison is empty"


# ------------------------------------------------------------------------------------------------ every chain
B = 3
STAGES = ("decode", "flicker", "denoise", "downsample")
OPTIONS = dict(decode=dict(decode="evt3"), flicker=FLICKER, denoise=NOISE, downsample=dict(downsample=2))
CHAINS = [tuple(name for i, name in enumerate(STAGES) if mask >> i & 1) for mask in range(16)]
CAP = 15


class _CountingDefinition(StreamDefinition):
    """StreamDefinition, which also counts what its front removes."""
    front_removed = 0

    def _downsample(self, x, y, t, p, batch):
        out = super()._downsample(x, y, t, p, batch)
        self.front_removed += len(t) - len(out[2])
        return out


def _entries(chain, capped):
    """The chain rule: the enabled stages in the order decoder, flicker, noise, front, then one staging entry --
    ``_dev_clock`` behind the decoder, ``_dev`` behind any other stage, the plain one with none; ``_capped`` with a cap."""
    stage = {"decode": "dagr_stream_decode", "flicker": "dagr_stream_flicker", "denoise": "dagr_stream_denoise",
             "downsample": "dagr_stream_downsample"}
    last = "dagr_stream_stage" + ("_dev_clock" if "decode" in chain else "_dev" if chain else "") + ("_capped" if capped else "")
    return [stage[name] for name in STAGES if name in chain] + [last]


@pytest.mark.parametrize("capped", [False, True], ids=["uncapped", "capped"])
@pytest.mark.parametrize("chain", CHAINS, ids=["+".join(c) or "plain" for c in CHAINS])
def test_every_chain_calls_what_the_rule_names_and_equals_the_definition(chain, capped, monkeypatch):
    """All 16 subsets of the four stages, without a cap and with one that drops events, over the first four pushes of
    tests/test_stream_flicker_gpu.py's sequence (push 3 lacks lane 1).  Per push: the step entries are ``_entries``'s, and
    counts(), filtered(), suppressed(), dropped(), the detections and the outputs equal StreamDefinition's.  By the last
    push every enabled stage has removed (the decoder: decoded) at least one event, and a cap has dropped one."""
    kw = {k: v for name in chain if name != "decode" for k, v in OPTIONS[name].items()}
    if capped:
        kw["max_lane_events"] = CAP
    fmt = "evt3" if "decode" in chain else None
    w, h = (2 * W, 2 * H) if "downsample" in chain else (W, H)
    seq = _flicker_sequence(w, h)[:4]
    model = _model(B)
    eng = model.engine().set_low_latency(True)
    calls = _record_stream_calls(monkeypatch)
    stream = EventStream(model, window_us=WINDOW_US, **kw, **(dict(decode=fmt, t_base=T_BASE) if fmt else {}))
    d = _CountingDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, **kw)
    words = _Words(B, fmt, w, h) if fmt else None
    with torch.no_grad():
        for k, s in enumerate(seq):
            del calls[:]
            det = _step(stream, d, words, s)
            assert [c for c in calls if c in FLICKER_STEP_ENTRIES] == _entries(chain, capped), (k, calls)
            _assert_window(stream, d, eng, det, B, k)
            _assert_counters(stream, d, k)
    stream.check_status()
    assert d.counts().sum() > 0
    bitten = dict(decode=fmt is None or words.dec.counts["decoded"].min() > 0, flicker=min(v.sum() for v in d.suppressed) > 0,
                  denoise=d.filtered.sum() > 0, downsample=d.front_removed > 0)
    assert all(bitten[name] for name in chain), bitten
    assert not capped or d.dropped.sum() > 0
