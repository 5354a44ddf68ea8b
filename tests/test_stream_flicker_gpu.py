"""The event stream's anti-flicker and trail filters on the GPU: dagr_stream_flicker through the binding against the numpy
definition (dagr_amd/streaming.py: flicker_definition) push by push over every case of tests/stream_flicker_cases.py;
EventStream(flicker=, trail_us=) against reset=True evaluations of StreamDefinition's window on the same engine -- alone,
in front of the noise filter, of downsample=, under max_lane_events= and behind decode="evt3" --; the absence of host waits;
and the library calls of streams with and without the filter."""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.data.evt import encode_events
from dagr_amd.engine import flicker_map_bytes, flicker_maps_from_state
from dagr_amd.streaming import DecodeDefinition, EventStream, StreamDefinition, flicker_periods, flicker_state, _flicker_options
from dagr_amd.utils import synthetic as syn
from tests import stream_flicker_cases as fc
from tests.test_stream_denoise_gpu import STEP_ENTRIES, _dense, _record_stream_calls
from tests.test_streaming_gpu import _assert_same_detections, _dev, _model

pytestmark = pytest.mark.gpu

W, H, B = 320, 215, 3
TW = 1000000
WINDOW_US = 20000
T_BASE = 1 << 33
BAD = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]


# ------------------------------------------------------------------------------------------------ the kernel, case by case
class _Flicker:
    """dagr_stream_flicker on a state of its own; the outputs start out as garbage."""

    def __init__(self, B_, W_, H_, max_push):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.W, self.H, self.max_push = B_, W_, H_, max_push
        nbytes = self.L.dagr_stream_flicker_bytes(B_, W_, H_, max_push)
        assert nbytes > flicker_map_bytes(B_, W_, H_)
        self.state = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        self.reset()
        self.xy = torch.full((max_push, 2), 77, dtype=torch.int16, device=self.dev)
        self.t = torch.full((max_push,), 77, dtype=torch.int64, device=self.dev)
        self.p = torch.full((max_push,), 77, dtype=torch.int8, device=self.dev)
        self.batch = torch.full((max_push,), 77, dtype=torch.int32, device=self.dev)
        self.n = torch.full((1,), -1, dtype=torch.int32, device=self.dev)
        self.removed = torch.zeros((2, B_), dtype=torch.int64, device=self.dev)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.dev)

    def reset(self):
        _lib.check(self.L.dagr_stream_flicker_reset(_lib.ptr(self.state), self.state.numel(), self.B, self.W, self.H,
                                                    self.max_push, _lib.cur_stream(self.dev)), "flicker_reset")

    def push(self, s, flicker, trail_us, batch_dtype=np.int64, rule=None, **over):
        P = _lib.ptr
        if rule is None:
            opt, trail_us = _flicker_options(flicker, trail_us, self.B, self.W, self.H, "test")
            rule = ((0, 0, 0, 0, 0) if opt is None else
                    (*flicker_periods(opt), opt["start"], opt["stop"], opt["max_count"])) + (trail_us or 0,)
        xy = _dev(np.stack([s["x"], s["y"]], -1).astype(np.int16).reshape(-1, 2))
        t, p, batch = _dev(s["t"]), _dev(s["p"]), _dev(s["batch"].astype(batch_dtype))
        a = dict(state=P(self.state), nbytes=self.state.numel(), B=self.B, max_push=self.max_push, n=len(s["t"]), n_out=P(self.n))
        a.update(over)
        return self.L.dagr_stream_flicker(a["state"], a["nbytes"], a["B"], a["max_push"], self.W, self.H, *rule, P(xy), P(t), P(p),
                                          P(batch), 1 if batch_dtype == np.int64 else 0, a["n"], P(self.xy), P(self.t),
                                          P(self.p), P(self.batch), a["n_out"], P(self.removed[0]), P(self.removed[1]),
                                          P(self.status), _lib.cur_stream(self.dev))

    def maps(self):
        return flicker_maps_from_state(self.state, self.B, self.W, self.H)


def _same_maps(got, want):
    return all(got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in want) and set(got) == set(want)


def _run_case(case, batch_dtype=np.int64):
    max_push = max(max(len(s["t"]) for s in case["pushes"]) + 3, 5)
    fl = _Flicker(case["B"], case["W"], case["H"], max_push)
    assert _same_maps(fl.maps(), flicker_state(case["B"], case["W"], case["H"]))
    high = 0
    for k, (s, (out, maps, removed, status)) in enumerate(zip(case["pushes"], fc.reference(case))):
        where = (case["name"], k)
        if case["expect"] is not None:
            assert out.tolist() == case["expect"][k].tolist(), where
        _lib.check(fl.push(s, case["flicker"], case["trail_us"], batch_dtype), "stream_flicker")
        keep = out == 0
        n_raw, n = len(s["t"]), int(keep.sum())
        assert int(fl.n) == n, where
        assert np.array_equal(fl.xy[:n].cpu().numpy(), np.stack([s["x"], s["y"]], -1)[keep].reshape(-1, 2)), where
        assert np.array_equal(fl.t[:n].cpu().numpy(), s["t"][keep]), where
        assert np.array_equal(fl.p[:n].cpu().numpy(), s["p"][keep]), where
        assert np.array_equal(fl.batch[:n].cpu().numpy(), s["batch"][keep].astype(np.int32)), where
        assert np.all(fl.batch[n:n_raw].cpu().numpy() == -1) and not fl.xy[n:n_raw].any(), where     # lane-less rows
        high = max(high, n_raw)
        assert np.all(fl.batch[high:].cpu().numpy() == 77) and np.all(fl.t[high:].cpu().numpy() == 77), where   # nothing past a push
        assert _same_maps(fl.maps(), maps), where
        got = fl.removed.cpu().numpy()
        assert np.array_equal(got[0], removed[0]) and np.array_equal(got[1], removed[1]), where
        assert int(fl.status) == status, where
        fl.status.zero_()
    return fl


@pytest.mark.parametrize("name", [c["name"] for c in fc.cases()])
def test_flicker_equals_the_definition_after_every_push(name):
    """Bit-equal after every push: the survivors (xy, t, p, lane, count) in push order, the lane-less rows, nothing past the
    push, the state maps read back, both counters and the status word."""
    _run_case(fc.case(name))


@pytest.mark.parametrize("name", ["not-of-this-sensor", "three-lanes", "random-seed0-whole"])
def test_int32_lanes(name):
    _run_case(fc.case(name), batch_dtype=np.int32)


def test_reset_and_refusals():
    case = fc.case("random-seed0-whole")
    fl = _run_case(case)
    fresh = flicker_state(fl.B, fl.W, fl.H)
    assert not _same_maps(fl.maps(), fresh)
    fl.reset()
    assert _same_maps(fl.maps(), fresh)
    fl.removed.zero_()
    s = case["pushes"][0]
    before, n_before, L = fl.state.clone(), int(fl.n), fl.L
    ok = (2000, 20000, 4, 1, 7, 1000)

    def rule(**kw):
        names = ("lo", "hi", "start", "stop", "top", "trail")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))
    assert fl.push(s, None, None, rule=rule(hi=0, trail=0)) == BAD and b"both off" in L.dagr_last_error()
    for r in (rule(trail=-1), rule(hi=-1), rule(lo=0), rule(lo=20001), rule(hi=1000001), rule(stop=4), rule(stop=-1),
              rule(start=8), rule(top=256)):
        assert fl.push(s, None, None, rule=r) == BAD, r
    big = {k: np.concatenate([v] * 2) for k, v in s.items()}
    assert len(big["t"]) > fl.max_push and fl.push(big, True, 1000) == BAD and b"max_push" in L.dagr_last_error()
    assert fl.push(s, True, 1000, n=-1) == BAD
    assert fl.push(s, True, 1000, state=None) == BAD and b"NULL" in L.dagr_last_error()
    assert fl.push(s, True, 1000, n_out=None) == BAD and b"NULL" in L.dagr_last_error()
    assert fl.push(s, True, 1000, nbytes=flicker_map_bytes(fl.B, fl.W, fl.H)) == BAD
    assert b"dagr_stream_flicker_bytes" in L.dagr_last_error()
    assert fl.push(s, True, 1000, B=128) == BAD and fl.push(s, True, 1000, max_push=0) == BAD
    torch.cuda.synchronize()
    assert torch.equal(fl.state, before) and int(fl.status) == 0 and int(fl.n) == n_before and not fl.removed.any()
    assert np.all(fl.batch[len(s["t"]):].cpu().numpy() == 77)
    # the stages one at a time on the same push: the other stage's fields stay initial
    _lib.check(fl.push(s, True, None), "stream_flicker")
    maps = fl.maps()
    assert _same_maps({k: maps[k] for k in ("t_pass", "p_pass")}, {k: fresh[k] for k in ("t_pass", "p_pass")})
    assert maps["blocking"].any() and int(fl.removed[0].sum()) > 0 and int(fl.removed[1].sum()) == 0


# ------------------------------------------------------------------------------------------------ the stream
_SEQS = {}
STEPS, STEP_US = 8, 10000


def _sequence(w, h):
    """Eight pushes of 10 ms on a ``w x h`` sensor, B = 3, times relative to T_BASE: per lane moving edges with spatial
    support (tests/test_stream_denoise_gpu.py: _dense), which trail, and 80 pixels lit at 250 / 100 Hz, which are blocked
    from 24 / 60 ms on; lane 1 misses a push, three pushes carry t_now."""
    if (w, h) not in _SEQS:
        rng = np.random.Generator(np.random.PCG64(77))
        lights = []
        for b in range(B):
            flat = rng.choice(w * h, 80, replace=False)
            hz = np.where(np.arange(80) % 4 == 3, 100, 250)
            lights.append(syn.flicker_events(np.stack([flat % w, flat // w], -1), hz, STEPS * STEP_US, seed=300 + b, t0=1000))
        seq = []
        for k in range(STEPS):
            lo, hi = 1000 + k * STEP_US, 1000 + (k + 1) * STEP_US
            parts = {}
            for b in range(B):
                if (k, b) == (3, 1):
                    continue
                m = (lights[b][2] >= lo) & (lights[b][2] < hi)
                parts[b] = fc._merge(tuple(v[m] for v in lights[b]),
                                     _dense(syn.edges_window, 110 if w == W else 500, 400 + 3 * k + b, lo, hi - 3, w, h))
            lanes = sorted(parts)
            s = {key: np.concatenate([parts[b][i] for b in lanes]) for i, key in enumerate("xytp")}
            s["batch"] = np.concatenate([np.full(len(parts[b][2]), b, np.int64) for b in lanes])
            s["t_now"] = np.full(B, hi + (500 if k == 5 else 0), np.int64) if k in (2, 3, 5) else None
            seq.append(s)
        _SEQS[(w, h)] = seq
    return _SEQS[(w, h)]


FILTER = dict(flicker=True, trail_us=1000)
CONFIGS = {"alone": dict(), "denoise": dict(denoise_us=2000, refractory_us=1), "downsample": dict(downsample=2),
           "capped": dict(max_lane_events=300), "evt3": dict(decode="evt3"),
           "evt3-all": dict(decode="evt3", downsample=2, denoise_us=2000, refractory_us=1, max_lane_events=15)}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_flicker_stream_equals_reset_true_on_the_definitions_window(config):
    """Every step's detections and outputs equal the engine's on StreamDefinition's window, bit for bit; counts(),
    suppressed(), filtered(), dropped() and flicker_state() equal the definition's; after reset() the replay gives the same
    again.  A decoding stream takes the project's encoder's words of the same events."""
    kw = dict(CONFIGS[config])
    fmt = kw.pop("decode", None)
    model = _model(B)
    eng = model.engine().set_low_latency(True)
    w, h = (2 * W, 2 * H) if "downsample" in kw else (W, H)
    stream = EventStream(model, window_us=WINDOW_US, **kw, **FILTER, **(dict(decode=fmt, t_base=T_BASE) if fmt else {}))
    seq = _sequence(w, h)
    total = 0
    with torch.no_grad():
        for rnd in range(2):
            d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, **kw, **FILTER)
            dec, last = DecodeDefinition(B, fmt, w, h, t_base=T_BASE) if fmt else None, [None] * B
            for k, s in enumerate(seq):
                t_now = None if s["t_now"] is None else s["t_now"] + T_BASE
                if fmt:
                    words, lane_words = [], []
                    for b in range(B):
                        m = s["batch"] == b
                        words.append(encode_events(s["x"][m], s["y"][m], s["t"][m], s["p"][m], fmt, t_prev=last[b]))
                        lane_words.append(len(words[-1]))
                        if m.any():
                            last[b] = int(s["t"][m][-1])
                    words = np.concatenate(words)
                    x, y, t, p, batch = dec.push(words, lane_words)
                    assert np.array_equal(t, s["t"] + T_BASE) and np.array_equal(x, s["x"]), "the decoder changed the events"
                    d.push(x, y, t, p, batch, t_now=t_now)
                    det, nk = stream.step_words_device(words, lane_words, t_now=t_now)
                else:
                    d.push(s["x"], s["y"], s["t"] + T_BASE, s["p"], s["batch"], t_now=t_now)
                    det, nk = stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"] + T_BASE, s["p"], batch=s["batch"],
                                                 t_now=t_now)
                got, out = (det.clone(), nk.clone()), stream.outputs.clone()
                window = tuple(_dev(v) for v in d.formatted())
                _assert_same_detections(got, eng.forward_detections(*window), B, (rnd, k))
                assert torch.equal(out, eng.forward_raw(*window)), (rnd, k)
                total += int(got[1].sum())
                if k in (0, 3, 7):
                    assert stream.counts().tolist() == d.counts().tolist(), (rnd, k)
                    assert all(np.array_equal(u, v) for u, v in zip(stream.suppressed(), d.suppressed)), (rnd, k)
                    assert np.array_equal(stream.filtered(), d.filtered) and np.array_equal(stream.dropped(), d.dropped), (rnd, k)
            assert _same_maps(stream.flicker_state(), d.flicker_state), rnd
            stream.check_status()
            assert d.suppressed[0].min() > 0 and d.suppressed[1].min() > 0 and d.counts().sum() > 0
            if "denoise_us" in kw:
                assert d.filtered.min() > 0
            if "max_lane_events" in kw:
                assert d.dropped.sum() > 0
            stream.reset()
            assert not any(v.any() for v in stream.suppressed()) and _same_maps(stream.flicker_state(), flicker_state(B, w, h))
    assert total > 0, "no step kept a detection: the comparison is empty"


def test_a_flicker_step_on_device_inputs_waits_for_nothing():
    """torch's sync debug mode turns every host synchronisation torch makes into an error: first the probe of
    tests/test_stream_denoise_gpu.py that it does so on this build (an .item()), then step_device on device-resident raw
    events under it, with every front in the chain."""
    probe = torch.ones((1,), device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    model = _model(B)
    model.engine().set_low_latency(True)
    kw = dict(downsample=2, denoise_us=2000, refractory_us=1)
    stream = EventStream(model, window_us=WINDOW_US, **kw, **FILTER)
    seq = _sequence(2 * W, 2 * H)[:6]
    pushes = [(_dev(np.stack([s["x"], s["y"]], -1)), _dev(s["t"] + T_BASE), _dev(s["p"]), _dev(s["batch"].astype(np.int32)))
              for s in seq]
    with torch.no_grad():
        for xy, t, p, batch in pushes[:4]:                 # two eager steps, the capture, one replay
            stream.step_device(xy, t, p, batch=batch)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for xy, t, p, batch in pushes[4:]:
                stream.step_device(xy, t, p, batch=batch)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, **kw, **FILTER)
    for s in seq:
        d.push(s["x"], s["y"], s["t"] + T_BASE, s["p"], s["batch"])
    assert stream.counts().tolist() == d.counts().tolist() and sum(d.counts()) > 0
    assert all(np.array_equal(u, v) and v.sum() > 0 for u, v in zip(stream.suppressed(), d.suppressed))
    stream.check_status()


def test_event_stream_refuses_bad_options_by_name():
    model = _model(B)
    for kw, name in ((dict(flicker=5), "flicker"), (dict(flicker=dict(hz=100)), "hz"), (dict(flicker=dict(min_hz=0)), "min_hz"),
                     (dict(flicker=dict(start=1)), "start"), (dict(trail_us=0), "trail_us"), (dict(trail_us=2.5), "trail_us")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)
    with pytest.raises(ValueError, match="W_in \\* H_in"):
        EventStream(model, window_us=WINDOW_US, downsample=2, sensor_size=(32000, 30000), trail_us=5)
    stream = EventStream(model, window_us=WINDOW_US, trail_us=np.int64(5))
    assert stream.state.flick == (W, H, 0, 0, 0, 0, 0, 5) and stream.flicker_state()["t_pass"].shape == (B, H, W)
    assert _same_maps(stream.flicker_state(), flicker_state(B, W, H)) and not any(v.any() for v in stream.suppressed())
    assert EventStream(model, window_us=WINDOW_US, flicker=dict(max_hz=130)).state.flick == (W, H, 7693, 20000, 4, 1, 7, 0)


FLICKER_STEP_ENTRIES = STEP_ENTRIES + ("dagr_stream_flicker", "dagr_stream_decode", "dagr_stream_stage_dev_clock",
                                       "dagr_stream_stage_dev_clock_capped")


@pytest.mark.parametrize("config", ["plain", "downsample", "denoise"])
def test_a_stream_without_the_options_calls_what_it_called_before(config, monkeypatch):
    """Without flicker / trail_us: no flicker state, no dagr_stream_flicker* call at all, and per step the entries the
    stream had before the filter existed.  With them: the filter in front, and the _dev staging behind it."""
    kw = {"plain": dict(), "downsample": dict(downsample=2), "denoise": dict(denoise_us=2000, refractory_us=1)}[config]
    model = _model(B)
    model.engine().set_low_latency(True)
    seq = _sequence(*((2 * W, 2 * H) if "downsample" in kw else (W, H)))[:3]
    calls = _record_stream_calls(monkeypatch)
    steps = {"plain": ["dagr_stream_stage"], "downsample": ["dagr_stream_downsample", "dagr_stream_stage_dev"],
             "denoise": ["dagr_stream_denoise", "dagr_stream_stage_dev"]}[config]

    def play(stream):
        del calls[:]
        with torch.no_grad():
            for s in seq:
                stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"] + T_BASE, s["p"], batch=s["batch"])
        return [c for c in calls if c in FLICKER_STEP_ENTRIES]
    for off in (dict(), dict(flicker=None, trail_us=None)):
        del calls[:]
        stream = EventStream(model, window_us=WINDOW_US, **kw, **off)
        st = stream.state
        assert st.flick is None and "flick" not in st.stages and st.lane_suppressed is None
        assert play(stream) == steps * len(seq), calls
        assert not any(v.any() for v in stream.suppressed())
        assert not any("flicker" in c for c in calls)
        with pytest.raises(RuntimeError, match="no per-pixel state"):
            stream.flicker_state()
    behind = ["dagr_stream_flicker"] + steps[:-1] + ["dagr_stream_stage_dev"]
    assert play(EventStream(model, window_us=WINDOW_US, **kw, **FILTER)) == behind * len(seq), calls
    torch.cuda.synchronize()


def test_run_stream_script_filters_and_prints_the_two_counters(tmp_path, capsys):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import _common as C
    import run_stream as R
    model = _model(1)
    argv = ["--step_us", "1000", "--window_us", "5000", "--steps", "60", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "100000", "--output_directory", str(tmp_path), "--sequence", "lit",
            "--flicker_pixels", "300", "--flicker_pixel_hz", "250", "--flicker_hz", "50", "500", "--trail_us", "1000"]
    source = R.SyntheticStream(C.flags("", argv, extra=R.stream_options))
    R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    stream = EventStream(model, window_us=5000, flicker=dict(min_hz=50, max_hz=500), trail_us=1000)
    t0, t1 = source.t_range()
    with torch.no_grad():
        for t_step in range(t0 + 1000, t1 + 1, 1000):
            ev = source.events(t_step - 1000, t_step)
            stream.step_device(np.stack([ev["x"], ev["y"]], -1), ev["t"], ev["p"], t_now=t_step)
    flicker, trail = (int(v.sum()) for v in stream.suppressed())
    assert flicker > 0 and trail > 0
    assert f"behind the flicker / trail filters ({flicker} flicker events, {trail} trail events suppressed)" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="--flicker_hz"):
        R.main(argv[:-4] + ["500", "50"])
    with pytest.raises(SystemExit, match="--trail_us"):
        R.main(argv[:-1] + ["0"])
