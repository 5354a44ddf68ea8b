"""The event stream's noise filter on the GPU: dagr_stream_denoise through the binding against the numpy definition
(dagr_amd/streaming.py: denoise_definition) push by push over every case of tests/stream_denoise_cases.py;
EventStream(denoise_us=, refractory_us=) against reset=True evaluations of StreamDefinition's window on the same engine,
with and without downsample= and max_lane_events=; a hot pixel under a cap; the absence of host waits; and the library
calls of streams with and without the filter."""
import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.streaming import NEVER, EventStream, StreamDefinition
from dagr_amd.utils import synthetic as syn
from tests import stream_denoise_cases as dc
from tests.test_streaming_gpu import _assert_same_detections, _dev, _model

pytestmark = pytest.mark.gpu

W, H, B = 320, 215, 3
TW = 1000000
WINDOW_US = 20000
T0 = dc.T0


# ------------------------------------------------------------------------------------------------ the kernel, case by case
class _Denoiser:
    """dagr_stream_denoise on a state of its own; the outputs start out as garbage."""

    def __init__(self, B_, W_, H_, max_push):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.W, self.H, self.max_push = B_, W_, H_, max_push
        nbytes = self.L.dagr_stream_denoise_bytes(B_, W_, H_, max_push)
        assert nbytes > 8 * B_ * W_ * H_
        self.state = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_denoise_reset(_lib.ptr(self.state), nbytes, B_, W_, H_, max_push,
                                                    _lib.cur_stream(self.dev)), "denoise_reset")
        self.xy = torch.full((max_push, 2), 77, dtype=torch.int16, device=self.dev)
        self.t = torch.full((max_push,), 77, dtype=torch.int64, device=self.dev)
        self.p = torch.full((max_push,), 77, dtype=torch.int8, device=self.dev)
        self.batch = torch.full((max_push,), 77, dtype=torch.int32, device=self.dev)
        self.n = torch.full((1,), -1, dtype=torch.int32, device=self.dev)
        self.filtered = torch.zeros((B_,), dtype=torch.int64, device=self.dev)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.dev)

    def push(self, s, D, R, batch_dtype=np.int64):
        P = _lib.ptr
        xy = _dev(np.stack([s["x"], s["y"]], -1).astype(np.int16).reshape(-1, 2))
        t, p, batch = _dev(s["t"]), _dev(s["p"]), _dev(s["batch"].astype(batch_dtype))
        return self.L.dagr_stream_denoise(P(self.state), self.state.numel(), self.B, self.max_push, self.W, self.H, D or 0,
                                          R or 0, P(xy), P(t), P(p), P(batch), 1 if batch_dtype == np.int64 else 0,
                                          len(s["t"]), P(self.xy), P(self.t), P(self.p), P(self.batch), P(self.n),
                                          P(self.filtered), P(self.status), _lib.cur_stream(self.dev))

    def maps(self):
        return self.state[:8 * self.B * self.W * self.H].view(torch.int64).view(self.B, self.H, self.W).cpu().numpy()


def _run_case(case, batch_dtype=np.int64):
    max_push = max(max(len(s["t"]) for s in case["pushes"]) + 3, 5)
    dn = _Denoiser(case["B"], case["W"], case["H"], max_push)
    assert np.all(dn.maps() == NEVER)
    high = 0
    for k, (s, (keep, maps, filtered, status)) in enumerate(zip(case["pushes"], dc.reference(case))):
        where = (case["name"], k)
        if case["expect"] is not None:
            assert keep.tolist() == case["expect"][k].tolist(), where
        _lib.check(dn.push(s, case["D"], case["R"], batch_dtype), "stream_denoise")
        n_raw, n = len(s["t"]), int(keep.sum())
        assert int(dn.n) == n, where
        assert np.array_equal(dn.xy[:n].cpu().numpy(), np.stack([s["x"], s["y"]], -1)[keep].reshape(-1, 2)), where
        assert np.array_equal(dn.t[:n].cpu().numpy(), s["t"][keep]), where
        assert np.array_equal(dn.p[:n].cpu().numpy(), s["p"][keep]), where
        assert np.array_equal(dn.batch[:n].cpu().numpy(), s["batch"][keep].astype(np.int32)), where
        assert np.all(dn.batch[n:n_raw].cpu().numpy() == -1) and not dn.xy[n:n_raw].any(), where     # lane-less rows
        high = max(high, n_raw)
        assert np.all(dn.batch[high:].cpu().numpy() == 77), where                                  # nothing past a push
        assert np.array_equal(dn.maps(), maps), where
        assert np.array_equal(dn.filtered.cpu().numpy(), filtered), where
        assert int(dn.status) == status, where
        dn.status.zero_()
    return dn


@pytest.mark.parametrize("name", [c["name"] for c in dc.cases()])
def test_denoise_equals_the_definition_after_every_push(name):
    """Bit-equal after every push: the survivors (xy, t, p, lane, count) in push order, the stamp maps read back,
    lane_filtered and the status word."""
    _run_case(next(c for c in dc.cases() if c["name"] == name))


def test_int32_lanes_reset_and_refusals():
    case = next(c for c in dc.cases() if c["name"] == "random-8x6-B3-both-outside")
    dn = _run_case(case, batch_dtype=np.int32)
    assert (dn.maps() != NEVER).any()
    _lib.check(dn.L.dagr_stream_denoise_reset(_lib.ptr(dn.state), dn.state.numel(), dn.B, dn.W, dn.H, dn.max_push,
                                              _lib.cur_stream(dn.dev)), "denoise_reset")
    assert np.all(dn.maps() == NEVER)
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    s = case["pushes"][0]
    assert dn.push(s, None, None) == bad and b"both off" in dn.L.dagr_last_error()
    assert dn.push(s, -1, 5) == bad
    big = {k: np.concatenate([v] * 2) for k, v in s.items()}
    assert len(big["t"]) > dn.max_push and dn.push(big, 5, 5) == bad and b"max_push" in dn.L.dagr_last_error()
    assert np.all(dn.maps() == NEVER) and int(dn.status) == 0


# ------------------------------------------------------------------------------------------------ the stream
def _dense(gen, n, seed, t_lo, t_hi, w, h):
    """Events with spatial support on a ``w x h`` sensor: ``n`` base events of ``gen`` on the half-resolution grid, each
    repeated 3 to 6 times at ``(2x + {0,1}, 2y + {0,1}, t + {0,1,2})``, sorted stably by t; T0 + t_lo <= t <= T0 + t_hi + 2."""
    x, y, t, p = gen(n, w // 2, h // 2, seed, window_us=t_hi - t_lo, time_window=t_hi - t_lo)
    rng = np.random.Generator(np.random.PCG64(2000 + seed))
    rep = rng.integers(3, 7, len(t))
    x, y, t, p = (np.repeat(np.asarray(v), rep) for v in (x, y, t, p))
    m = len(t)
    x = x.astype(np.int64) * 2 + rng.integers(0, 2, m)
    y = y.astype(np.int64) * 2 + rng.integers(0, 2, m)
    t = np.int64(t_lo) + t.astype(np.int64) + rng.integers(0, 3, m)
    o = np.argsort(t, kind="stable")
    return x[o], y[o], t[o], p[o]


_SEQS = {}


def _sequence(w, h):
    """Six pushes on a ``w x h`` sensor, B = 3: edges and uniform events (the uniform lane is mostly noise), a lane without
    events, an empty push with t_now, a jump that expires a lane."""
    if (w, h) not in _SEQS:
        E, U = syn.edges_window, syn.uniform_window
        plan = [({0: (E, 500, 0, 6000), 1: (U, 300, 0, 5000), 2: (E, 260, 0, 5500)}, None),
                ({1: (U, 140, 6000, 9000)}, None),
                ({}, [12000] * 3),
                ({0: (E, 410, 12000, 17000), 2: (U, 220, 12500, 16000)}, [18000] * 3),
                ({1: (E, 120, 17000, 17900)}, [45000, 18000, 45000]),
                ({0: (E, 300, 45000, 49000), 1: (U, 30, 18010, 20000), 2: (E, 7, 45500, 46000)}, None)]
        seq = []
        for k, (lanes, t_now) in enumerate(plan):
            s = dc.push({b: _dense(g, n, 50 + 3 * k + b, lo, hi, w, h) for b, (g, n, lo, hi) in lanes.items()})
            s["t_now"] = None if t_now is None else np.asarray(t_now, np.int64) + T0
            seq.append(s)
        _SEQS[(w, h)] = seq
    return _SEQS[(w, h)]


CONFIGS = {"plain": dict(), "downsample": dict(downsample=2), "capped": dict(max_lane_events=300),
           "downsample-capped": dict(downsample=2, max_lane_events=150)}
NOISE = dict(denoise_us=2000, refractory_us=1)


def _definition(kw, noise=NOISE):
    return StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, **kw, **noise)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_filtering_stream_equals_reset_true_on_the_definitions_window(config):
    """Every step's detections and outputs equal the engine's on StreamDefinition's window, bit for bit; counts(),
    filtered(), dropped() and last_stamps() equal the definition's; after reset() the replay gives the same again."""
    kw = CONFIGS[config]
    model = _model(B)
    eng = model.engine().set_low_latency(True)
    stream = EventStream(model, window_us=WINDOW_US, **kw, **NOISE)
    seq = _sequence(*((2 * W, 2 * H) if "downsample" in kw else (W, H)))
    total = 0
    with torch.no_grad():
        for rnd in range(2):
            d = _definition(kw)
            for k, s in enumerate(seq):
                d.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
                det, nk = stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], t_now=s["t_now"])
                got, out = (det.clone(), nk.clone()), stream.outputs.clone()
                window = tuple(_dev(v) for v in d.formatted())
                _assert_same_detections(got, eng.forward_detections(*window), B, (rnd, k))
                assert torch.equal(out, eng.forward_raw(*window)), (rnd, k)
                total += int(got[1].sum())
                if k in (0, 3, 5):
                    assert stream.counts().tolist() == d.counts().tolist(), (rnd, k)
                    assert np.array_equal(stream.filtered(), d.filtered), (rnd, k)
                    assert np.array_equal(stream.dropped(), d.dropped), (rnd, k)
            assert np.array_equal(stream.last_stamps(), d.last_t), rnd
            stream.check_status()
            assert d.filtered.min() > 0 and d.counts().sum() > 0
            if "max_lane_events" in kw:
                assert d.dropped.sum() > 0
            stream.reset()
            assert not stream.filtered().any() and not stream.dropped().any() and np.all(stream.last_stamps() == NEVER)
    assert total > 0, "no step kept a detection: the comparison is empty"


def test_a_hot_pixel_under_a_cap():
    """A pixel firing every 10 us among a few real events, max_lane_events = 200.  Without the filter the hot pixel fills
    the window and `dropped` grows.  With refractory_us = 1000 it passes once and then stays silent -- every event stamps,
    kept or not, so its own stamp is never more than 10 us old -- and nothing is dropped.  Both as the definition has it."""
    N, steps = 200, 4
    model = _model(B)
    eng = model.engine().set_low_latency(True)
    pushes = []
    for k in range(steps):
        x, y, t, p = _dense(syn.edges_window, 8, 90 + k, 2000 * k, 2000 * k + 1900, W, H)
        ht = np.arange(2000 * k, 2000 * (k + 1), 10, dtype=np.int64)
        x, y = np.concatenate([x, np.full(len(ht), 100)]), np.concatenate([y, np.full(len(ht), 50)])
        t, p = np.concatenate([t, ht]), np.concatenate([p, np.ones(len(ht), np.int64)])
        o = np.argsort(t, kind="stable")
        pushes.append(dc.push({0: (x[o], y[o], t[o], p[o])}))
    seen = {}
    for name, noise in (("unfiltered", dict()), ("refractory", dict(refractory_us=1000))):
        stream = EventStream(model, window_us=WINDOW_US, max_lane_events=N, **noise)
        d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, max_lane_events=N, **noise)
        with torch.no_grad():
            for k, s in enumerate(pushes):
                d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
                det, nk = stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"])
                got = (det.clone(), nk.clone())
                _assert_same_detections(got, eng.forward_detections(*(_dev(v) for v in d.formatted())), B, (name, k))
                assert stream.counts().tolist() == d.counts().tolist(), (name, k)
                assert np.array_equal(stream.dropped(), d.dropped) and np.array_equal(stream.filtered(), d.filtered), (name, k)
        stream.check_status()
        w = d.window()
        seen[name] = (int(((w[0] == 100) & (w[1] == 50)).sum()), int(d.dropped[0]), int(d.counts()[0]))
    hot, dropped, count = seen["unfiltered"]
    assert count == N and hot > 0.7 * N and dropped > 2 * N, seen
    hot, dropped, count = seen["refractory"]
    assert hot == 1 and dropped == 0 and hot < count < N, seen


def test_a_filtering_step_on_device_inputs_waits_for_nothing():
    """torch's sync debug mode turns every host synchronisation torch makes into an error: first a probe that it does so
    on this build (an .item()), then step_device on device-resident raw events under it."""
    probe = torch.ones((1,), device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
        caught, why = False, "torch.cuda.set_sync_debug_mode('error') let an .item() pass"
    except RuntimeError as e:
        caught, why = True, str(e)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not caught:
        pytest.skip(why)
    model = _model(B)
    model.engine().set_low_latency(True)
    kw = dict(downsample=2)
    stream = EventStream(model, window_us=WINDOW_US, **kw, **NOISE)
    pushes = []
    for k in range(6):
        s = dc.push({b: _dense(syn.edges_window, 80, 70 + 3 * k + b, 1000 * k, 1000 * k + 900, 2 * W, 2 * H) for b in range(B)})
        pushes.append((_dev(np.stack([s["x"], s["y"]], -1)), _dev(s["t"]), _dev(s["p"]), _dev(s["batch"].astype(np.int32))))
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
    d = _definition(kw)
    for xy, t, p, batch in pushes:
        d.push(xy[:, 0].cpu().numpy(), xy[:, 1].cpu().numpy(), t.cpu().numpy(), p.cpu().numpy(), batch.cpu().numpy())
    assert stream.counts().tolist() == d.counts().tolist() and sum(d.counts()) > 0
    assert np.array_equal(stream.filtered(), d.filtered) and d.filtered.sum() > 0
    stream.check_status()


def test_event_stream_refuses_bad_options_by_name():
    model = _model(B)
    for kw, name in ((dict(denoise_us=0), "denoise_us"), (dict(denoise_us=2.5), "denoise_us"),
                     (dict(refractory_us=-1), "refractory_us"), (dict(refractory_us=True), "refractory_us")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)
    with pytest.raises(ValueError, match="W_in \\* H_in"):
        EventStream(model, window_us=WINDOW_US, downsample=2, sensor_size=(32000, 30000), refractory_us=5)
    stream = EventStream(model, window_us=WINDOW_US, refractory_us=np.int64(5))
    assert stream.state.noise == (W, H, 0, 5) and stream.last_stamps().shape == (B, H, W)
    assert np.all(stream.last_stamps() == NEVER) and not stream.filtered().any()


def test_run_stream_script_filters_and_prints_the_filtered_count(tmp_path, capsys):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import _common as C
    import run_stream as R
    from dagr_amd.utils.buffers import detections_to_records
    model = _model(1)
    argv = ["--step_us", "1000", "--window_us", "5000", "--steps", "6", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "400000", "--output_directory", str(tmp_path), "--sequence", "clean",
            "--denoise_us", "300", "--refractory_us", "50"]
    source = R.SyntheticStream(C.flags("", argv, extra=R.stream_options))
    path = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    rec = np.load(path)
    stream = EventStream(model, window_us=5000, denoise_us=300, refractory_us=50)
    t0, t1 = source.t_range()
    with torch.no_grad():
        for t_step in range(t0 + 1000, t1 + 1, 1000):
            ev = source.events(t_step - 1000, t_step)
            det = stream.step(np.stack([ev["x"], ev["y"]], -1), ev["t"], ev["p"], t_now=t_step)[0]
            want = detections_to_records({k: v.cpu() for k, v in det.items()}, np.uint64(t_step))
            got = rec[rec["t"] == t_step]
            assert len(got) == len(want) and got.tobytes() == want.tobytes(), t_step
    removed = int(stream.filtered().sum())
    assert 0 < removed < len(source.t) and int(stream.counts().sum()) > 0
    assert f"behind the noise filter ({removed} events filtered)" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="--denoise_us"):
        R.main(argv[:-3] + ["0"])


STEP_ENTRIES = ("dagr_stream_denoise", "dagr_stream_downsample", "dagr_stream_frame", "dagr_stream_stage",
                "dagr_stream_stage_capped", "dagr_stream_stage_dev", "dagr_stream_stage_dev_capped")     # not: sizes, resets, growth


def _record_stream_calls(monkeypatch):
    """Every dagr_stream_* entry of the library, wrapped to note its name."""
    L, calls = _lib.lib(), []
    for name in _lib.SIGNATURES:
        if name.startswith("dagr_stream_"):
            def wrapper(*a, _f=getattr(L, name), _n=name):
                calls.append(_n)
                return _f(*a)
            monkeypatch.setattr(L, name, wrapper)
    return calls


@pytest.mark.parametrize("config", ["plain", "downsample"])
def test_a_stream_without_the_options_calls_what_it_called_before(config, monkeypatch):
    """Without denoise_us / refractory_us: no denoise state, no denoise call, and per step the entries the stream had before
    the filter existed.  With them: the filter in front, and the _dev staging behind it."""
    kw = CONFIGS[config]
    model = _model(B)
    model.engine().set_low_latency(True)
    seq = _sequence(*((2 * W, 2 * H) if kw else (W, H)))[:3]
    calls = _record_stream_calls(monkeypatch)
    steps = {"plain": ["dagr_stream_stage"], "downsample": ["dagr_stream_downsample", "dagr_stream_stage_dev"]}[config]
    for noise in (dict(), dict(denoise_us=None, refractory_us=None)):
        stream = EventStream(model, window_us=WINDOW_US, **kw, **noise)
        st = stream.state
        assert st.noise is None and "noise" not in st.stages and st.lane_filtered is None
        del calls[:]
        with torch.no_grad():
            for s in seq:
                stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], t_now=s["t_now"])
        assert [c for c in calls if c in STEP_ENTRIES] == steps * len(seq), calls
        assert not any("denoise" in c for c in calls)
        assert not stream.filtered().any()
        with pytest.raises(RuntimeError, match="no stamp maps"):
            stream.last_stamps()
    stream = EventStream(model, window_us=WINDOW_US, **kw, **NOISE)
    del calls[:]
    with torch.no_grad():
        for s in seq:
            stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], t_now=s["t_now"])
    behind = ["dagr_stream_denoise"] + steps[:-1] + ["dagr_stream_stage_dev"]
    assert [c for c in calls if c in STEP_ENTRIES] == behind * len(seq), calls
    torch.cuda.synchronize()
