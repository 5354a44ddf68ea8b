"""Raw sensor events through the event stream on the GPU: dagr_stream_downsample + dagr_stream_stage_dev against the numpy
definition (StreamDefinition(downsample=2)), EventStream(downsample=2) against reset=True evaluations of the definition's
window on the same engine, a hot pixel, buffer growth, status bit 16, the absence of host waits and
scripts/run_stream.py --downsample.

The sequence and its reference are tests/stream_downsample_cases.py's (8 raw pushes, B = 3 lanes, a 640x480 sensor over the
320x215 model); tests/test_stream_downsample_cpu.py holds the definition to oracle/downsample.py on the same sequence.
That sequence has 2 x 2 cells, where the increment is a power of two; the front alone at 3 x 3, 4 x 3 and 3 x 1 runs on
tests/downsample_factor_cases.py's chunks against the reference script's own recorded outputs."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.streaming import EventStream, StreamDefinition
from dagr_amd.utils import synthetic as syn
from tests import downsample_factor_cases as fc
from tests import stream_downsample_cases as sc
from tests.test_streaming_gpu import _Stager, _assert_same_detections, _dev, _model, _window_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = sc.W, sc.H, sc.B


def _definition(window_us=sc.WINDOW_US):
    return StreamDefinition(B, W, H, time_window=sc.TW, window_us=window_us, downsample=sc.F, sensor_size=(sc.W_IN, sc.H_IN))


_WINDOWS = None


def _windows():
    """The definition's state after every push of the sequence: (pos, feat, batch, counts, change maps)."""
    global _WINDOWS
    if _WINDOWS is None:
        d = _definition()
        _WINDOWS = []
        for s in sc.sequence():
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
            _WINDOWS.append(d.formatted() + (d.counts(), d.change_map.copy()))
    return _WINDOWS


class _Front:
    """dagr_stream_downsample on a front state of its own: ``lanes`` lanes of a ``sensor`` = (W_in, H_in) sensor in cells of
    ``factors`` = (fx, fy) over a ``model`` = (width, height) model; the sequence's geometry unless told otherwise."""

    def __init__(self, max_push, lanes=B, factors=(sc.F, sc.F), sensor=(sc.W_IN, sc.H_IN), model=(W, H)):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.max_push, self.lanes, self.factors, self.sensor, self.model = max_push, lanes, factors, sensor, model
        self.cw, self.ch = sensor[0] // factors[0], sensor[1] // factors[1]
        nbytes = self.L.dagr_stream_front_bytes(lanes, self.cw, self.ch, max_push)
        assert nbytes > 4 * lanes * self.cw * self.ch
        self.front = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_front_reset(_lib.ptr(self.front), nbytes, lanes, self.cw, self.ch, max_push,
                                                  _lib.cur_stream(self.dev)), "front_reset")
        if not hasattr(self, "status"):
            self.status = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.s_xy = torch.zeros((max_push, 2), dtype=torch.int16, device=self.dev)
        self.s_t = torch.zeros((max_push,), dtype=torch.int64, device=self.dev)
        self.s_p = torch.zeros((max_push,), dtype=torch.int8, device=self.dev)
        self.s_batch = torch.zeros((max_push,), dtype=torch.int32, device=self.dev)
        self.s_n = torch.full((1,), -1, dtype=torch.int32, device=self.dev)

    def downsample(self, s, batch_dtype=np.int64):
        """One raw push through the front: the return code and the raw ``t`` and ``batch`` on the device."""
        P = _lib.ptr
        xy = _dev(np.stack([s["x"], s["y"]], -1).astype(np.int16).reshape(-1, 2))
        t, p, batch = _dev(s["t"]), _dev(s["p"]), _dev(s["batch"].astype(batch_dtype))
        rc = self.L.dagr_stream_downsample(P(self.front), self.front.numel(), self.lanes, self.max_push, *self.factors,
                                           *self.sensor, *self.model, P(xy), P(t), P(p), P(batch),
                                           1 if batch_dtype == np.int64 else 0, len(s["t"]), P(self.s_xy), P(self.s_t),
                                           P(self.s_p), P(self.s_batch), P(self.s_n), P(self.status),
                                           _lib.cur_stream(self.dev))
        return rc, t, batch

    def survivors(self):
        n = int(self.s_n)
        return dict(x=self.s_xy[:n, 0].cpu().numpy(), y=self.s_xy[:n, 1].cpu().numpy(), t=self.s_t[:n].cpu().numpy(),
                    p=self.s_p[:n].cpu().numpy(), batch=self.s_batch[:n].cpu().numpy())

    def maps(self):
        return self.front[:4 * self.lanes * self.cw * self.ch].view(torch.float32).view(self.lanes, self.ch, self.cw) \
            .cpu().numpy()


class _FrontStager(_Stager, _Front):
    """dagr_stream_downsample + dagr_stream_stage_dev on a bare graph workspace."""

    def __init__(self, cap, max_push):
        _Stager.__init__(self, cap)
        _Front.__init__(self, max_push)

    def stage(self, s, batch_dtype=np.int64):
        P, st = _lib.ptr, _lib.cur_stream(self.dev)
        n = len(s["t"])
        is64 = 1 if batch_dtype == np.int64 else 0
        t_now = None if s["t_now"] is None else _dev(s["t_now"])
        rc, t, batch = self.downsample(s, batch_dtype)
        if rc:
            return rc
        return self.L.dagr_stream_stage_dev(ctypes.byref(self.g.desc), P(self.g.workspace), P(self.state), B, self.state_cap,
                                            P(self.s_xy), P(self.s_t), P(self.s_p), P(self.s_batch), P(self.s_n), n, P(t),
                                            P(batch), is64, n, P(t_now), sc.WINDOW_US, P(self.pos), P(self.feat),
                                            P(self.batch), P(self.n_dev), P(self.lane_count), P(self.status), st)


def _assert_staged(st, want, where):
    pos, feat, batch, counts, maps = want
    n = int(counts.sum())
    assert int(st.n_dev) == n, where
    assert st.lane_count.tolist() == counts.tolist(), where
    assert np.array_equal(st.pos[:n].cpu().numpy(), pos), where
    assert np.array_equal(st.feat[:n].cpu().numpy(), feat.reshape(-1)), where
    assert np.array_equal(st.batch[:n].cpu().numpy(), batch.astype(np.int32)), where
    assert np.array_equal(st.maps(), maps), where
    assert int(st.status) == 0, where


@pytest.mark.parametrize("batch_dtype", [np.int64, np.int32], ids=["int64", "int32"])
def test_the_front_and_the_staging_equal_the_definition_and_the_build_continues(batch_dtype):
    """After every raw push: pos_out / feat_out / batch_out / *n_dev / lane_count equal the definition's window bit for bit,
    the survivors' count on the device equals the definition's, the change maps read back equal the definition's bit for
    bit, and the neighbour lists dagr_graph_build_window_dev then produces equal those of dagr_stage_window + the same build
    on the same window."""
    L, P = _lib.lib(), _lib.ptr
    cap = 16384
    st, ref = _FrontStager(cap, 12000), _Stager(cap)
    seq = sc.sequence()
    assert max(len(s["t"]) for s in seq) <= 12000
    before = np.zeros(B, np.int64)
    d = _definition()
    for k, (s, want) in enumerate(zip(seq, _windows())):
        _lib.check(st.stage(s, batch_dtype), "stream_downsample + stream_stage_dev")
        st.build()
        _assert_staged(st, want, k)
        # the survivors' count: what the definition's front lets through (the window's newcomers may be fewer)
        n_sv = len(d._downsample(s["x"], s["y"], s["t"], s["p"], s["batch"])[2])
        assert int(st.s_n) == n_sv, k
        pos, feat, batch, counts = want[:4]
        n = int(counts.sum())
        w_pos, w_feat, w_batch = _dev(pos), _dev(feat.reshape(-1)), _dev(batch)
        _lib.check(L.dagr_stage_window(ctypes.byref(ref.g.desc), P(ref.g.workspace), P(w_pos), P(w_feat), P(w_batch), 1, n,
                                       P(ref.pos), P(ref.feat), P(ref.batch), P(ref.n_dev), _lib.cur_stream(st.dev)),
                   "stage_window")
        ref.build()
        assert st.g.status() == ref.g.status(), k
        if n:
            assert torch.equal(st.g.edge_index(st.out[0][:n], st.out[2][:n])[0],
                               ref.g.edge_index(ref.out[0][:n], ref.out[2][:n])[0]), k
            assert torch.equal(st.out[2][:n], ref.out[2][:n]), k
        before = counts
    assert before.tolist() == [0, 0, 0]


_FACTOR_CASES = {}


def _factor_case(fx, fy):
    """tests/downsample_factor_cases.py's chunks as three raw pushes of 2 lanes (chunk 0 cut in two, then chunk 1; lane 1 a
    shifted copy) on a sensor one pixel larger than the 8 x 6 cells in every direction that has a strip (a factor of 1 has
    none), with four events per lane and chunk in that strip, over a model one cell smaller than the grid: ``(sensor,
    model, pushes, per push the definition's survivors and maps)``, computed once."""
    if (fx, fy) in _FACTOR_CASES:
        return _FACTOR_CASES[(fx, fy)]
    sx, sy = fc.CW * fx, fc.CH * fy                       # the first pixel right of / below the last whole cell
    sensor, model = (sx + (fx > 1), sy + (fy > 1)), (fc.CW - 1, fc.CH - 1)
    rng = np.random.Generator(np.random.PCG64(31 * fx + fy))

    def with_strip(ev):
        ry = rng.integers(0, sy, 4)
        pts = [(sx, ry[0]), (int(rng.integers(0, sx)), sy), (sx, sy), (sx, ry[3])] if fy > 1 else [(sx, int(v)) for v in ry]
        at = np.array([3, 5000, 17000, fc.CHUNK_EVENTS - 1])
        return dict(x=np.insert(ev["x"], at, [q[0] for q in pts]), y=np.insert(ev["y"], at, [q[1] for q in pts]),
                    t=np.insert(ev["t"], at, ev["t"][at]), p=np.insert(ev["p"], at, 1))

    pushes = []
    for ev in fc.chunks(fx, fy):
        lanes = [with_strip(ev), with_strip(fc.shifted(ev))]
        cuts = (0, 11003, len(lanes[0]["t"])) if not pushes else (0, len(lanes[0]["t"]))
        for a, b in zip(cuts[:-1], cuts[1:]):
            s = {k: np.concatenate([lane[k][a:b] for lane in lanes]) for k in ("x", "y", "t", "p")}
            s["batch"] = np.repeat(np.arange(2, dtype=np.int64), b - a)
            pushes.append(s)
    d = StreamDefinition(2, *model, downsample=(fx, fy), sensor_size=sensor)
    assert d.change_map.shape == (2, fc.CH, fc.CW)
    want = []
    for s in pushes:
        x, y, t, p, batch = d._downsample(s["x"], s["y"], s["t"], s["p"], s["batch"])
        want.append((dict(x=x, y=y, t=t, p=p, batch=batch), d.change_map.copy()))
    _FACTOR_CASES[(fx, fy)] = sensor, model, pushes, want
    return _FACTOR_CASES[(fx, fy)]


@pytest.mark.parametrize("batch_dtype", [np.int64, np.int32], ids=["int64", "int32"])
@pytest.mark.parametrize("fx,fy", [(3, 3), (4, 3), (3, 1)], ids=["3x3", "4x3", "3x1"])
def test_the_front_equals_the_reference_script_at_areas_that_are_no_power_of_two(fx, fy, batch_dtype):
    """k_front_integrate where the increment ``1 / (fx * fy)`` is no power of two: after every push the survivors, their
    count and the lanes' maps equal the definition's bit for bit, and lane 0 -- the fixture's own chunks plus events in the
    strip, which are dropped without a status bit -- equals what the reference's scripts/downsample_events.py kept and left
    in its change map (tests/golden/ref_py_downsample_factors.npz), cut to the model: a cell outside the model integrates as
    every other and keeps nothing."""
    fc.check_inputs(fx, fy)
    sensor, model, pushes, want = _factor_case(fx, fy)
    fr = _Front(len(pushes[-1]["t"]), lanes=2, factors=(fx, fy), sensor=sensor, model=model)
    assert (fr.cw, fr.ch) == (fc.CW, fc.CH)
    lane0 = []
    golden = fc.expected(fx, fy)
    for k, (s, (sv, maps)) in enumerate(zip(pushes, want)):
        strip = (s["x"] >= fc.CW * fx) | (s["y"] >= fc.CH * fy)
        assert int(strip.sum()) == (4, 4, 8)[k] and s["x"].max() < sensor[0] and s["y"].max() < sensor[1], k
        rc, _, _ = fr.downsample(s, batch_dtype)
        _lib.check(rc, "stream_downsample")
        got = fr.survivors()
        print(f"{fx}x{fy} push {k}: {len(s['t'])} raw, {len(got['t'])} survivors ({len(sv['t'])} by the definition), "
              f"cells that differ {int((fr.maps() != maps).sum())}")
        assert int(fr.s_n) == len(sv["t"]) > 100, k
        for name in ("x", "y", "t", "p", "batch"):
            assert np.array_equal(got[name].astype(np.int64), sv[name].astype(np.int64)), (k, name)
        assert np.array_equal(fr.maps(), maps), k
        assert int(fr.status) == 0, k
        lane0.append({name: got[name][got["batch"] == 0] for name in ("x", "y", "t", "p")})
        if k in (1, 2):                                    # the end of a chunk: lane 0 against the fixture itself
            _, ref, ref_map = golden[k - 1]
            inside = (ref["x"] < model[0]) & (ref["y"] < model[1])
            assert 0 < int(inside.sum()) < len(inside)
            for name in ("x", "y", "t", "p"):
                mine = np.concatenate([q[name] for q in lane0])
                assert np.array_equal(mine.astype(np.int64), ref[name][inside].astype(np.int64)), (k, name)
            assert np.array_equal(fr.maps()[0], ref_map), k
            lane0 = []


def test_a_hot_pixel_is_one_long_run():
    """One push with 2000 raw events on one cell (alternating in bursts, so the cell fires many times) among ordinary
    events: one thread walks the whole run."""
    rng = np.random.Generator(np.random.PCG64(5))
    n_hot = 2000
    hx, hy = 2 * 100 + rng.integers(0, 2, n_hot), 2 * 50 + rng.integers(0, 2, n_hot)
    hp = np.where((np.arange(n_hot) // 37) % 2 == 0, 1, -1).astype(np.int8)
    ht = np.int64(sc.T0) + np.sort(rng.integers(0, 9000, n_hot)).astype(np.int64)
    x, y, t, p = sc.raw_chunk(syn.edges_window, 300, 41, 0, 9000)
    x, y, t, p = np.concatenate([x, hx.astype(np.int16)]), np.concatenate([y, hy.astype(np.int16)]), \
        np.concatenate([t, ht]), np.concatenate([p, hp])
    o = np.argsort(t, kind="stable")
    lane1 = (x[o], y[o], t[o], p[o])
    s = sc.push({0: sc.raw_chunk(syn.uniform_window, 200, 42, 0, 9000), 1: lane1})
    d = _definition()
    d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
    w = d.window()
    hot = (w[4] == 1) & (w[0] == 100) & (w[1] == 50)
    assert int(hot.sum()) >= 200, int(hot.sum())
    st = _FrontStager(8192, 8192)
    _lib.check(st.stage(s), "stream_downsample + stream_stage_dev")
    st.build()
    _assert_staged(st, d.formatted() + (d.counts(), d.change_map), "hot pixel")


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_downsampling_stream_detections_equal_reset_true_on_the_definitions_window(latency):
    model = _model(B)
    eng = model.engine().set_low_latency(latency)
    stream = EventStream(model, window_us=sc.WINDOW_US, downsample=sc.F, sensor_size=(sc.W_IN, sc.H_IN))
    total = 0
    with torch.no_grad():
        for rnd in range(2):                    # after reset() the same pushes give the same results again
            for k, (s, w) in enumerate(zip(sc.sequence(), _windows())):
                det, nk = stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], t_now=s["t_now"])
                got = (det.clone(), nk.clone())
                want = eng.forward_detections(*_window_dev(w))
                _assert_same_detections(got, want, B, (rnd, k))
                total += int(got[1].sum())
                if k in (0, 4):
                    assert stream.counts().tolist() == w[3].tolist(), (rnd, k)
                    assert np.array_equal(stream.change_maps(), w[4]), (rnd, k)
            stream.check_status()
            assert stream.counts().tolist() == [0, 0, 0]
            stream.reset()
            assert not stream.change_maps().any()
    assert total > 0, "no step kept a detection: the comparison is empty"
    if latency:
        assert eng._wg is not None, "the window was not captured"
    eng.set_low_latency(True)


def test_a_raw_stream_that_outgrows_the_engine_and_the_front_grows_and_stays_equal():
    from dagr_amd.engine import StreamState, WindowEngine
    model = _model(B)
    eng = WindowEngine(model, max_events=1024).set_low_latency(True)
    cap0 = eng.max_events
    st = StreamState(B, sc.TW, eng.device)               # a window that never expires anything here
    st.enable_front(sc.F, sc.F, sc.W_IN, sc.H_IN, W, H)
    front0 = st.stages["front"].cap
    d = _definition(window_us=sc.TW)
    sizes = [(40, 10, 21)] * 4 + [(1000, 0, 199)] + [(23, 11, 5)] * 3   # raw pushes of ~320, then ~5400 > the front's 4096
    t = 0
    grown_at = None
    with torch.no_grad():
        for k, lanes in enumerate(sizes):
            s = sc.push({b: sc.raw_chunk(syn.edges_window, n, 100 + 3 * k + b, t, t + 1000) for b, n in enumerate(lanes) if n})
            t += 1003
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
            xy = _dev(np.stack([s["x"], s["y"]], -1))
            _, (det, nk) = eng.forward_stream(st, xy, _dev(s["t"]), _dev(s["p"]), _dev(s["batch"]))
            got = (det.clone(), nk.clone())
            if grown_at is None and eng.max_events > cap0:
                grown_at = k
                assert eng._wg is None and st.cap == eng.max_events        # grown: captured anew
            pos, feat, batch = d.formatted()
            _assert_same_detections(got, eng.forward_detections(_dev(pos), _dev(feat), _dev(batch)), B, k)
    assert grown_at is not None and grown_at > 0, grown_at
    assert st.stages["front"].cap > front0 and len(s["t"]) < front0
    assert eng._wg is not None, "the grown window was not captured again"
    torch.cuda.synchronize()
    assert int(st.status) == 0 and st.lane_count.tolist() == d.counts().tolist()
    assert np.array_equal(st.change_maps(), d.change_map)                  # carried across the front's growth
    eng.check_status()


def test_a_raw_event_outside_the_sensor_raises_bit_16_and_is_named():
    model = _model(B)
    model.check_device_status = False
    stream = EventStream(model, window_us=sc.WINDOW_US, downsample=sc.F)
    assert stream.state.front[:4] == (2, 2, 2 * W, 2 * H)
    xy = np.array([[5, 5], [2 * W, 6], [7, 7]], np.int16)
    t = np.array([sc.T0 + 100, sc.T0 + 200, sc.T0 + 300], np.int64)
    p = np.array([1, -1, 1], np.int8)
    with torch.no_grad():
        out = stream.step(xy, t, p, batch=np.array([0, 1, 1]))
    assert len(out) == B
    assert int(stream.state.status) == 16
    with pytest.raises(RuntimeError, match="outside the sensor"):
        stream.check_status()
    maps = stream.change_maps()
    assert maps[0, 2, 2] == np.float32(0.25) and maps[1, 3, 3] == np.float32(0.25) and int((maps != 0).sum()) == 2
    model.check_device_status = True
    stream.reset()
    with torch.no_grad():
        stream.step(xy[:1], t[:1], p[:1])                 # check_status inside: the reset stream is clean
    assert stream.counts().tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="cell grid"):
        EventStream(model, downsample=2, sensor_size=(640, 428))
    with pytest.raises(ValueError, match="downsample"):
        EventStream(model, downsample=0)


def test_a_step_on_device_inputs_waits_for_nothing():
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
    stream = EventStream(model, window_us=sc.WINDOW_US, downsample=sc.F, sensor_size=(sc.W_IN, sc.H_IN))
    pushes = []
    for k in range(6):
        s = sc.push({b: sc.raw_chunk(syn.edges_window, 300, 60 + 3 * k + b, 1000 * k, 1000 * k + 900) for b in range(B)})
        pushes.append((_dev(np.stack([s["x"], s["y"]], -1)), _dev(s["t"]), _dev(s["p"]), _dev(s["batch"].astype(np.int32))))
    with torch.no_grad():
        for xy, t, p, batch in pushes[:4]:                 # two eager steps, the capture, one replay
            stream.step_device(xy, t, p, batch=batch)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for xy, t, p, batch in pushes[4:]:
                det, nk = stream.step_device(xy, t, p, batch=batch)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    d = _definition()
    for xy, t, p, batch in pushes:
        d.push(xy[:, 0].cpu().numpy(), xy[:, 1].cpu().numpy(), t.cpu().numpy(), p.cpu().numpy(), batch.cpu().numpy())
    assert stream.counts().tolist() == d.counts().tolist() and sum(d.counts()) > 0
    stream.check_status()


def test_run_stream_script_downsamples_and_writes_one_row_block_per_step(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    from dagr_amd.utils.buffers import detections_to_records
    model = _model(1)
    argv = ["--step_us", "1000", "--window_us", "5000", "--steps", "8", "--stream", "edges", "--width", str(W),
            "--height", str(H), "--events_per_window", "400000", "--output_directory", str(tmp_path), "--sequence", "raw",
            "--downsample", "2", "--sensor_width", "640", "--sensor_height", "480"]
    a = C.flags("", argv, extra=R.stream_options)
    source = R.SyntheticStream(a)
    assert (source.width, source.height) == (W, H) and (source.sensor_width, source.sensor_height) == (640, 480)
    assert int(source.x.max()) >= W and int(source.y.max()) >= H            # sensor coordinates
    path = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    assert os.path.basename(str(path)) == "detections_raw.npy"
    rec = np.load(path)
    assert np.all(np.diff(rec["t"].astype(np.int64)) >= 0)
    t0, t1 = source.t_range()
    steps = list(range(t0 + 1000, t1 + 1, 1000))
    assert len(steps) == 8 and set(rec["t"].tolist()) <= set(steps)
    stream = EventStream(model, window_us=5000, downsample=2, sensor_size=(640, 480))
    with torch.no_grad():
        for t_step in steps:
            ev = source.events(t_step - 1000, t_step)
            det = stream.step(np.stack([ev["x"], ev["y"]], -1), ev["t"], ev["p"], t_now=t_step)[0]
            want = detections_to_records({k: v.cpu() for k, v in det.items()}, np.uint64(t_step))
            got = rec[rec["t"] == t_step]
            assert len(got) == len(want) and got.tobytes() == want.tobytes(), t_step
    assert int(stream.counts().sum()) > 0, "nothing survived the downsampling: the comparison is empty"
