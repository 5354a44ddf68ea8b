"""Event streams on the GPU: dagr_stream_stage against the numpy definition (dagr_amd/streaming.py: StreamDefinition),
EventStream / WindowEngine.forward_stream against reset=True evaluations of the definition's window on the same engine,
buffer growth, the status bits, the --use_image path and scripts/run_stream.py.

One scripted sequence of 8 pushes serves the staging, detection and model-level tests: B = 3 lanes on the engine suite's
small sensor (320x215), S-edges and uniform events with absolute timestamps from 2^33 us on (int64 matters), lane sizes
that put no lane boundary on a multiple of the 256-thread block."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import model as om
from dagr_amd import _lib
from dagr_amd.streaming import EventStream, StreamDefinition
from dagr_amd.utils import synthetic as syn
from dagr_amd.utils.testing_weights import randomize_

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 3
TW = 1000000
WINDOW_US = 20000
T0 = (1 << 33) + 777


def _chunk(gen, n, seed, t_lo, t_hi):
    """n events of a synthetic stream with T0 + t_lo <= t <= T0 + t_hi (sorted, int64)."""
    x, y, t, p = gen(n, W, H, seed, window_us=t_hi - t_lo, time_window=t_hi - t_lo)
    return x, y, np.int64(T0 + t_lo) + t.astype(np.int64), p


def _push(parts, t_now=None):
    """parts: {lane: (x, y, t, p)} -> one push in lane order."""
    lanes = sorted(parts)
    cat = [np.concatenate([parts[b][k] for b in lanes]) if lanes else np.zeros(0, dt)
           for k, dt in enumerate((np.int16, np.int16, np.int64, np.int8))]
    batch = np.concatenate([np.full(len(parts[b][2]), b, np.int64) for b in lanes]) if lanes else np.zeros(0, np.int64)
    return dict(x=cat[0].astype(np.int16), y=cat[1].astype(np.int16), t=cat[2].astype(np.int64), p=cat[3].astype(np.int8),
                batch=batch, t_now=None if t_now is None else np.asarray(t_now, np.int64) + T0)


_SEQ = None


def _sequence():
    """The 8 pushes (see the module docstring); WINDOW_US = 20 ms."""
    global _SEQ
    if _SEQ is not None:
        return _SEQ
    E, U = syn.edges_window, syn.uniform_window
    # 0: three lanes of 1500 / 37 / 700 events in the first 10 ms; lane 0 holds two events at t = 3000 and two at 3001
    l0 = list(_chunk(E, 1500, 1, 0, 10000))
    i = int(np.searchsorted(l0[2], T0 + 3000))
    l0[2][i:i + 2], l0[2][i + 2:i + 4] = T0 + 3000, T0 + 3001
    l0[2] = np.maximum.accumulate(l0[2])
    seq = [_push({0: tuple(l0), 1: _chunk(U, 37, 2, 0, 9000), 2: _chunk(E, 700, 3, 0, 9500)})]
    # 1: events for lane 1 only (lanes 0 and 2 keep their reference instants)
    seq.append(_push({1: _chunk(U, 421, 4, 10000, 15000)}))
    # 2: a single event
    seq.append(_push({2: (np.array([17], np.int16), np.array([101], np.int16), np.array([T0 + 12000], np.int64),
                          np.array([-1], np.int8))}))
    # 3: zero events, t_now = 23000: lane 0's events at t = 3000 are exactly WINDOW_US old and leave, those at 3001 stay
    seq.append(_push({}, t_now=[23000] * 3))
    # 4: lanes 0 and 2, t_now given
    seq.append(_push({0: _chunk(E, 1203, 5, 23000, 30000), 2: _chunk(U, 655, 6, 23500, 29000)}, t_now=[30000] * 3))
    # 5: a jump that expires lanes 0 and 2 entirely; lane 1 stays where it was and receives events
    seq.append(_push({1: _chunk(E, 333, 7, 29000, 30000)}, t_now=[55000, 30000, 55000]))
    # 6: all lanes again, no t_now
    seq.append(_push({0: _chunk(E, 801, 8, 55000, 60000), 1: _chunk(U, 64, 9, 30000, 34000),
                      2: (np.array([300], np.int16), np.array([7], np.int16), np.array([T0 + 56000], np.int64),
                          np.array([1], np.int8))}))
    # 7: a jump that expires everything
    seq.append(_push({}, t_now=[200000] * 3))
    _SEQ = seq
    return seq


_WINDOWS = None


def _windows():
    """The definition's state after every push: (formatted pos, feat, batch, counts)."""
    global _WINDOWS
    if _WINDOWS is None:
        d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US)
        _WINDOWS = []
        for s in _sequence():
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
            _WINDOWS.append(d.formatted() + (d.counts(),))
    return _WINDOWS


def test_the_sequence_holds_what_it_is_meant_to():
    counts = [w[3].tolist() for w in _windows()]
    seq = _sequence()
    assert counts[0] == [1500, 37, 700] and set(seq[1]["batch"].tolist()) == {1} and len(seq[2]["t"]) == 1
    assert len(seq[3]["t"]) == 0 and len(seq[7]["t"]) == 0
    t0 = seq[0]["t"][seq[0]["batch"] == 0] - T0
    n3000, n_le = int((t0 == 3000).sum()), int((t0 <= 3000).sum())
    assert n3000 >= 2 and int((t0 == 3001).sum()) >= 2 and counts[3][0] == 1500 - n_le       # the cut splits equal stamps
    assert counts[5][0] == 0 and counts[5][2] == 0 and counts[5][1] > 333
    assert counts[7] == [0, 0, 0]
    for c in counts:                        # no lane boundary on a multiple of the block size
        for edge in np.cumsum(c)[:-1]:
            assert edge % 256 != 0 or edge == 0 or c == [0, 0, 0], c


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bare_builder(cap):
    from dagr_amd.graph.ev_graph import WindowGraphBuilder
    return WindowGraphBuilder(W, H, B, 16, 128, int(0.01 * W + 1), int(0.01 * TW), time_window=TW, max_events=cap,
                              device=torch.device("cuda:0"))


class _Stager:
    """dagr_stream_stage on a bare graph workspace."""

    def __init__(self, cap, state_cap=None):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.g, self.cap = _bare_builder(cap), cap
        self.state_cap = state_cap or cap
        self.state = torch.empty(self.L.dagr_stream_state_bytes(B, self.state_cap), dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_reset(_lib.ptr(self.state), B, self.state_cap, _lib.cur_stream(self.dev)), "reset")
        self.pos = torch.zeros((cap, 3), device=self.dev)
        self.feat = torch.zeros((cap,), device=self.dev)
        self.batch = torch.zeros((cap,), dtype=torch.int32, device=self.dev)
        self.n_dev = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.lane_count = torch.zeros((B,), dtype=torch.int32, device=self.dev)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.out = (torch.zeros((cap, 16), dtype=torch.int32, device=self.dev),
                    torch.zeros((cap, 16), dtype=torch.int16, device=self.dev),
                    torch.zeros((cap,), dtype=torch.int32, device=self.dev))

    def stage(self, s, window_us=WINDOW_US):
        P = _lib.ptr
        xy = _dev(np.stack([s["x"], s["y"]], -1).astype(np.int16).reshape(-1, 2))
        t, p, batch = _dev(s["t"]), _dev(s["p"]), _dev(s["batch"])
        t_now = None if s["t_now"] is None else _dev(s["t_now"])
        return self.L.dagr_stream_stage(ctypes.byref(self.g.desc), P(self.g.workspace), P(self.state), B, self.state_cap,
                                        P(xy), P(t), P(p), P(batch), 1, len(s["t"]), P(t_now), window_us, P(self.pos),
                                        P(self.feat), P(self.batch), P(self.n_dev), P(self.lane_count), P(self.status),
                                        _lib.cur_stream(self.dev))

    def build(self):
        """dagr_graph_build_window_dev continues from the staging (and leaves the workspace ready for the next window)."""
        self.g.build(self.pos, self.batch, out=self.out, n_dev=self.n_dev)


def test_staging_equals_the_definition_and_the_build_continues_from_it():
    """Staging alone, no model: after every push pos_out / feat_out / batch_out / *n_dev / lane_count equal the numpy
    definition + format_data_np bit for bit, and the neighbour lists dagr_graph_build_window_dev then produces equal those of
    dagr_stage_window + the same build on the same window."""
    L, P = _lib.lib(), _lib.ptr
    cap = 4096
    st, ref = _Stager(cap), _Stager(cap)
    dev = st.dev
    for k, (s, (pos, feat, batch, counts)) in enumerate(zip(_sequence(), _windows())):
        _lib.check(st.stage(s), "stream_stage")
        st.build()
        n = int(counts.sum())
        assert int(st.n_dev) == n, k
        assert st.lane_count.tolist() == counts.tolist(), k
        assert np.array_equal(st.pos[:n].cpu().numpy(), pos), k
        assert np.array_equal(st.feat[:n].cpu().numpy(), feat.reshape(-1)), k
        assert np.array_equal(st.batch[:n].cpu().numpy(), batch.astype(np.int32)), k
        assert int(st.status) == 0, k
        # the same window through dagr_stage_window
        w_pos, w_feat, w_batch = _dev(pos), _dev(feat.reshape(-1)), _dev(batch)     # (alive until the launch is issued)
        _lib.check(L.dagr_stage_window(ctypes.byref(ref.g.desc), P(ref.g.workspace), P(w_pos), P(w_feat), P(w_batch), 1, n,
                                       P(ref.pos), P(ref.feat), P(ref.batch), P(ref.n_dev), _lib.cur_stream(dev)),
                   "stage_window")
        ref.build()
        assert st.g.status() == ref.g.status(), k
        if n:
            e_st = st.g.edge_index(st.out[0][:n], st.out[2][:n])[0]
            e_ref = ref.g.edge_index(ref.out[0][:n], ref.out[2][:n])[0]
            assert torch.equal(e_st, e_ref), k
            assert torch.equal(st.out[2][:n], ref.out[2][:n]), k
            valid = torch.arange(16, device=dev)[None, :] < st.out[2][:n, None]       # slots >= deg are left untouched
            assert torch.equal(st.out[0][:n][valid], ref.out[0][:n][valid]), k
            assert torch.equal(st.out[1][:n][valid], ref.out[1][:n][valid]), k


def test_capacity_overflow_is_flagged_and_clamped():
    """Bit 2 through the C entry point, with a state sized below the need: argument checking, not fault provocation --
    the kernel clamps the window to the capacity and says so."""
    st = _Stager(4096, state_cap=512)
    a = _push({0: _chunk(syn.uniform_window, 400, 21, 0, 1000)})
    b = _push({0: _chunk(syn.uniform_window, 150, 22, 1000, 2000), 2: _chunk(syn.uniform_window, 250, 23, 0, 2000)})
    _lib.check(st.stage(a), "stream_stage")
    st.build()
    assert int(st.status) == 0 and int(st.n_dev) == 400
    _lib.check(st.stage(b), "stream_stage")            # 400 + 400 > 512
    st.build()
    assert int(st.status) == 4
    assert int(st.n_dev) == 512 and int(st.lane_count.sum()) == 512 and st.lane_count.tolist()[0] == 512
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    big = _push({1: _chunk(syn.uniform_window, 513, 24, 3000, 4000)})
    assert st.stage(big) == bad                          # capacity < n_new: refused before any launch
    assert st.stage(a, window_us=TW + 1) == bad


_MODELS = {}


def _model(batch_size, **over):
    """tests/test_engine_gpu.py::_setup, cached per configuration."""
    from dagr_amd.model.networks.dagr import DAGR
    key = (batch_size, tuple(sorted(over.items())))
    if key not in _MODELS:
        torch.manual_seed(12)
        args = om.default_args(batch_size=batch_size, **over)
        model = randomize_(DAGR(args, height=H, width=W), seed=12).eval().cuda()
        model.cache_luts(width=W, height=H, radius=args.radius)
        _MODELS[key] = model
    m = _MODELS[key]
    m.conf_threshold, m.nms_threshold, m.check_device_status = 0.001, 0.65, True
    return m


def _step_args(s):
    return (np.stack([s["x"], s["y"]], -1), s["t"], s["p"]), dict(batch=s["batch"], t_now=s["t_now"])


def _window_dev(w):
    return _dev(w[0]), _dev(w[1]), _dev(w[2])


def _assert_same_detections(got, want, lanes, where):
    (det, nk), (det_w, nk_w) = got, want
    assert torch.equal(nk, nk_w), where
    for b in range(lanes):
        n = int(nk[b])
        assert torch.equal(det[b, :n], det_w[b, :n]), (where, b)


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_stream_detections_equal_reset_true_on_the_same_window(latency):
    """step_device's (det, n_keep) == eng.forward_detections(the definition's window) on the same engine, called between
    the stream steps (a plain window between two steps leaves the stream intact), every lane, every step; latency mode
    replays the captured window, throughput mode runs its body launch by launch."""
    model = _model(B)
    eng = model.engine().set_low_latency(latency)
    stream = EventStream(model, window_us=WINDOW_US)
    total = 0
    with torch.no_grad():
        for k, (s, w) in enumerate(zip(_sequence(), _windows())):
            a, kw = _step_args(s)
            det, nk = stream.step_device(*a, **kw)
            got = (det.clone(), nk.clone())
            assert not eng.can_append()                        # the count has not been read
            want = eng.forward_detections(*_window_dev(w))
            _assert_same_detections(got, want, B, k)
            total += int(got[1].sum())
    assert total > 0, "no step kept a detection: the comparison is empty"
    if latency:
        assert eng._wg is not None, "the window was not captured"
    stream.check_status()
    assert stream.counts().tolist() == [0, 0, 0]
    eng.set_low_latency(True)


def test_a_stream_may_begin_with_an_empty_push():
    """A sensor that is quiet at start-up: the first step brings zero events and only moves t_now.  The state is
    allocated all the same, the counts are zero, the detections are those of the empty window, and the stream goes on."""
    model = _model(B)
    eng = model.engine().set_low_latency(True)
    stream = EventStream(model, window_us=WINDOW_US)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US)
    empty = _push({}, t_now=[100] * 3)
    more = _push({0: _chunk(syn.edges_window, 611, 31, 100, 4000), 2: _chunk(syn.uniform_window, 45, 32, 200, 3000)})
    with torch.no_grad():
        for k, s in enumerate((empty, more)):
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
            a, kw = _step_args(s)
            det, nk = stream.step_device(*a, **kw)
            got = (det.clone(), nk.clone())
            _assert_same_detections(got, eng.forward_detections(*_window_dev(d.formatted())), B, k)
            assert stream.counts().tolist() == d.counts().tolist(), k
    assert d.counts().tolist() == [611, 0, 45]
    stream.check_status()


def test_step_returns_what_the_model_returns_and_counts_what_the_definition_counts():
    model = _model(B)
    stream = EventStream(model, window_us=WINDOW_US)
    eng = model.engine().set_low_latency(True)
    with torch.no_grad():
        for k, (s, w) in enumerate(zip(_sequence(), _windows())):
            a, kw = _step_args(s)
            got = stream.step(*a, **kw)
            got = [{n: v.clone() for n, v in d.items()} for d in got]
            assert model._window is None
            assert stream.counts().tolist() == w[3].tolist(), k
            assert eng._N == int(w[3].sum()), k
            pos, feat, batch = _window_dev(w)
            want = model(types.SimpleNamespace(pos=pos, x=feat, batch=batch), reset=True)[0]
            assert len(got) == len(want) == B
            for b in range(B):
                for name in ("boxes", "scores", "labels"):
                    assert torch.equal(got[b][name], want[b][name]), (k, b, name)
    # the same stream again after reset(), from device tensors this time
    stream.reset()
    s, w = _sequence()[0], _windows()[0]
    a, kw = _step_args(s)
    with torch.no_grad():
        det, nk = stream.step_device(_dev(a[0]), _dev(a[1]), _dev(a[2]), batch=_dev(kw["batch"]))
        got = (det.clone(), nk.clone())
        _assert_same_detections(got, eng.forward_detections(*_window_dev(w)), B, "device inputs")
    assert stream.counts().tolist() == w[3].tolist()


def test_a_stream_that_outgrows_the_engine_grows_recaptures_and_stays_equal():
    from dagr_amd.engine import StreamState, WindowEngine
    model = _model(B)
    eng = WindowEngine(model, max_events=1024).set_low_latency(True)
    cap0 = eng.max_events
    assert cap0 == 1024
    st = StreamState(B, TW, eng.device)                  # a window that never expires anything here
    d = StreamDefinition(B, W, H, time_window=TW, window_us=TW)
    sizes = [(150, 20, 31)] * 4 + [(301, 0, 199)] + [(23, 11, 5)] * 5        # 804 resident, then 1304 > 1024
    t = 0
    with torch.no_grad():
        for k, lanes in enumerate(sizes):
            s = _push({b: _chunk(syn.edges_window, n, 100 + 3 * k + b, t, t + 1000) for b, n in enumerate(lanes) if n})
            t += 1000
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
            xy = _dev(np.stack([s["x"], s["y"]], -1))
            _, (det, nk) = eng.forward_stream(st, xy, _dev(s["t"]), _dev(s["p"]), _dev(s["batch"]))
            got = (det.clone(), nk.clone())
            if k == 3:
                assert eng._wg is not None and eng.max_events == cap0
            if k == 4:
                assert eng.max_events > cap0 and st.cap == eng.max_events and eng._wg is None      # grown: captured anew
            pos, feat, batch = d.formatted()
            _assert_same_detections(got, eng.forward_detections(_dev(pos), _dev(feat), _dev(batch)), B, k)
    assert eng._wg is not None, "the grown window was not captured again"
    torch.cuda.synchronize()
    assert int(st.status) == 0 and st.lane_count.tolist() == d.counts().tolist()
    eng.check_status()
    # the stream outlives the engine: a rebuilt engine with a smaller capacity is grown to the stream's on its next step
    eng2 = WindowEngine(model, max_events=1024).set_low_latency(True)
    s = _push({1: _chunk(syn.uniform_window, 77, 150, t, t + 1000)})
    d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
    with torch.no_grad():
        _, (det, nk) = eng2.forward_stream(st, _dev(np.stack([s["x"], s["y"]], -1)), _dev(s["t"]), _dev(s["p"]), _dev(s["batch"]))
        got = (det.clone(), nk.clone())
        pos, feat, batch = d.formatted()
        _assert_same_detections(got, eng2.forward_detections(_dev(pos), _dev(feat), _dev(batch)), B, "rebuilt engine")
    assert eng2.max_events >= st.cap
    torch.cuda.synchronize()
    assert int(st.status) == 0 and st.lane_count.tolist() == d.counts().tolist()


@pytest.mark.parametrize("case", ["backwards_in_push", "backwards_across_pushes", "t_now_behind", "unsorted_batch",
                                  "batch_out_of_range"])
def test_malformed_pushes_are_flagged_and_named(case):
    model = _model(B)
    model.check_device_status = False
    stream = EventStream(model, window_us=WINDOW_US)
    xy = np.array([[5, 5], [6, 6]], np.int16)
    p = np.array([1, -1], np.int8)
    t = np.array([T0 + 100, T0 + 200], np.int64)
    with torch.no_grad():
        out = stream.step(xy, t, p, batch=np.array([0, 1]))
        stream.check_status()
        if case == "backwards_in_push":
            out = stream.step(xy, t[::-1].copy() + 1000, p, batch=np.array([1, 1]))
            name = "backwards"
        elif case == "backwards_across_pushes":
            out = stream.step(xy, t - 50, p, batch=np.array([0, 2]))          # lane 0: T0 + 50 after T0 + 100
            name = "backwards"
        elif case == "t_now_behind":
            out = stream.step(xy, t + 1000, p, batch=np.array([0, 1]), t_now=np.array([T0 + 1050, T0 + 1300, T0 + 1300]))
            name = "t_now"
        elif case == "unsorted_batch":
            out = stream.step(xy, t + 1000, p, batch=np.array([1, 0]))
            name = "batch"
        else:
            out = stream.step(xy, t + 1000, p, batch=np.array([1, 3]))
            name = "batch"
    assert len(out) == B                                 # the call returns normally
    with pytest.raises(RuntimeError, match=name):
        stream.check_status()
    model.check_device_status = True
    stream.reset()
    with torch.no_grad():
        stream.step(xy, t, p, batch=np.array([0, 1]))    # check_status inside: the reset stream is clean
    assert stream.counts().tolist() == [1, 1, 0]


def _rel_err(a, b):
    """|a - b| <= tol * (unit + |b|), unit = max(1, rms(b)) over finite entries: the engine suite's measure."""
    a, b = a.float().cpu(), b.float().cpu()
    ok = torch.isfinite(a) & torch.isfinite(b)
    a, b = a[ok], b[ok]
    unit = max(1.0, float(b.pow(2).mean().sqrt()))
    return ((a - b).abs() / (unit + b.abs())).max().item()


def test_use_image_stream_keeps_the_last_frame():
    """resnet18, B = 2: a frame on the first step, none on the second, a new one on the third.  Every step's (det, n_keep)
    are compared with eng.forward_detections(the definition's window, image=the frame in force).  Two replays of the same
    captured graph on the same inputs were observed NOT to be bit-equal here (n_keep equal, 175 of 175 anchors kept at
    conf 0.001, but rows in another order: the image branch's library kernels differ in their last bits from run to
    run), so n_keep is compared exactly and every row is matched to a row of the other side.  The decoded outputs
    are held to the engine suite's 1e-4 against forward_raw as well, and a plain call with ANOTHER frame between two
    steps must not change what the next frame-less step sees."""
    model = _model(2, use_image=True, img_net="resnet18")
    eng = model.engine().set_low_latency(True)
    stream = EventStream(model, window_us=WINDOW_US)
    d = StreamDefinition(2, W, H, time_window=TW, window_us=WINDOW_US)
    imgs = [torch.rand((2, 3, H, W), generator=torch.Generator().manual_seed(s)).cuda() for s in (7, 8)]
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="frame"):
            stream.step_device(np.zeros((0, 2), np.int16), np.zeros(0, np.int64), np.zeros(0, np.int8))
        warm = _push({b: _chunk(syn.uniform_window, 500, 190 + b, 0, 5000) for b in range(2)})
        dw = StreamDefinition(2, W, H, time_window=TW, window_us=WINDOW_US)
        dw.push(warm["x"], warm["y"], warm["t"], warm["p"], warm["batch"])
        w_in = tuple(_dev(v) for v in dw.formatted())
        for _ in range(4):                                    # two eager runs, the capture, one replay
            eng.forward_detections(*w_in, image=imgs[1])
        assert eng._wg is not None
        t = 0
        for k, (frame, used) in enumerate(((imgs[0], imgs[0]), (None, imgs[0]), (imgs[1], imgs[1]))):
            s = _push({b: _chunk(syn.uniform_window, n, 200 + 2 * k + b, t, t + 5000) for b, n in enumerate((901, 650))})
            t += 5000
            d.push(s["x"], s["y"], s["t"], s["p"], s["batch"])
            out, (det, nk) = eng.forward_stream(stream.state, _dev(np.stack([s["x"], s["y"]], -1)), _dev(s["t"]),
                                                _dev(s["p"]), _dev(s["batch"]), image=frame)
            out, det, nk = out.clone(), det.clone(), nk.clone()
            pos, feat, batch = (_dev(v) for v in d.formatted())
            want_det, want_nk = eng.forward_detections(pos, feat, batch, image=used)
            want_det, want_nk = want_det.clone(), want_nk.clone()
            assert torch.equal(nk, want_nk), k
            for b in range(2):
                n = int(nk[b])
                g_, w_ = det[b, :n], want_det[b, :n]
                # rows come out by descending score, and scores that differ in their last bits change places: every row
                # is matched with its nearest row of the other side (label equal; boxes to 1e-2 px, scores to 1e-4, the
                # bounds tests/test_model_api_gpu.py holds detections to)
                diff = (g_[:, None, :] - w_[None, :, :]).abs()
                cost = torch.maximum(diff[..., :4].amax(-1) / 1e-2, diff[..., 4] / 1e-4) + 1e9 * (diff[..., 5] != 0)
                print(k, b, "n_keep", n, "rows in place", int((g_ == w_).all(1).sum()), "worst matched row (in bounds)",
                      float(cost.min(1).values.max()), float(cost.min(0).values.max()))
                assert float(cost.min(1).values.max()) <= 1.0 and float(cost.min(0).values.max()) <= 1.0, (k, b)
            want = eng.forward_raw(pos, feat, batch, image=used).clone()
            assert _rel_err(out, want) < 1e-4, k
            # a plain call with ANOTHER frame between two steps (it rewrites the engine's frame buffer, not the stream's)
            other = eng.forward_raw(pos, feat, batch, image=imgs[1] if used is imgs[0] else imgs[0]).clone()
            assert _rel_err(out, other) > 1e-3, k         # (the frame matters: the comparison above can tell frames apart)
    stream.check_status()
    assert stream.counts().tolist() == d.counts().tolist()


def test_run_stream_script_writes_one_row_block_per_step(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    from dagr_amd.utils.buffers import detections_to_records
    model = _model(1)
    argv = ["--step_us", "1000", "--window_us", "5000", "--steps", "10", "--stream", "edges", "--width", str(W),
            "--height", str(H), "--events_per_window", "40000", "--output_directory", str(tmp_path), "--sequence", "mem"]
    a = C.flags("", argv, extra=R.stream_options)
    source = R.SyntheticStream(a)
    path = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    assert os.path.basename(str(path)) == "detections_mem.npy"
    rec = np.load(path)
    assert len(rec) > 0 and np.all(np.diff(rec["t"].astype(np.int64)) >= 0)
    t0, t1 = source.t_range()
    steps = list(range(t0 + 1000, t1 + 1, 1000))
    assert len(steps) == 10 and set(rec["t"].tolist()) <= set(steps)
    stream = EventStream(model, window_us=5000)
    with torch.no_grad():
        for t_step in steps:
            ev = source.events(t_step - 1000, t_step)
            det = stream.step(np.stack([ev["x"], ev["y"]], -1), ev["t"], ev["p"], t_now=t_step)[0]
            want = detections_to_records({k: v.cpu() for k, v in det.items()}, np.uint64(t_step))
            got = rec[rec["t"] == t_step]
            assert len(got) == len(want) and got.tobytes() == want.tobytes(), t_step
