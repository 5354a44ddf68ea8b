"""The capped event stream on the GPU (max_lane_events): dagr_stream_stage_capped / dagr_stream_stage_dev_capped against
the numpy definition (dagr_amd/streaming.py: StreamDefinition), the uncapped entries unchanged, EventStream against
reset=True evaluations of the definition's window on the same engine, a burst that costs its own lane only, buffers and
graphs that stay the same objects over steps without a read-back, the pure count window as an N-Caltech101 sample, and
scripts/run_stream.py --max_lane_events.

Everything compared is an integer or compared bit for bit.  Shapes as in tests/test_streaming_gpu.py: B = 3 lanes on
320x215, timestamps from 2^33 us on, the dagr-s events-only model of that file; the sequences are in
tests/stream_cap_cases.py, whose CPU tests say what they hold."""
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
from tests import stream_cap_cases as cc
from tests.test_streaming_gpu import _assert_same_detections, _bare_builder, _dev, _model, _sequence, _step_args, _window_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B, TW, T0 = cc.W, cc.H, cc.B, cc.TW, cc.T0
WINDOW_US = cc.WINDOW_US
F = 2                                   # the front of test 3: a 640 x 430 sensor over the 320 x 215 model


class _Stager:
    """The four stream staging entries on a bare graph workspace (the _Stager of tests/test_streaming_gpu.py with the cap,
    the device-count entries and the front)."""

    def __init__(self, cap, max_push=0):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.g, self.cap = _bare_builder(cap), cap
        self.state = torch.empty(self.L.dagr_stream_state_bytes(B, cap), dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_reset(_lib.ptr(self.state), B, cap, _lib.cur_stream(self.dev)), "reset")
        self.pos = torch.zeros((cap, 3), device=self.dev)
        self.feat = torch.zeros((cap,), device=self.dev)
        self.batch = torch.zeros((cap,), dtype=torch.int32, device=self.dev)
        self.n_dev = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.lane_count = torch.zeros((B,), dtype=torch.int32, device=self.dev)
        self.lane_dropped = torch.zeros((B,), dtype=torch.int64, device=self.dev)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.out = (torch.zeros((cap, 16), dtype=torch.int32, device=self.dev),
                    torch.zeros((cap, 16), dtype=torch.int16, device=self.dev),
                    torch.zeros((cap,), dtype=torch.int32, device=self.dev))
        self.max_push = max_push
        if max_push:                    # the downsampling front and its survivors' buffers
            nbytes = self.L.dagr_stream_front_bytes(B, W, H, max_push)
            self.front = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            _lib.check(self.L.dagr_stream_front_reset(_lib.ptr(self.front), nbytes, B, W, H, max_push,
                                                      _lib.cur_stream(self.dev)), "front_reset")
            self.s_xy = torch.zeros((max_push, 2), dtype=torch.int16, device=self.dev)
            self.s_t = torch.zeros((max_push,), dtype=torch.int64, device=self.dev)
            self.s_p = torch.zeros((max_push,), dtype=torch.int8, device=self.dev)
            self.s_batch = torch.zeros((max_push,), dtype=torch.int32, device=self.dev)
            self.s_n = torch.full((1,), -1, dtype=torch.int32, device=self.dev)

    def _outputs(self):
        P = _lib.ptr
        return (P(self.pos), P(self.feat), P(self.batch), P(self.n_dev), P(self.lane_count), P(self.status),
                _lib.cur_stream(self.dev))

    def stage(self, s, N=None, dev_count=False, window_us=WINDOW_US):
        """dagr_stream_stage[_capped], or with dev_count dagr_stream_stage_dev[_capped] on the push as its own clock."""
        P = _lib.ptr
        n = len(s["t"])
        xy = _dev(np.stack([s["x"], s["y"]], -1).astype(np.int16).reshape(-1, 2))
        t, p, batch = _dev(s["t"]), _dev(s["p"]), _dev(s["batch"])
        t_now = None if s["t_now"] is None else _dev(s["t_now"])
        cap_args = () if N is None else (N, P(self.lane_dropped))
        head = (ctypes.byref(self.g.desc), P(self.g.workspace), P(self.state), B, self.cap)
        if not dev_count:
            fn = self.L.dagr_stream_stage if N is None else self.L.dagr_stream_stage_capped
            return fn(*head, P(xy), P(t), P(p), P(batch), 1, n, P(t_now), window_us, *cap_args, *self._outputs())
        fn = self.L.dagr_stream_stage_dev if N is None else self.L.dagr_stream_stage_dev_capped
        batch32, count = _dev(s["batch"].astype(np.int32)), _dev(np.array([n], np.int32))
        return fn(*head, P(xy), P(t), P(p), P(batch32), P(count), n, P(t), P(batch), 1, n, P(t_now), window_us, *cap_args,
                  *self._outputs())

    def stage_raw(self, s, N, window_us=WINDOW_US):
        """dagr_stream_downsample + dagr_stream_stage_dev_capped on a raw push."""
        P, st = _lib.ptr, _lib.cur_stream(self.dev)
        n = len(s["t"])
        xy = _dev(np.stack([s["x"], s["y"]], -1).astype(np.int16).reshape(-1, 2))
        t, p, batch = _dev(s["t"]), _dev(s["p"]), _dev(s["batch"])
        t_now = None if s["t_now"] is None else _dev(s["t_now"])
        rc = self.L.dagr_stream_downsample(P(self.front), self.front.numel(), B, self.max_push, F, F, F * W, F * H, W, H,
                                           P(xy), P(t), P(p), P(batch), 1, n, P(self.s_xy), P(self.s_t), P(self.s_p),
                                           P(self.s_batch), P(self.s_n), P(self.status), st)
        if rc:
            return rc
        return self.L.dagr_stream_stage_dev_capped(
            ctypes.byref(self.g.desc), P(self.g.workspace), P(self.state), B, self.cap, P(self.s_xy), P(self.s_t),
            P(self.s_p), P(self.s_batch), P(self.s_n), n, P(t), P(batch), 1, n, P(t_now), window_us, N,
            P(self.lane_dropped), *self._outputs())

    def build(self):
        self.g.build(self.pos, self.batch, out=self.out, n_dev=self.n_dev)


def _assert_staged(st, d, where, dropped=True):
    """The stager's outputs against the definition ``d``'s current window (``dropped``: and its dropped counts)."""
    pos, feat, batch = d.formatted()
    counts = d.counts()
    n = int(counts.sum())
    assert int(st.n_dev) == n, where
    assert st.lane_count.tolist() == counts.tolist(), where
    assert np.array_equal(st.pos[:n].cpu().numpy(), pos), where
    assert np.array_equal(st.feat[:n].cpu().numpy(), feat.reshape(-1)), where
    assert np.array_equal(st.batch[:n].cpu().numpy(), batch.astype(np.int32)), where
    if dropped:
        assert st.lane_dropped.dtype == torch.int64 and st.lane_dropped.tolist() == d.dropped.tolist(), where
    assert int(st.status) == 0, where


def _push_def(d, s):
    d.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])


# ------------------------------------------------------------------------------------------------------ 1
def test_capped_staging_equals_the_definition():
    """dagr_stream_stage_capped after every push of the scripted sequence (N = 257, capacity exactly B * N = 771 for the
    state AND the outputs): pos_out / feat_out / batch_out / *n_dev / lane_count / lane_dropped equal the definition, the
    status word stays 0, and the build continues from the staging as it does from dagr_stage_window."""
    N = cc.N_STAGE
    st, ref = _Stager(B * N), _Stager(B * N)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, max_lane_events=N)
    seq = cc.stage_sequence()
    assert max(len(s["t"]) for s in seq) > B * N
    for k, s in enumerate(seq):
        _push_def(d, s)
        _lib.check(st.stage(s, N), "stream_stage_capped")
        st.build()
        _assert_staged(st, d, k)
        # the same window through dagr_stage_window and the same build: the same edge count, flags and degrees
        pos, feat, batch = d.formatted()
        n = len(batch)
        w_pos, w_feat, w_batch = _dev(pos), _dev(feat.reshape(-1)), _dev(batch)
        _lib.check(st.L.dagr_stage_window(ctypes.byref(ref.g.desc), _lib.ptr(ref.g.workspace), _lib.ptr(w_pos),
                                          _lib.ptr(w_feat), _lib.ptr(w_batch), 1, n, *ref._outputs()[:4],
                                          _lib.cur_stream(st.dev)), "stage_window")
        ref.build()
        assert st.g.status() == ref.g.status(), k
        assert torch.equal(st.out[2][:n], ref.out[2][:n]), k
    assert d.dropped.sum() > 0 and d.counts().tolist() == [0, 0, 0]
    # lane_dropped may be NULL
    st2 = _Stager(B * N)
    d2 = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, max_lane_events=N)
    P = _lib.ptr
    for k, s in enumerate(seq[:3]):
        _push_def(d2, s)
        xy = _dev(np.stack([s["x"], s["y"]], -1).astype(np.int16).reshape(-1, 2))
        t, p, batch = _dev(s["t"]), _dev(s["p"]), _dev(s["batch"])
        _lib.check(st2.L.dagr_stream_stage_capped(ctypes.byref(st2.g.desc), P(st2.g.workspace), P(st2.state), B, st2.cap,
                                                  P(xy), P(t), P(p), P(batch), 1, len(s["t"]), None, WINDOW_US, N, None,
                                                  *st2._outputs()), "stream_stage_capped")
        st2.build()
        assert st2.lane_count.tolist() == d2.counts().tolist() and st2.lane_dropped.tolist() == [0, 0, 0], k
        assert np.array_equal(st2.pos[:int(st2.n_dev)].cpu().numpy(), d2.formatted()[0]), k


def test_an_empty_capped_push_on_a_lane_that_holds_more_than_the_cap():
    """An empty push with t_now where the time rule AND the count rule remove events.  A lane fed through the capped entry
    never holds more than N, so the lane is filled through dagr_stream_stage first (the state serves both entries): lane
    0 holds 600 events, the empty capped push expires its oldest by time and cuts the rest to N = 257."""
    N = cc.N_STAGE
    st = _Stager(B * N)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US)
    fill = cc.push({0: cc.chunk(syn.edges_window, 600, 71, 0, 10000), 2: cc.chunk(syn.uniform_window, 100, 72, 0, 10000)})
    _push_def(d, fill)
    _lib.check(st.stage(fill), "stream_stage")
    st.build()
    assert int(st.n_dev) == 700 and int(st.status) == 0
    d.max_lane_events = N                              # from here on the definition is the capped one
    empty = cc.push({}, t_now=[22000] * 3)
    _push_def(d, empty)
    by_time = int((fill["t"][fill["batch"] == 0] - T0 <= 2000).sum())
    assert 0 < by_time < 600 - N and d.dropped.tolist() == [600 - by_time - N, 0, 0]
    _lib.check(st.stage(empty, N), "stream_stage_capped")
    st.build()
    _assert_staged(st, d, "empty capped push")
    assert st.lane_count.tolist()[0] == N


# ------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("dev_count", [False, True], ids=["stream_stage", "stream_stage_dev"])
def test_the_uncapped_entries_give_what_they_gave(dev_count):
    """dagr_stream_stage and dagr_stream_stage_dev on the 8-push sequence of tests/test_streaming_gpu.py against the
    definition without a cap (this test uses nothing the cap added: it passes before and after); the dropped counters
    are not theirs to touch."""
    st = _Stager(4096)
    st.lane_dropped.fill_(7)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US)
    for k, s in enumerate(_sequence()):
        _push_def(d, s)
        _lib.check(st.stage(s, None, dev_count=dev_count), "stream_stage")
        st.build()
        assert st.lane_dropped.tolist() == [7, 7, 7], k
        _assert_staged(st, d, k, dropped=False)
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    small = _Stager(512)
    big = cc.push({1: cc.chunk(syn.uniform_window, 513, 24, 3000, 4000)})
    assert small.stage(big, None, dev_count=dev_count) == bad         # capacity < n_new is still refused here


# ------------------------------------------------------------------------------------------------------ 3
def _raw_chunk(gen, n, seed, t_lo, t_hi):
    """Raw events of the 640 x 430 sensor from ``n`` base events at the cell grid (tests/stream_downsample_cases.py: every
    base event repeated 3 to 6 times inside its cell, within 2 us), T0 + t_lo <= t <= T0 + t_hi + 2."""
    x, y, t, p = gen(n, W, H, seed, window_us=t_hi - t_lo, time_window=t_hi - t_lo)
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    rep = rng.integers(3, 7, len(t))
    x, y, t, p = (np.repeat(np.asarray(v), rep) for v in (x, y, t, p))
    m = len(t)
    x = x.astype(np.int64) * F + rng.integers(0, F, m)
    y = y.astype(np.int64) * F + rng.integers(0, F, m)
    t = np.int64(T0 + t_lo) + t.astype(np.int64) + rng.integers(0, 3, m)
    o = np.argsort(t, kind="stable")
    return x[o].astype(np.int16), y[o].astype(np.int16), t[o], p[o].astype(np.int8)


def test_behind_the_front_the_cap_counts_survivors():
    """dagr_stream_downsample + dagr_stream_stage_dev_capped on raw 640 x 430 pushes, N = 257 and capacity B * N, against
    StreamDefinition(downsample=2, max_lane_events=N).  The raw pushes (up to ~4 000 events) are larger than the capacity,
    lane 1 stays under the cap, lanes 0 and 2 are cut."""
    N = cc.N_STAGE
    E, U = syn.edges_window, syn.uniform_window
    seq = [cc.push({0: _raw_chunk(E, 500, 1, 0, 6000), 1: _raw_chunk(U, 37, 2, 0, 5000), 2: _raw_chunk(E, 300, 3, 0, 5500)}),
           cc.push({0: _raw_chunk(E, 150, 4, 6010, 9000), 2: _raw_chunk(U, 200, 5, 5510, 9000)}),
           cc.push({}, t_now=[24000] * 3),
           cc.push({0: _raw_chunk(E, 60, 6, 24000, 25000), 1: _raw_chunk(U, 50, 7, 24000, 25000),
                    2: _raw_chunk(E, 700, 1, 24000, 27000)}, t_now=[27500] * 3),
           cc.push({}, t_now=[90000] * 3)]
    assert max(len(s["t"]) for s in seq) > B * N
    st = _Stager(B * N, max_push=8192)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, downsample=F, max_lane_events=N)
    u = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, downsample=F)
    assert d.front == (F, F, F * W, F * H)
    drops = []
    for k, s in enumerate(seq):
        _push_def(d, s)
        _push_def(u, s)
        _lib.check(st.stage_raw(s, N), "stream_downsample + stream_stage_dev_capped")
        st.build()
        _assert_staged(st, d, k)
        assert np.array_equal(st.front[:4 * B * W * H].view(torch.float32).view(B, H, W).cpu().numpy(), d.change_map), k
        drops.append(d.dropped.copy())
        print(k, "raw", len(s["t"]), "uncapped", u.counts().tolist(), "capped", d.counts().tolist(), "dropped", drops[-1])
    assert drops[0][0] > 0 and drops[1][2] > drops[0][2] and drops[3][2] > drops[1][2] and drops[-1][1] == 0
    assert d.counts().tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------ 4
def _clone(dets):
    return [{n: v.clone() for n, v in d.items()} for d in dets]


def test_capped_stream_steps_equal_the_model_and_a_burst_costs_its_own_lane_only():
    """EventStream(window_us=20000, max_lane_events=300): step after every push == model(definition window, reset=True)[0]
    on the same engine, dropped() == the definition's, no status bit; and with a burst of 5 000 events into lane 1 the
    results of lanes 0 and 2 are those of the same sequence without it."""
    model = _model(B)
    eng = model.engine().set_low_latency(True)
    runs = {}
    for burst in (True, False):
        stream = EventStream(model, window_us=WINDOW_US, max_lane_events=cc.N_MODEL)
        d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, max_lane_events=cc.N_MODEL)
        runs[burst] = []
        assert stream.dropped().tolist() == [0, 0, 0] and stream.dropped().dtype == np.int64
        with torch.no_grad():
            for k, s in enumerate(cc.burst_sequence(burst)):
                _push_def(d, s)
                a, kw = _step_args(s)
                got = _clone(stream.step(*a, **kw))                 # (check_status inside: no bit is raised)
                assert stream.counts().tolist() == d.counts().tolist(), (burst, k)
                assert stream.dropped().tolist() == d.dropped.tolist(), (burst, k)
                pos, feat, batch = _window_dev(d.formatted())
                want = model(types.SimpleNamespace(pos=pos, x=feat, batch=batch), reset=True)[0]
                assert len(got) == len(want) == B
                for b in range(B):
                    for name in ("boxes", "scores", "labels"):
                        assert torch.equal(got[b][name], want[b][name]), (burst, k, b, name)
                runs[burst].append(got)
        stream.check_status()
        assert int(stream.state.status) == 0
        if burst:
            assert len(cc.burst_sequence(True)[3]["t"]) > 5000 > B * cc.N_MODEL and d.dropped[1] >= 4700
        else:
            assert d.dropped[1] == 0 and d.dropped[0] > 0 and d.dropped[2] > 0
        stream.reset()
        assert stream.dropped().tolist() == [0, 0, 0] and stream.counts().tolist() == [0, 0, 0]
    assert sum(len(g[b]["scores"]) for g in runs[True] for b in (0, 2)) > 0, "no detection in lanes 0 and 2"
    for k, (with_burst, without) in enumerate(zip(runs[True], runs[False])):
        for b in (0, 2):
            for name in ("boxes", "scores", "labels"):
                assert torch.equal(with_burst[b][name], without[b][name]), (k, b, name)


# ------------------------------------------------------------------------------------------------------ 5
def _steady_pushes(steps, per_lane):
    return [cc.push({b: cc.chunk(syn.edges_window if b != 1 else syn.uniform_window, per_lane + b, 300 + 3 * k + b,
                                 1000 * k, 1000 * k + 900) for b in range(B)}, t_now=[1000 * (k + 1)] * 3)
            for k in range(steps)]


def test_nothing_grows_over_sixty_steps_without_a_read_back():
    """60 step_device calls, about N / 3 events per lane each, nothing read back in between: from the step after the window
    graph's capture on, eng.max_events, the state's capacity and tensor, the engine's input buffer and the captured graph
    objects are the same; the last step's detections are reset=True's on the definition's window."""
    model = _model(B)
    eng = model.engine().set_low_latency(True)
    N = cc.N_MODEL
    stream = EventStream(model, window_us=WINDOW_US, max_lane_events=N)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, max_lane_events=N)
    allocs = []
    alloc = eng._alloc_events
    eng._alloc_events = lambda n: (allocs.append(n), alloc(n))[1]
    seen = []
    try:
        with torch.no_grad():
            for k, s in enumerate(_steady_pushes(60, N // 3)):
                _push_def(d, s)
                a, kw = _step_args(s)
                det, nk = stream.step_device(*a, **kw)
                assert stream.state.bound() <= B * N
                seen.append((eng.max_events, stream.state.cap, stream.state.state.data_ptr(), eng.in_pos.data_ptr(),
                             id(eng._wg), id(eng._graph), id(stream.state.state), eng._wg is not None))
            got = (det.clone(), nk.clone())
    finally:
        del eng._alloc_events
    assert allocs == [], allocs                      # B * N fits the engine's buffers: no call, not even on the first step
    captured = [k for k, row in enumerate(seen) if row[-1]]
    assert captured and captured[0] <= 3, "the window was not captured"
    assert len(set(seen[captured[0]:])) == 1, "a buffer or a graph changed after the capture"
    assert len({row[:4] for row in seen}) == 1, "a buffer changed after the first step"
    assert d.counts().tolist() == [N] * 3 and d.dropped.min() > 50 * (N // 3) - N
    _assert_same_detections(got, eng.forward_detections(*_window_dev(d.formatted())), B, "last step")
    assert stream.counts().tolist() == [N] * 3 and stream.dropped().tolist() == d.dropped.tolist()
    stream.check_status()


def test_a_small_engine_is_sized_once_for_a_capped_stream():
    """An engine smaller than B * N: one _alloc_events(B * N) on the first step, no doubling, and then nothing -- where an
    uncapped stream's bound (everything pushed since the last read-back) would pass the buffers again and again."""
    from dagr_amd.engine import StreamState, WindowEngine
    model = _model(B)
    eng = WindowEngine(model, max_events=1024).set_low_latency(True)
    N = 400                                          # B * N = 1200 > 1024
    st = StreamState(B, WINDOW_US, eng.device, max_lane_events=N)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, max_lane_events=N)
    seen = []
    with torch.no_grad():
        for k, s in enumerate(_steady_pushes(12, 250)):
            _push_def(d, s)
            _, (det, nk) = eng.forward_stream(st, _dev(np.stack([s["x"], s["y"]], -1)), _dev(s["t"]), _dev(s["p"]),
                                              _dev(s["batch"]), t_now=_dev(s["t_now"]))
            seen.append((eng.max_events, st.cap, st.state.data_ptr(), eng.in_pos.data_ptr()))
        got = (det.clone(), nk.clone())
    assert seen[0][:2] == (B * N, B * N) and len(set(seen)) == 1
    assert eng._wg is not None
    _assert_same_detections(got, eng.forward_detections(*_window_dev(d.formatted())), B, "last step")
    torch.cuda.synchronize()
    assert int(st.status) == 0 and st.lane_count.tolist() == d.counts().tolist() == [N] * 3
    assert st.dropped().tolist() == d.dropped.tolist()
    eng.check_status()


# ------------------------------------------------------------------------------------------------------ 6
def test_a_pure_count_window_stages_the_ncaltech101_sample(tmp_path):
    """EventStream(window_us=None, max_lane_events=1000) on a 240 x 180 model, the synthetic recording in 5 pushes, the
    last with t_now = t_last + 1: the engine's staged rows equal format_data of NCaltech101's sample bit for bit."""
    from dagr_amd.data import Batch
    from dagr_amd.model.networks.dagr import DAGR
    from dagr_amd.utils.buffers import format_data
    from dagr_amd.utils.testing_weights import randomize_
    rec = cc.recording()
    cc.write_recording(tmp_path, rec)
    ds, sample = cc.ncaltech_sample(tmp_path, 1000)
    torch.manual_seed(12)
    args = om.default_args(batch_size=1)
    model = randomize_(DAGR(args, height=ds.height, width=ds.width), seed=12).eval().cuda()
    model.cache_luts(width=ds.width, height=ds.height, radius=args.radius)
    model.conf_threshold, model.nms_threshold, model.check_device_status = 0.001, 0.65, True
    eng = model.engine()
    assert (eng.W, eng.H, eng.time_window) == (ds.width, ds.height, ds.time_window)
    stream = EventStream(model, window_us=None, max_lane_events=1000)
    assert stream.window_us == ds.time_window
    edges = [0, 411, 1000, 1001, 2500, 3000]
    with torch.no_grad():
        for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            last = k == len(edges) - 2
            stream.step(np.stack([rec["x"][lo:hi], rec["y"][lo:hi]], -1), rec["t"][lo:hi], rec["p"][lo:hi],
                        t_now=int(rec["t"][-1]) + 1 if last else None)
    assert stream.counts().tolist() == [1000] and stream.dropped().tolist() == [2000]
    want = format_data(Batch.from_data_list([sample]).cuda())
    assert want.pos.dtype == torch.float32 and tuple(want.pos.shape) == (1000, 3)
    assert float(want.pos[-1, 2]) == np.float32(ds.time_window - 1) / np.float32(ds.time_window)
    assert torch.equal(eng.in_pos[:1000], want.pos)
    assert torch.equal(eng.in_feat[:1000], want.x.reshape(-1))
    assert torch.equal(eng.in_batch[:1000], want.batch.to(torch.int32)) and int(eng.n_dev) == 1000


# ------------------------------------------------------------------------------------------------------ 7
def test_run_stream_script_with_a_cap(tmp_path):
    """scripts/run_stream.py --max_lane_events 300 on the synthetic stand-in source: the rows of detections_<sequence>.npy
    are those of stepping the definition's windows through model(..., reset=True)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    from dagr_amd.utils.buffers import detections_to_records
    model = _model(1)
    argv = ["--step_us", "1000", "--window_us", "5000", "--steps", "10", "--stream", "edges", "--width", str(W),
            "--height", str(H), "--events_per_window", "40000", "--output_directory", str(tmp_path), "--sequence", "capped",
            "--max_lane_events", "300"]
    a = C.flags("", argv, extra=R.stream_options)
    source = R.SyntheticStream(a)
    path = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    assert os.path.basename(str(path)) == "detections_capped.npy"
    rec = np.load(path)
    assert len(rec) > 0
    t0, t1 = source.t_range()
    d = StreamDefinition(1, W, H, time_window=TW, window_us=5000, max_lane_events=300)
    rows = pushed = 0
    with torch.no_grad():
        for t_step in range(t0 + 1000, t1 + 1, 1000):
            ev = source.events(t_step - 1000, t_step)
            d.push(ev["x"], ev["y"], ev["t"], ev["p"], t_now=t_step)
            pushed += len(ev["t"])
            assert d.counts().tolist() == [300]             # ~800 events per step: the cap is what sizes the window
            pos, feat, batch = _window_dev(d.formatted())
            det = model(types.SimpleNamespace(pos=pos, x=feat, batch=batch), reset=True)[0][0]
            want = detections_to_records({k: v.cpu() for k, v in det.items()}, np.uint64(t_step))
            got = rec[rec["t"] == t_step]
            assert len(got) == len(want) and got.tobytes() == want.tobytes(), t_step
            rows += len(got)
    assert rows == len(rec) and pushed > 7000 and d.dropped.tolist() == [pushed - 300]
