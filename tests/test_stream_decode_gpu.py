"""The camera-word decoder on the GPU: dagr_stream_decode through the binding against the sequential loop
(dagr_amd/streaming.py: DecodeDefinition) over every case of tests/stream_decode_cases.py -- rows, count, padding rows,
counters, states and status bits --, the same streams cut into two and three pushes, max_out below the emit count, and
the staging entries that read the clock's length from the device against the ones that take it from the host.  Every
comparison is exact equality."""
import ctypes

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.streaming import DECODE_COUNTERS, DECODE_FORMATS, DECODE_STATE, DecodeDefinition, StreamDefinition
from tests import stream_decode_cases as dc
from tests.test_stream_cap_gpu import B, H, TW, W, WINDOW_US, _Stager, _assert_staged, _push_def
from tests.test_streaming_gpu import _dev, _sequence

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in dc.all_cases()}
BAD = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]


class _Decoder:
    """dagr_stream_decode on a state of its own; state and outputs start out as garbage."""

    def __init__(self, B, fmt, sensor, max_words, max_out, t_base=None):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.fmt, self.sensor, self.max_words, self.max_out = B, fmt, sensor, max_words, max_out
        nbytes = self.L.dagr_stream_decode_bytes(B, max_words)
        assert nbytes >= 64 * B
        self.state = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_decode_reset(_lib.ptr(self.state), nbytes, B, max_words, _lib.cur_stream(self.dev)),
                   "decode_reset")
        self.xy = torch.full((max_out + 5, 2), 77, dtype=torch.int16, device=self.dev)
        self.t = torch.full((max_out + 5,), 77, dtype=torch.int64, device=self.dev)
        self.p = torch.full((max_out + 5,), 77, dtype=torch.int8, device=self.dev)
        self.batch = torch.full((max_out + 5,), 77, dtype=torch.int32, device=self.dev)
        self.n = torch.full((1,), -1, dtype=torch.int32, device=self.dev)
        self.counts = torch.zeros((B, 4), dtype=torch.int64, device=self.dev)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.t_base = None if t_base is None else _dev(np.asarray(t_base, np.int64))

    def push(self, words, lane_words, max_out=None, word_end=None):
        P = _lib.ptr
        w = _dev(np.ascontiguousarray(words).view(np.int16 if self.fmt == "evt3" else np.int32)) if len(words) else None
        end = _dev(np.cumsum(lane_words).astype(np.int64) if word_end is None else np.asarray(word_end, np.int64))
        return self.L.dagr_stream_decode(P(self.state), self.state.numel(), self.B, self.max_words, DECODE_FORMATS[self.fmt][0],
                                         *self.sensor, P(w), P(end), len(words), P(self.t_base),
                                         self.max_out if max_out is None else max_out, P(self.xy), P(self.t), P(self.p),
                                         P(self.batch), P(self.n), P(self.counts), P(self.status), _lib.cur_stream(self.dev))

    def lane_states(self):
        s = self.state[:64 * self.B].view(torch.int64).view(self.B, 8).cpu().numpy()
        assert not s[:, 7].any()
        return {k: s[:, i] for i, k in enumerate(DECODE_STATE)}

    def rows(self):
        n = int(self.n)
        xy = self.xy[:n].cpu().numpy()
        return xy[:, 0], xy[:, 1], self.t[:n].cpu().numpy(), self.p[:n].cpu().numpy(), self.batch[:n].cpu().numpy()

    def assert_equals(self, d, want, where, max_out=None):
        """The last push's rows against ``want`` and everything carried against the definition ``d``."""
        max_out = self.max_out if max_out is None else max_out
        n = len(want[0])
        assert int(self.n) == n, where
        for got, ref in zip(self.rows(), want):
            assert got.dtype == ref.dtype and np.array_equal(got, ref), where
        assert np.all(self.batch[n:max_out].cpu().numpy() == -1) and not self.xy[n:max_out].any(), where    # lane-less rows
        assert np.all(self.batch[max_out:].cpu().numpy() == 77) and np.all(self.t[max_out:].cpu().numpy() == 77), where
        got = self.counts.cpu().numpy()
        for i, k in enumerate(DECODE_COUNTERS):
            assert np.array_equal(got[:, i], d.counts[k]), (where, k)
        for k, v in self.lane_states().items():
            assert np.array_equal(v, d.state[k]), (where, k)
        assert int(self.status) == d.status, where


def _pair(case, max_out=None, t_base=None):
    worst = DECODE_FORMATS[case["format"]][2] * max(len(case["words"]), 1)
    dec = _Decoder(case["B"], case["format"], case["sensor"], max(len(case["words"]), 1) + 3, max_out or worst, t_base)
    return dec, DecodeDefinition(case["B"], case["format"], *case["sensor"], t_base=t_base, max_out=max_out)


@pytest.mark.parametrize("name", list(CASES))
def test_decode_equals_the_definition(name):
    case = CASES[name]
    t_base = (np.arange(case["B"], dtype=np.int64) + 1) << 40
    dec, d = _pair(case, t_base=t_base)
    assert not any(v.any() for v in dec.lane_states().values())
    want = d.push(case["words"], case["lane_words"])
    _lib.check(dec.push(case["words"], case["lane_words"]), "stream_decode")
    dec.assert_equals(d, want, name)
    if case["events"] is not None:
        assert np.array_equal(want[2], case["events"][2] + t_base[case["events"][4]]) and len(want[2]) > 0
    # the same words again, on the state the first push left
    want = d.push(case["words"], case["lane_words"])
    _lib.check(dec.push(case["words"], case["lane_words"]), "stream_decode")
    dec.assert_equals(d, want, (name, "again"))
    # t_base may be NULL, lane_counts too; reset zeroes the states
    _lib.check(dec.L.dagr_stream_decode_reset(_lib.ptr(dec.state), dec.state.numel(), dec.B, dec.max_words,
                                              _lib.cur_stream(dec.dev)), "decode_reset")
    assert not any(v.any() for v in dec.lane_states().values())


CUT_CASES = ["a_encoded-evt3-640x480", "a_encoded-evt2-64x48", "c_late_wrap-evt3-64x48", "d_unsynced-evt3-64x48",
             "g_lanes-evt3-640x480", "b_carried_base-evt3-32767x48", "h_len%d-evt3-64x48" % (3 * dc.T + 5)]


@pytest.mark.parametrize("name", CUT_CASES)
def test_any_chunking_gives_the_same_rows_counters_and_states(name):
    """~40 seeded cuts of every lane's run into two and into three pushes: the pushes' rows, regrouped by lane, are the
    whole stream's, and so are the counters and the final states."""
    case = CASES[name]
    whole = DecodeDefinition(case["B"], case["format"], *case["sensor"])
    want = whole.push(case["words"], case["lane_words"])
    starts = np.concatenate([[0], np.cumsum(case["lane_words"])])
    rng = np.random.default_rng(5)
    worst = DECODE_FORMATS[case["format"]][2] * len(case["words"])
    dec = _Decoder(case["B"], case["format"], case["sensor"], len(case["words"]), worst)
    for trial in range(40):
        parts = 2 + trial % 2
        cuts = np.sort(rng.integers(0, case["lane_words"] + 1, (parts - 1, case["B"])), axis=0)      # per lane
        if trial < 4:           # the tile boundaries themselves
            cuts[:] = np.minimum(case["lane_words"], dc.T * (trial // 2 + 1) - trial % 2)
            cuts.sort(axis=0)
        edges = np.concatenate([np.zeros((1, case["B"]), np.int64), cuts, case["lane_words"][None]])
        _lib.check(dec.L.dagr_stream_decode_reset(_lib.ptr(dec.state), dec.state.numel(), dec.B, dec.max_words,
                                                  _lib.cur_stream(dec.dev)), "decode_reset")
        dec.counts.zero_()
        got = []
        for k in range(parts):
            lane_words = edges[k + 1] - edges[k]
            words = np.concatenate([case["words"][starts[b] + edges[k][b]:starts[b] + edges[k + 1][b]] for b in range(case["B"])])
            _lib.check(dec.push(words, lane_words), "stream_decode")
            got.append(dec.rows())
        rows = [np.concatenate(v) for v in zip(*got)]
        order = np.argsort(rows[4], kind="stable")
        for g, ref in zip(rows, want):
            assert np.array_equal(g[order], ref), (name, trial)
        counts = dec.counts.cpu().numpy()
        assert all(np.array_equal(counts[:, i], whole.counts[k]) for i, k in enumerate(DECODE_COUNTERS)), (name, trial)
        assert all(np.array_equal(v, whole.state[k]) for k, v in dec.lane_states().items()), (name, trial)
        assert int(dec.status) == whole.status, (name, trial)
        dec.status.zero_()


def test_max_out_below_the_emit_count():
    """Bit 6, the first max_out rows, lane-less rows nowhere (the buffer is full), and the state as if unbounded."""
    case = CASES["i_full_vectors-evt3-640x480"]
    full = DecodeDefinition(1, "evt3", *case["sensor"])
    full.push(case["words"])
    for max_out in (100, 479, 480, 1):
        dec, d = _pair(case, max_out=max_out)
        want = d.push(case["words"], case["lane_words"])
        _lib.check(dec.push(case["words"], case["lane_words"]), "stream_decode")
        dec.assert_equals(d, want, max_out)
        assert int(dec.status) == (64 if max_out < 480 else 0) and len(want[0]) == min(max_out, 480)
        assert all(np.array_equal(v, full.state[k]) for k, v in dec.lane_states().items())
        assert int(dec.counts[0, 0]) == 480


def test_refusals_and_a_bad_word_end():
    case = CASES["a_encoded-evt3-64x48"]
    dec, d = _pair(case)
    L, P, n = dec.L, _lib.ptr, len(case["words"])
    assert L.dagr_stream_decode_bytes(0, 16) == 0 and L.dagr_stream_decode_bytes(128, 16) == 0
    assert L.dagr_stream_decode_bytes(1, 0) == 0 and L.dagr_stream_decode_bytes(1, 1 << 25) == 0
    assert L.dagr_stream_decode_bytes(127, (1 << 25) - 1) > 0
    before = dec.state.clone()
    assert dec.push(case["words"], case["lane_words"], max_out=0) == BAD and b"max_out" in L.dagr_last_error()
    assert dec.push(case["words"], case["lane_words"], max_out=1 << 30) == BAD
    big = np.concatenate([case["words"]] * 2)
    assert dec.push(big, [len(big)]) == BAD and b"max_words" in L.dagr_last_error()
    odd = _dev(case["words"].view(np.int16))
    end = _dev(np.array([4], np.int64))
    args = (P(end), 4, None, dec.max_out, P(dec.xy), P(dec.t), P(dec.p), P(dec.batch), P(dec.n), P(dec.counts), P(dec.status),
            _lib.cur_stream(dec.dev))
    assert L.dagr_stream_decode(P(dec.state), dec.state.numel(), 1, dec.max_words, 2, 64, 48,
                                ctypes.c_void_p(odd.data_ptr() + 2), *args) == BAD and b"aligned" in L.dagr_last_error()
    assert L.dagr_stream_decode(P(dec.state), dec.state.numel(), 1, dec.max_words, 4, 64, 48, P(odd), *args) == BAD
    assert L.dagr_stream_decode(P(dec.state), 64, 1, dec.max_words, 3, 64, 48, P(odd), *args) == BAD
    assert L.dagr_stream_decode(None, dec.state.numel(), 1, dec.max_words, 3, 64, 48, P(odd), *args) == BAD
    assert torch.equal(dec.state, before) and int(dec.status) == 0 and int(dec.n) == -1
    # a word_end past n_words is clamped and flagged; nothing is read or written outside the buffers
    _lib.check(dec.push(case["words"], None, word_end=[n + 1000]), "stream_decode")
    want = d.push(case["words"], case["lane_words"])
    assert int(dec.status) == 8
    dec.status.zero_()
    dec.assert_equals(d, want, "clamped")
    lanes = CASES["g_lanes-evt3-640x480"]
    dec, d = _pair(lanes)
    end = np.cumsum(lanes["lane_words"])
    _lib.check(dec.push(lanes["words"], None, word_end=[end[0], end[0] - 7, end[2]]), "stream_decode")      # not non-decreasing
    want = d.push(lanes["words"], lanes["lane_words"])
    assert int(dec.status) == 8
    dec.status.zero_()
    dec.assert_equals(d, want, "decreasing")


# ------------------------------------------------------------------------------------------------ the clock on the device
class _ClockStager(_Stager):
    def __init__(self, cap):
        super().__init__(cap)
        self.state.fill_(0x5a)          # (the states are compared whole)
        _lib.check(self.L.dagr_stream_reset(_lib.ptr(self.state), B, cap, _lib.cur_stream(self.dev)), "reset")

    def stage_clock(self, s, N=None, pad=0, clock_count=True):
        """The ``_dev_clock`` entries on the push as its own clock, ``pad`` lane-less rows behind it and both counts on
        the device -- or with ``pad=None`` the ``_dev`` entries given ``n_clock = n``."""
        P, n = _lib.ptr, len(s["t"])
        m = n + (pad or 0)
        xy = np.zeros((m, 2), np.int16)
        xy[:n] = np.stack([s["x"], s["y"]], -1)
        t, p, batch = np.full(m, -5, np.int64), np.zeros(m, np.int8), np.full(m, -1, np.int32)
        t[:n], p[:n], batch[:n] = s["t"], s["p"], s["batch"]
        xy, t, p, batch, count = _dev(xy), _dev(t), _dev(p), _dev(batch), _dev(np.array([n], np.int32))
        t_now = None if s["t_now"] is None else _dev(s["t_now"])
        cap_args = () if N is None else (N, P(self.lane_dropped))
        head = (ctypes.byref(self.g.desc), P(self.g.workspace), P(self.state), B, self.cap, P(xy), P(t), P(p), P(batch), P(count), m,
                P(t), P(batch), 0)
        tail = (P(t_now), WINDOW_US, *cap_args, *self._outputs())
        if pad is None:
            fn = self.L.dagr_stream_stage_dev if N is None else self.L.dagr_stream_stage_dev_capped
            return fn(*head, n, *tail)
        fn = self.L.dagr_stream_stage_dev_clock if N is None else self.L.dagr_stream_stage_dev_clock_capped
        return fn(*head, P(count) if clock_count else None, m, *tail)


@pytest.mark.parametrize("N", [None, 257], ids=["uncapped", "capped"])
def test_the_clock_entries_equal_the_dev_entries(N):
    """*n_clock_dev = n equals n_clock = n, bit for bit on the outputs and on the stream state, with lane-less rows behind
    the count that a host-side n_clock would have flagged; dagr_stream_stage_dev itself still equals StreamDefinition."""
    cap = 4096
    a, b = _ClockStager(cap), _ClockStager(cap)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=WINDOW_US, **({} if N is None else dict(max_lane_events=N)))
    for k, s in enumerate(_sequence()):
        _push_def(d, s)
        _lib.check(a.stage_clock(s, N, pad=None), "stream_stage_dev")
        _lib.check(b.stage_clock(s, N, pad=9 + k), "stream_stage_dev_clock")
        a.build()
        b.build()
        _assert_staged(a, d, k, dropped=N is not None)
        for name in ("pos", "feat", "batch", "n_dev", "lane_count", "lane_dropped", "status", "state"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        assert a.g.status() == b.g.status(), k
    assert b.stage_clock(_sequence()[0], N, pad=3, clock_count=False) == BAD and b"n_clock_dev" in b.L.dagr_last_error()
