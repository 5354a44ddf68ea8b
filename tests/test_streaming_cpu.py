"""Event streams without a GPU: the numpy definition of a stream step (dagr_amd/streaming.py: StreamDefinition) on
hand-written cases, the three stream entry points in header, library and binding, the host-side argument checks of
dagr_stream_stage, what EventStream refuses, and run_stream.py's flags."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd.streaming import EventStream, StreamDefinition
from dagr_amd.utils import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = (1 << 33) + 12345          # absolute microseconds beyond int32
TW = 1000000


def _d(B=2, window_us=100):
    return StreamDefinition(B, 320, 215, time_window=TW, window_us=window_us)


def test_cut_is_half_open_and_splits_equal_timestamps_by_value():
    """t_ref - t == window_us leaves, window_us - 1 stays; two events with the same t sit on each side of the cut."""
    d = _d(B=1)
    t = T0 + np.array([0, 0, 1, 1, 60, 100])
    d.push([1, 2, 3, 4, 5, 6], [9, 8, 7, 6, 5, 4], t, [1, -1, 1, -1, 1, 1])
    # t_ref = T0 + 100: ages 100, 100 (leave), 99, 99 (stay), 40, 0
    x, y, t_rel, p, b = d.window()
    assert x.tolist() == [3, 4, 5, 6] and y.tolist() == [7, 6, 5, 4] and p.tolist() == [1, -1, 1, 1]
    assert t_rel.dtype == np.int32 and t_rel.tolist() == [TW - 99, TW - 99, TW - 40, TW]
    assert b.tolist() == [0, 0, 0, 0] and d.counts().tolist() == [4]
    pos, feat, batch = d.formatted()
    assert pos.dtype == np.float32 and np.array_equal(pos, syn.format_data_np(x, y, t_rel, 320, 215, TW))
    assert np.array_equal(feat, p.astype(np.float32).reshape(-1, 1)) and batch.dtype == np.int64


def test_time_jump_expires_a_whole_lane_and_what_left_never_comes_back():
    d = _d(B=2)
    d.push([1, 2, 3], [1, 2, 3], T0 + np.array([0, 50, 10]), [1, 1, -1], batch=[0, 0, 1])
    assert d.counts().tolist() == [2, 1]
    d.push([7], [7], [T0 + 5000], [1], batch=[0])          # lane 0 jumps, lane 1 receives nothing and keeps its t_ref
    x, y, t_rel, p, b = d.window()
    assert x.tolist() == [7, 3] and b.tolist() == [0, 1] and t_rel.tolist() == [TW, TW]
    d.push([], [], [], [], batch=[], t_now=T0 + 5050)      # lane 1's event is 5040 us old now
    assert d.counts().tolist() == [1, 0] and d.window()[2].tolist() == [TW - 50]


def test_a_lane_that_never_received_an_event():
    d = _d(B=3)
    d.push([4, 5], [4, 5], [T0, T0 + 1], [1, -1], batch=[0, 2])
    assert d.counts().tolist() == [1, 0, 1] and d.window()[4].tolist() == [0, 2]
    d.push([6], [6], [T0 + 2], [1], batch=[2], t_now=[T0 + 3] * 3)
    assert d.counts().tolist() == [1, 0, 2] and d.window()[2].tolist() == [TW - 3, TW - 2, TW - 1]
    assert d.formatted()[0].shape == (3, 3)


def test_t_now_ahead_of_the_newest_event_and_an_empty_push_that_moves_it():
    d = _d(B=1, window_us=50)
    d.push([1, 2], [1, 2], [T0, T0 + 30], [1, 1], t_now=T0 + 40)
    assert d.window()[2].tolist() == [TW - 40, TW - 10]
    d.push([], [], [], [], t_now=T0 + 50)                  # zero events, t_now moves: the first event is 50 us old
    assert d.counts().tolist() == [1] and d.window()[2].tolist() == [TW - 20]
    d.push([], [], [], [], t_now=T0 + 80)
    assert d.counts().tolist() == [0] and d.formatted()[0].shape == (0, 3)
    d.push([3], [3], [T0 + 80], [-1])                      # the stream goes on after an empty window
    assert d.window()[0].tolist() == [3] and d.window()[2].tolist() == [TW]


def test_the_definition_refuses_malformed_pushes():
    d = _d(B=2)
    d.push([1, 2], [1, 2], [T0 + 10, T0 + 20], [1, 1], batch=[0, 1])
    with pytest.raises(ValueError, match="backwards"):
        d.push([1, 1], [1, 1], [T0 + 40, T0 + 30], [1, 1], batch=[0, 0])        # inside a push
    with pytest.raises(ValueError, match="backwards"):
        d.push([1], [1], [T0 + 5], [1], batch=[0])                              # against the lane's newest event
    with pytest.raises(ValueError, match="t_now"):
        d.push([1], [1], [T0 + 50], [1], batch=[0], t_now=[T0 + 49, T0 + 49])   # behind the newest event
    d.push([], [], [], [], batch=[], t_now=[T0 + 60, T0 + 60])
    with pytest.raises(ValueError, match="t_now"):
        d.push([], [], [], [], batch=[], t_now=[T0 + 59, T0 + 60])              # behind the previous t_ref
    with pytest.raises(ValueError, match="batch"):
        d.push([1, 1], [1, 1], [T0 + 70, T0 + 70], [1, 1], batch=[1, 0])
    with pytest.raises(ValueError, match="batch"):
        d.push([1], [1], [T0 + 70], [1], batch=[2])
    assert d.counts().tolist() == [1, 1]                                        # a refused push changes nothing
    with pytest.raises(ValueError, match="window_us"):
        StreamDefinition(1, 320, 215, time_window=1000, window_us=1001)


STREAM_FUNCTIONS = ("dagr_stream_state_bytes", "dagr_stream_reset", "dagr_stream_stage")


def test_stream_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dagr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dagr_[A-Za-z0-9_]+)\s*\(", src))
    L = _lib.lib()
    for n in STREAM_FUNCTIONS:
        assert n in declared, f"{n} is not declared in dagr_hip.h"
        assert hasattr(L, n), f"{n} declared in dagr_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} declared in dagr_hip.h but not bound in dagr_amd/_lib.py"
    res, args = _lib.SIGNATURES["dagr_stream_stage"]
    assert res is ctypes.c_int and len(args) == 20 and args[0] is ctypes.POINTER(_lib.GraphDesc)
    assert args[12] is ctypes.c_int64 and args[10] is ctypes.c_int64          # window_us, n_new
    assert _lib.SIGNATURES["dagr_stream_state_bytes"] == (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int64])


def test_stream_stage_rejects_bad_arguments_before_any_launch():
    """Rejected on the host, so this runs without a GPU: no pointer below is ever dereferenced."""
    L = _lib.lib()
    d = _lib.GraphDesc(width=320, height=215, batch_size=3, max_neighbors=16, queue_size=128, radius=4, delta_t_us=10000,
                       time_window=TW, max_events=4096)
    one = ctypes.c_void_p(256)
    # two raw sets of 13 bytes per event, plus the lanes' bounds
    assert L.dagr_stream_state_bytes(3, 4096) >= 2 * 13 * 4096
    assert L.dagr_stream_state_bytes(3, 8192) - L.dagr_stream_state_bytes(3, 4096) == 2 * 13 * 4096
    assert L.dagr_stream_state_bytes(0, 4096) == 0 and L.dagr_stream_state_bytes(3, 0) == 0

    def stage(desc=d, B=3, capacity=4096, n_new=16, window_us=50000, state=one, xy=one, status=one):
        return L.dagr_stream_stage(ctypes.byref(desc), one, state, B, capacity, xy, one, one, one, 0, n_new, None, window_us,
                                   one, one, one, one, one, status, None)
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    assert stage(window_us=0) == bad and b"window_us" in L.dagr_last_error()
    assert stage(window_us=-5) == bad
    assert stage(window_us=TW + 1) == bad and b"window_us" in L.dagr_last_error()
    assert stage(capacity=15) == bad and b"capacity < n_new" in L.dagr_last_error()
    assert stage(capacity=4097) == bad and b"max_events" in L.dagr_last_error()
    assert stage(state=None) == bad and b"NULL" in L.dagr_last_error()
    assert stage(status=None) == bad and b"NULL" in L.dagr_last_error()
    assert stage(xy=None) == bad and b"NULL" in L.dagr_last_error()
    assert stage(B=2) == bad and b"batch_size" in L.dagr_last_error()
    assert L.dagr_stream_reset(None, 3, 4096, None) == bad


def test_event_stream_refuses_a_cpu_model_and_a_window_beyond_the_time_axis():
    from oracle import model as om
    from dagr_amd.model.networks.dagr import DAGR
    model = DAGR(om.default_args(batch_size=1), height=215, width=320).eval()
    with pytest.raises(ValueError, match="window_us"):
        EventStream(model, window_us=TW + 1)
    with pytest.raises(ValueError, match="window_us"):
        EventStream(model, window_us=0)
    with pytest.raises(RuntimeError, match="GPU"):
        EventStream(model, window_us=50000)
    with pytest.raises(RuntimeError, match="eval"):
        EventStream(model.train(), window_us=50000)


def test_run_stream_flags_parse():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    a = C.flags("", [], extra=R.stream_options)
    assert (a.step_us, a.window_us, a.sequence) == (1000, 50000, "synthetic_stream")
    a = C.flags("", ["--config", "dagr-s", "--step_us", "500", "--window_us", "20000", "--steps", "7", "--stream", "edges",
                     "--width", "320", "--height", "215", "--events_per_window", "4000"], extra=R.stream_options)
    assert (a.step_us, a.window_us, a.steps, a.stream, a.net_stem_width) == (500, 20000, 7, "edges", 0.5)
    s = R.SyntheticStream(a)
    t0, t1 = s.t_range()
    assert t1 - t0 == 3500 and t0 >= 1 << 33 and np.all(np.diff(s.t) >= 0)
    ev = s.events(t0 + 500, t0 + 1000)
    assert len(ev["t"]) > 0 and ev["t"].min() >= t0 + 500 and ev["t"].max() < t0 + 1000 and ev["t"].dtype == np.int64
    assert callable(R.main)
