"""The capped event stream without a GPU: StreamDefinition(max_lane_events=N) against a brute-force restatement that keeps
every event ever pushed, applies the time rule and takes the last N (tests/stream_cap_cases.py: BruteForce), chunking
invariance, the N-Caltech101 identity through NCaltech101's own preprocessing, what the constructors refuse, the capped
entry points in header, library and binding with their host-side argument checks, and run_stream.py's flag."""
import ctypes
import os
import sys

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd.streaming import EventStream, StreamDefinition
from dagr_amd.utils import synthetic as syn
from tests import stream_cap_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B, TW, T0 = cc.W, cc.H, cc.B, cc.TW, cc.T0


def _run(seq, N, window_us=cc.WINDOW_US, check_every_push=True):
    """The definition and the brute force through a sequence; (definition, dropped after every push)."""
    d = StreamDefinition(B, W, H, time_window=TW, window_us=window_us, max_lane_events=N)
    bf = cc.BruteForce(B, d.window_us, N)
    dropped = []
    for k, s in enumerate(seq):
        d.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
        bf.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
        if check_every_push:
            assert cc.same_window(d.window(), bf.window()), k
            assert d.dropped.dtype == np.int64 and d.dropped.tolist() == bf.dropped().tolist(), k
            assert np.all(d.counts() <= N), k
        dropped.append(d.dropped.copy())
    return d, dropped


def test_the_capped_definition_equals_the_brute_force_after_every_push():
    for seq, N in ((cc.stage_sequence(), cc.N_STAGE), (cc.burst_sequence(True), cc.N_MODEL),
                   (cc.burst_sequence(False), cc.N_MODEL)):
        d, dropped = _run(seq, N)
        assert dropped[-1].sum() > 0
        pos, feat, batch = d.formatted()
        x, y, t_rel, p, b = d.window()
        assert np.array_equal(pos, syn.format_data_np(x, y, t_rel, W, H, TW)) and np.array_equal(batch, b)


def test_the_staging_sequence_holds_what_it_is_meant_to():
    seq, N = cc.stage_sequence(), cc.N_STAGE
    d = StreamDefinition(B, W, H, time_window=TW, window_us=cc.WINDOW_US, max_lane_events=N)
    u = StreamDefinition(B, W, H, time_window=TW, window_us=cc.WINDOW_US)         # the time rule alone
    counts, dropped, uncapped, t_rel = [], [], [], []
    for s in seq:
        for dd in (d, u):
            dd.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
        counts.append(d.counts().tolist())
        dropped.append(d.dropped.tolist())
        uncapped.append(u.counts().tolist())
        t_rel.append(d.window()[2])
    step = np.diff(np.array([[0, 0, 0]] + dropped), axis=0)
    assert all(c[1] < N for c in counts) and all(row[1] == 0 for row in dropped)      # lane 1 stays under N
    assert counts[0] == [200, 37, 150] and dropped[0] == [0, 0, 0]
    assert counts[1] == [N, 37, 200] and step[1].tolist() == [93, 0, 0]               # cut inside lane 0's survivors
    assert counts[2][2] == N and step[2][2] == 200 + 143                              # no survivor stays, first_new moves
    # push 3, lane 0: the time rule removes survivors (fewer than the 257 stay of 257 + 120) and the count rule removes more
    assert 0 < step[3][0] < 120 and counts[3][0] == N and len(seq[3]["t"]) == 120 and counts[3][1] == 0
    assert len(seq[4]["t"]) == 0 and counts[4][0] < counts[3][0] and counts[4][2] < counts[3][2] and step[4].sum() == 0
    assert len(seq[5]["t"]) == 920 > B * N and counts[5] == [N, 20, N]
    cut_t = t_rel[6]                 # push 6: lane 0's oldest kept event shares its timestamp with a dropped one
    assert counts[6][0] == N and step[6][0] == N + 300 - N
    t6 = seq[6]["t"]
    assert t6[300 - N - 1] == t6[300 - N], "the count cut does not fall between equal timestamps"
    assert cut_t[0] == TW - (int(t6[-1]) - int(t6[300 - N]))
    assert counts[7] == [0, 0, 0]
    for c in counts:                        # no lane boundary on a multiple of the block size
        for edge in np.cumsum(c)[:-1]:
            assert edge % 256 != 0 or edge == 0 or c == [0, 0, 0], c
    assert any(sum(c) > 256 for c in counts)                                          # more than one block of the gather
    assert max(sum(c) for c in uncapped) > B * N                                      # the time rule alone would not fit


@pytest.mark.parametrize("pushes", [1, 3, 17])
def test_chunking_invariance(pushes):
    """The same event sequence as 1, 3 and 17 pushes, the same final t_now: the same window.  (dropped differs: what a
    coarser chunking never saw inside the window, a finer one has counted.)"""
    n = [1900, 140, 777]
    lanes = []
    for b in range(B):
        x, y, t, p = cc.chunk(syn.edges_window, n[b], 60 + b, 0, 30000)
        lanes.append((x, y, (t - T0) // 5 * 5 + T0, p))                              # runs of equal timestamps
    t_end = 31000
    edges = np.linspace(0, t_end, pushes + 1).astype(np.int64)
    d = StreamDefinition(B, W, H, time_window=TW, window_us=cc.WINDOW_US, max_lane_events=cc.N_MODEL)
    for lo, hi in zip(edges[:-1], edges[1:]):
        parts = {}
        for b, (x, y, t, p) in enumerate(lanes):
            m = (t - T0 >= lo) & (t - T0 < hi)
            if m.any():
                parts[b] = (x[m], y[m], t[m], p[m])
        s = cc.push(parts, t_now=[int(hi)] * 3)
        d.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
    one = cc.BruteForce(B, cc.WINDOW_US, cc.N_MODEL)
    s = cc.push(dict(enumerate(lanes)), t_now=[t_end] * 3)
    one.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
    assert cc.same_window(d.window(), one.window())
    assert d.counts().tolist() == [cc.N_MODEL, sum(lanes[1][2] - T0 > t_end - cc.WINDOW_US), cc.N_MODEL]


def test_a_cap_of_one_event():
    d, dropped = _run(cc.stage_sequence(), 1)
    assert dropped[5].tolist() == [200 + 150 + 120 + 500 - 1, 37 + 20 - 2, 150 + 50 + 400 + 400 - 2]      # (lanes 1 and 2 lose one resident event to the time rule)
    d, _ = _run(cc.stage_sequence()[:6], 1)
    s = cc.stage_sequence()[5]
    assert d.counts().tolist() == [1, 1, 1]
    assert d.window()[0].tolist() == [s["x"][s["batch"] == b][-1] for b in range(B)]
    assert d.window()[2].tolist() == [TW] * 3


def test_a_cap_equal_to_the_lanes_count_drops_nothing():
    seq = cc.stage_sequence()[:2]                      # lane 0 holds 350 events after these, all inside the window
    d, dropped = _run(seq, 350)
    assert d.counts().tolist() == [350, 37, 200] and dropped[-1].tolist() == [0, 0, 0]
    d, dropped = _run(seq, 349)
    assert d.counts().tolist() == [349, 37, 200] and dropped[-1].tolist() == [1, 0, 0]


def test_equal_timestamps_are_cut_by_arrival_order():
    d = StreamDefinition(1, W, H, time_window=TW, window_us=100, max_lane_events=3)
    d.push([1, 2, 3, 4, 5], [9, 8, 7, 6, 5], T0 + np.array([10, 20, 20, 20, 20]), [1, -1, 1, -1, 1])
    x, y, t_rel, p, b = d.window()
    assert x.tolist() == [3, 4, 5] and y.tolist() == [7, 6, 5] and t_rel.tolist() == [TW] * 3 and d.dropped.tolist() == [2]
    d.push([6], [4], [T0 + 20], [1], t_now=T0 + 119)          # the time rule keeps all four (age 99), the cap three
    assert d.window()[0].tolist() == [4, 5, 6] and d.window()[2].tolist() == [TW - 99] * 3 and d.dropped.tolist() == [3]
    d.push([], [], [], [], t_now=T0 + 120)                    # age 100: all leave by time, nothing more is dropped
    assert d.counts().tolist() == [0] and d.dropped.tolist() == [3]
    d.reset()
    assert d.dropped.tolist() == [0]


def test_without_a_cap_the_definition_is_todays():
    """max_lane_events=None on the existing 8-push sequence of tests/test_streaming_gpu.py: the brute force without a cap
    is the time rule on everything ever pushed, which is what the definition was before the cap."""
    from tests.test_streaming_gpu import _sequence
    d = StreamDefinition(B, W, H, time_window=TW, window_us=cc.WINDOW_US, max_lane_events=None)
    plain = StreamDefinition(B, W, H, time_window=TW, window_us=cc.WINDOW_US)
    bf = cc.BruteForce(B, cc.WINDOW_US, None)
    for k, s in enumerate(_sequence()):
        for dd in (d, plain, bf):
            dd.push(s["x"], s["y"], s["t"], s["p"], s["batch"], t_now=s["t_now"])
        assert cc.same_window(d.window(), bf.window()) and cc.same_window(d.window(), plain.window()), k
        assert d.dropped.tolist() == [0, 0, 0], k
    assert d.max_lane_events is None


def test_a_pure_count_window_is_the_ncaltech101_sample(tmp_path):
    """window_us=None, max_lane_events=num_events, the last step with t_now = t_last + 1: the window is
    NCaltech101.preprocess of the last num_events events, t - (t_last - time_window + 1)."""
    rec = cc.recording()
    cc.write_recording(tmp_path, rec)
    ds, sample = cc.ncaltech_sample(tmp_path, 1000)
    assert len(rec["t"]) == 3000 and sample.pos.shape == (1000, 2)
    d = StreamDefinition(1, ds.width, ds.height, time_window=ds.time_window, window_us=None, max_lane_events=1000)
    assert d.window_us == ds.time_window
    edges = [0, 411, 1000, 1001, 2500, 3000]
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        last = k == len(edges) - 2
        d.push(rec["x"][lo:hi], rec["y"][lo:hi], rec["t"][lo:hi], rec["p"][lo:hi],
               t_now=int(rec["t"][-1]) + 1 if last else None)
    x, y, t_rel, p, b = d.window()
    assert d.counts().tolist() == [1000] and d.dropped.tolist() == [2000]
    assert np.array_equal(np.stack([x, y], -1), sample.pos.numpy()) and sample.pos.numpy().dtype == np.int16
    assert t_rel.dtype == np.int32 and np.array_equal(t_rel, sample.t.numpy()) and t_rel[-1] == ds.time_window - 1
    assert np.array_equal(p, sample.x.numpy().reshape(-1))
    assert np.array_equal(d.formatted()[0], syn.format_data_np(sample.pos[:, 0].numpy(), sample.pos[:, 1].numpy(),
                                                               sample.t.numpy(), ds.width, ds.height, ds.time_window))


def test_the_constructors_refuse_a_count_window_without_a_cap_and_a_bad_cap():
    with pytest.raises(ValueError, match="needs max_lane_events"):
        StreamDefinition(1, W, H, window_us=None)
    for bad in (0, -3, 2.5, "7", True):
        with pytest.raises(ValueError, match="max_lane_events"):
            StreamDefinition(1, W, H, max_lane_events=bad)
    with pytest.raises(ValueError, match="capacity"):
        StreamDefinition(3, W, H, max_lane_events=(1 << 25) // 3 + 1)
    with pytest.raises(ValueError, match="window_us"):
        StreamDefinition(1, W, H, time_window=1000, window_us=1001, max_lane_events=5)
    assert StreamDefinition(2, W, H, time_window=1234, window_us=None, max_lane_events=np.int64(5)).window_us == 1234
    from oracle import model as om
    from dagr_amd.model.networks.dagr import DAGR
    model = DAGR(om.default_args(batch_size=1), height=H, width=W).eval()
    with pytest.raises(ValueError, match="needs max_lane_events"):
        EventStream(model, window_us=None)
    with pytest.raises(ValueError, match="max_lane_events"):
        EventStream(model, window_us=50000, max_lane_events=0)
    with pytest.raises(RuntimeError, match="GPU"):            # a valid cap: the next refusal is the CPU model
        EventStream(model, window_us=None, max_lane_events=1000)


def test_the_capped_entry_points_are_bound_and_check_their_arguments_before_any_launch():
    """Rejected on the host, so this runs without a GPU: no pointer below is ever dereferenced."""
    L = _lib.lib()
    for name, plain in (("dagr_stream_stage_capped", "dagr_stream_stage"),
                        ("dagr_stream_stage_dev_capped", "dagr_stream_stage_dev")):
        assert hasattr(L, name) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        res0, args0 = _lib.SIGNATURES[plain]
        k = len(args0) - 7                  # ... window_us | max_lane_events, lane_dropped | the seven outputs
        assert res is res0 and args[:k] == args0[:k] and args[k + 2:] == args0[k:]
        assert args[k] is ctypes.c_int64 and args[k + 1] is ctypes.c_void_p
    d = _lib.GraphDesc(width=W, height=H, batch_size=3, max_neighbors=16, queue_size=128, radius=4, delta_t_us=10000,
                       time_window=TW, max_events=4096)
    one = ctypes.c_void_p(256)
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]

    def stage(capacity=4096, n_new=16, N=1000, window_us=50000, dropped=one):
        return L.dagr_stream_stage_capped(ctypes.byref(d), one, one, 3, capacity, one, one, one, one, 0, n_new, None,
                                          window_us, N, dropped, one, one, one, one, one, one, None)

    def stage_dev(capacity=4096, n_new=16, n_clock=16, N=1000):
        return L.dagr_stream_stage_dev_capped(ctypes.byref(d), one, one, 3, capacity, one, one, one, one, one, n_new, one,
                                              one, 0, n_clock, None, 50000, N, one, one, one, one, one, one, one, None)
    assert stage(N=0) == bad and b"max_lane_events" in L.dagr_last_error()
    assert stage(N=-1) == bad and stage_dev(N=0) == bad
    assert stage(N=1366) == bad and b"B * max_lane_events" in L.dagr_last_error()        # 3 * 1366 = 4098 > 4096
    assert stage_dev(N=1366) == bad and b"B * max_lane_events" in L.dagr_last_error()
    assert stage(capacity=4097) == bad and b"max_events" in L.dagr_last_error()
    assert stage(window_us=TW + 1) == bad and b"window_us" in L.dagr_last_error()
    assert stage(n_new=-1) == bad and stage(n_new=1 << 30) == bad and b"n_new" in L.dagr_last_error()
    assert stage_dev(n_clock=1 << 30) == bad and b"n_clock" in L.dagr_last_error()
    # the uncapped entry still refuses a push above its capacity
    assert L.dagr_stream_stage(ctypes.byref(d), one, one, 3, 15, one, one, one, one, 0, 16, None, 50000, one, one, one, one,
                               one, one, None) == bad and b"capacity < n_new" in L.dagr_last_error()


def test_run_stream_takes_the_cap():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    a = C.flags("", [], extra=R.stream_options)
    assert a.max_lane_events is None and a.window_us == 50000
    a = C.flags("", ["--max_lane_events", "300", "--window_us", "0"], extra=R.stream_options)
    assert (a.max_lane_events, a.window_us) == (300, 0)
    with pytest.raises(SystemExit, match="window_us"):
        R.main(["--window_us", "0"])
    with pytest.raises(SystemExit, match="max_lane_events"):
        R.main(["--max_lane_events", "0"])
