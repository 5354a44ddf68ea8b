"""The event stream's tracker on the GPU: dagr_stream_track through the binding against the numpy definition
(dagr_amd/streaming.py: TrackDefinition) step by step over every case of tests/stream_track_cases.py and over a seeded
random walk; EventStream(track=) against an untracked stream on the same pushes and against a TrackDefinition fed with every
step's own detections, in latency and in throughput mode; the same behind the frame steps and the held steps of a
--use_image model; the absence of host waits; the library calls of streams with and
without the tracker; and scripts/run_stream.py --track."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.streaming import TRACK_DTYPE, EventStream, TrackDefinition, _track_options
from dagr_amd.utils import synthetic as syn
from tests import stream_track_cases as tc
from tests.test_streaming_gpu import _chunk, _dev, _model, _push

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 3
WINDOW_US = 20000


# ------------------------------------------------------------------------------------------------ the kernel, case by case
class _Tracker:
    """dagr_stream_track on a state of its own; the state starts out as garbage in front of its reset, the outputs as -7."""

    def __init__(self, B_, A, track):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.A, self.o = B_, A, _track_options(track, "test")
        self.M = self.o["max_tracks"]
        self.nbytes = self.L.dagr_stream_track_bytes(B_, self.M)
        assert self.nbytes == 40 * B_ * self.M + 8 * B_
        self.state = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_track_reset(_lib.ptr(self.state), self.nbytes, B_, self.M, _lib.cur_stream(self.dev)),
                   "stream_track_reset")
        self.ids = torch.full((B_, A), -7, dtype=torch.int64, device=self.dev)
        self.hits = torch.full((B_, A), -7, dtype=torch.int32, device=self.dev)
        self.untracked = torch.zeros((B_,), dtype=torch.int64, device=self.dev)

    def call(self, s, **over):
        P = _lib.ptr
        det, n_keep, t_ref = _dev(s["det"]), _dev(s["n_keep"]), _dev(s["t_ref"])
        a = dict(tracks=P(self.state), bytes=self.nbytes, B=self.B, M=self.M, iou=self.o["iou"], age=self.o["max_age_us"],
                 min_score=self.o["min_score"], det=P(det), n_keep=P(n_keep), A=self.A, t_ref=P(t_ref), ids=P(self.ids),
                 hits=P(self.hits), untracked=P(self.untracked))
        a.update(over)
        rc = self.L.dagr_stream_track(a["tracks"], a["bytes"], a["B"], a["M"], a["iou"], a["age"], a["min_score"], a["det"],
                                      a["n_keep"], a["A"], a["t_ref"], a["ids"], a["hits"], a["untracked"],
                                      _lib.cur_stream(self.dev))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        return rc

    def slots(self):
        """The state through the layout include/dagr_hip.h documents."""
        n, raw, B_, M = self.B * self.M, self.state, self.B, self.M
        return (raw[:8 * n].view(torch.int64).view(B_, M).cpu().numpy(),
                raw[8 * n:16 * n].view(torch.int64).view(B_, M).cpu().numpy(),
                raw[16 * n:32 * n].view(torch.float32).view(B_, M, 4).cpu().numpy(),
                raw[32 * n:36 * n].view(torch.int32).view(B_, M).cpu().numpy(),
                raw[36 * n:40 * n].view(torch.int32).view(B_, M).cpu().numpy(),
                raw[40 * n:].view(torch.int64).cpu().numpy())


def _assert_same_slots(got, want, where):
    """Slot by slot: the ids (0: free) and next_id everywhere, the other fields where a track lives."""
    assert np.array_equal(got[0], want[0]), (where, "ids of the slots")
    assert np.array_equal(got[5], want[5]), (where, "next_id")
    live = want[0] != 0
    for k, name in ((1, "t_last"), (2, "box"), (3, "label"), (4, "hits")):
        assert np.array_equal(got[k][live], want[k][live]), (where, name)


def _run_case(case):
    tr = _Tracker(case["B"], case["A"], case["track"])
    fresh = tr.slots()
    assert not fresh[0].any() and fresh[5].tolist() == [1] * case["B"]
    steps, d = tc.run_definition(case)
    for k, (s, (ids, hits, untracked, slots)) in enumerate(zip(case["steps"], steps)):
        where = (case["name"], k)
        tr.ids.fill_(-7)
        tr.hits.fill_(-7)
        _lib.check(tr.call(s), "stream_track")
        got_ids, got_hits = tr.ids.cpu().numpy(), tr.hits.cpu().numpy()
        for b in range(case["B"]):
            n = min(max(int(s["n_keep"][b]), 0), case["A"])
            assert np.array_equal(got_ids[b, :n], ids[b, :n]), (where, b)
            assert np.array_equal(got_hits[b, :n], hits[b, :n]), (where, b)
            assert np.all(got_ids[b, n:] == -7) and np.all(got_hits[b, n:] == -7), (where, b)     # nothing behind n_keep
        assert np.array_equal(tr.untracked.cpu().numpy(), untracked), where
        _assert_same_slots(tr.slots(), slots, where)
        if case["expect"] is not None:
            tc.check_expectation(case, k, got_ids, got_hits, tr.untracked.cpu().numpy())
    return tr, d


@pytest.mark.parametrize("name", [c["name"] for c in tc.cases()])
def test_track_equals_the_definition_after_every_step(name):
    """Equal after every step: ids and hits of the rows, nothing written behind n_keep, `untracked`, and the tracks read
    back from the state slot by slot; and the case's written-out expectation."""
    _run_case(next(c for c in tc.cases() if c["name"] == name))


def test_argument_errors_launch_nothing_and_reset_empties():
    case = next(c for c in tc.cases() if c["name"] == "three-lanes-doing-different-things")
    tr, d = _run_case(case)
    assert tr.slots()[0].any()
    before, s = tr.state.clone(), case["steps"][-1]
    ids, untracked = tr.ids.clone(), tr.untracked.clone()
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    for over, text in ((dict(tracks=None), b"NULL"), (dict(n_keep=None), b"NULL"), (dict(t_ref=None), b"NULL"),
                       (dict(ids=None), b"NULL"), (dict(det=None), b"NULL"), (dict(bytes=tr.nbytes - 1), b"smaller"),
                       (dict(M=0), b"max_tracks"), (dict(M=257), b"max_tracks"), (dict(iou=0.0), b"iou"),
                       (dict(iou=1.5), b"iou"), (dict(iou=float("nan")), b"iou"), (dict(age=-1), b"max_age_us"),
                       (dict(B=0), b"out of range"), (dict(A=-1), b"A out of range"),
                       (dict(tracks=ctypes.c_void_p(tr.state.data_ptr() + 8)), b"aligned")):
        assert tr.call(s, **over) == bad, over
        assert text in tr.L.dagr_last_error(), (over, tr.L.dagr_last_error())
    assert torch.equal(tr.state, before) and torch.equal(tr.ids, ids) and torch.equal(tr.untracked, untracked)
    L, P = tr.L, _lib.ptr
    assert L.dagr_stream_track_bytes(0, 8) == 0 and L.dagr_stream_track_bytes(3, 0) == 0
    assert L.dagr_stream_track_bytes(3, 257) == 0 and L.dagr_stream_track_bytes(3, 256) == 40 * 3 * 256 + 24
    assert L.dagr_stream_track_reset(None, tr.nbytes, tr.B, tr.M, None) == bad
    assert L.dagr_stream_track_reset(P(tr.state), tr.nbytes - 1, tr.B, tr.M, _lib.cur_stream(tr.dev)) == bad
    assert L.dagr_stream_track_reset(P(tr.state), tr.nbytes, tr.B, 300, _lib.cur_stream(tr.dev)) == bad
    torch.cuda.synchronize()
    assert torch.equal(tr.state, before)
    _lib.check(L.dagr_stream_track_reset(P(tr.state), tr.nbytes, tr.B, tr.M, _lib.cur_stream(tr.dev)), "stream_track_reset")
    fresh = tr.slots()
    assert not fresh[0].any() and fresh[5].tolist() == [1] * tr.B
    # untracked may be NULL
    assert tr.call(case["steps"][0], untracked=None) == 0
    assert tr.slots()[0].any()


def test_t_ref_points_into_the_stream_state():
    """dagr_stream_t_ref is pointer arithmetic: the int64 [B] it names holds "never" after dagr_stream_reset."""
    L, dev = _lib.lib(), torch.device("cuda:0")
    cap = 1000
    nbytes = L.dagr_stream_state_bytes(B, cap)
    state = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=dev)
    _lib.check(L.dagr_stream_reset(_lib.ptr(state), B, cap, _lib.cur_stream(dev)), "stream_reset")
    where = L.dagr_stream_t_ref(_lib.ptr(state), B, cap)
    off = where - state.data_ptr()
    assert 0 < off and off + 8 * B <= nbytes and off % 8 == 0
    assert state[off:off + 8 * B].view(torch.int64).tolist() == [tc.NEVER] * B
    assert L.dagr_stream_t_ref(None, B, cap) is None and L.dagr_stream_t_ref(_lib.ptr(state), 0, cap) is None
    assert L.dagr_stream_t_ref(_lib.ptr(state), B, 0) is None


@pytest.mark.parametrize("max_tracks", [8, 64])
def test_random_walk_equals_the_definition_at_every_step(max_tracks):
    """B = 3, A = 64, 40 steps, up to 40 jittered boxes a lane that vanish and come back, two labels; 8 slots overflow.
    tests/test_stream_track_cpu.py holds the walk to matches, retirements, slots taken again and untracked rows."""
    _, d = _run_case(tc.random_walk(max_tracks))
    e = d.events
    assert e["matched"] > 0 and e["retired"] > 0 and e["reused"] > 0 and (max_tracks != 8 or e["untracked"] > 0), e


# ------------------------------------------------------------------------------------------------ the stream
_PUSHES = None


def _pushes():
    """12 steps of 1 ms on a 20 ms window: every lane keeps most of its window from step to step, so most detections
    continue; lane 1 pauses for two steps and lane 2 starts late."""
    global _PUSHES
    if _PUSHES is None:
        E = syn.edges_window
        _PUSHES = []
        for k in range(12):
            lo = 10000 + 1000 * (k - 1) if k else 0
            hi = 10000 + 1000 * k
            lanes = {0: (E, 2000 if k == 0 else 180), 1: (E, 1500 if k == 0 else 150), 2: (E, 0 if k < 2 else (1200 if k == 2 else 90))}
            parts = {b: _chunk(g, n, 300 + 3 * k + b, lo, hi) for b, (g, n) in lanes.items() if n and not (b == 1 and k in (5, 6))}
            _PUSHES.append(_push(parts, t_now=[hi] * 3))
    return _PUSHES


# the suite's model (random weights) keeps all of its 175 anchors at conf 0.001, with scores between 0.21 and 0.33; min_score
# cuts them to the tenth or so that stands out, which fits the slots
TRACK = dict(iou=0.3, max_age_us=2500, min_score=0.3, max_tracks=32)


def _step(stream, s):
    return stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], t_now=s["t_now"])


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_a_tracking_stream_changes_nothing_else_and_equals_the_definition(latency):
    """Boxes, scores and labels of a tracking stream are bit-equal to those of a stream without track= on the same pushes;
    track_ids / track_hits equal a TrackDefinition fed with every step's own detections and t_now; tracks() and untracked()
    equal the definition's; some id lives through several steps; after reset() the ids start at 1 again."""
    model = _model(B)                                   # (conf_threshold = 0.001: every step has detections)
    model.engine().set_low_latency(latency)
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK)
    assert stream.track_ids is None and stream.tracks()[0].dtype == np.dtype(TRACK_DTYPE) and not stream.untracked().any()
    d = TrackDefinition(B, TRACK)
    tracked, longest, rows = [], 0, 0
    with torch.no_grad():
        for rnd in range(2):
            for k, s in enumerate(_pushes()):
                det, nk = _step(stream, s)
                det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
                ids, hits = stream.track_ids.cpu().numpy(), stream.track_hits.cpu().numpy()
                assert stream.track_ids.dtype == torch.int64 and stream.track_hits.dtype == torch.int32
                assert ids.shape == det.shape[:2] == hits.shape
                want_ids, want_hits = d.step(det, nk, s["t_now"])
                for b in range(B):
                    n = int(nk[b])
                    assert np.array_equal(ids[b, :n], want_ids[b, :n]), (rnd, k, b)
                    assert np.array_equal(hits[b, :n], want_hits[b, :n]), (rnd, k, b)
                    longest, rows = max(longest, int(hits[b, :n].max(initial=0))), rows + n
                if rnd == 0:
                    tracked.append((det, nk))
            print("round", rnd, "rows", rows, "longest track", longest, d.events, "untracked", d.untracked.tolist())
            for got, want in zip(stream.tracks(), d.tracks()):
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), rnd
            assert np.array_equal(stream.untracked(), d.untracked), rnd
            stream.check_status()
            assert d.events["matched"] > 0 and d.events["spawned"] > 0 and longest >= 3, (d.events, longest)
            stream.reset()
            assert all(len(t) == 0 for t in stream.tracks()) and not stream.untracked().any()
            d.reset()                                   # the second round must give ids from 1 again
        # step(): the dicts carry the ids, cut by n_keep
        out = stream.step(*(np.stack([_pushes()[0]["x"], _pushes()[0]["y"]], -1), _pushes()[0]["t"], _pushes()[0]["p"]),
                          batch=_pushes()[0]["batch"], t_now=_pushes()[0]["t_now"])
        for b, lane in enumerate(out):
            n = len(lane["scores"])
            assert lane["track_ids"].dtype == torch.int64 and lane["track_hits"].dtype == torch.int32
            assert lane["track_ids"].shape == (n,) and lane["track_hits"].shape == (n,)
            ids = lane["track_ids"].tolist()            # a fresh stream: the eligible rows spawn 1, 2, ... in row order
            eligible = (lane["scores"] >= TRACK["min_score"]).tolist()
            assert [v for v in ids if v] == list(range(1, min(sum(eligible), TRACK["max_tracks"]) + 1)), b
            assert all(e or not v for e, v in zip(eligible, ids)) and lane["track_hits"].tolist() == [int(v > 0) for v in ids], b
        # the same pushes through a stream that does not track
        plain = EventStream(model, window_us=WINDOW_US)
        assert plain.track is None and plain.track_ids is None and plain.state.track_state is None
        for k, (s, (det_t, nk_t)) in enumerate(zip(_pushes(), tracked)):
            det, nk = _step(plain, s)
            nk = nk.cpu().numpy()
            assert np.array_equal(nk, nk_t), k
            for b in range(B):
                assert np.array_equal(det[b, :nk[b]].cpu().numpy(), det_t[b, :nk[b]]), (k, b)
        lane = plain.step(np.zeros((0, 2), np.int16), np.zeros(0, np.int64), np.zeros(0, np.int8),
                          t_now=_pushes()[-1]["t_now"])[0]
        assert sorted(lane) == ["boxes", "labels", "scores"]
        with pytest.raises(RuntimeError, match="does not track"):
            plain.tracks()
        with pytest.raises(RuntimeError, match="does not track"):
            plain.untracked()
    model.engine().set_low_latency(True)


TRACK_IMAGE = dict(iou=0.3, max_age_us=5000, min_score=0.0, max_tracks=64)


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_tracking_behind_frame_steps_and_held_steps(latency):
    """A --use_image model (resnet18, B = 2; tests/test_stream_hold_gpu.py's, warmed as that suite warms it, so that in
    latency mode both bodies are captured graphs before the tracking stream exists): frame step, two held steps, frame
    step, held step.  The image branch is not bit-reproducible, so nothing is compared with a second run: track_ids /
    track_hits equal a TrackDefinition fed with every step's own det / n_keep / t_now, the bodies are counted, an id lives
    from a frame step into the held step behind it, and the captured graphs are the objects they were -- no re-capture."""
    from tests import test_stream_hold_gpu as hold
    model = hold._image_model()
    eng = hold._warm(model, latency)
    graphs = (eng._wg, eng._hg)
    lanes = hold.B
    imgs = hold._images(7, 8)
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK_IMAGE)
    d = TrackDefinition(lanes, TRACK_IMAGE)
    previous, carried = None, []
    with torch.no_grad():
        for k, img in enumerate((imgs[0], None, None, imgs[1], None)):
            lo, hi = (0, 10000) if k == 0 else (10000 + 1000 * (k - 1), 10000 + 1000 * k)
            s = _push({b: _chunk(syn.edges_window, 1500 if k == 0 else 150, 500 + 2 * k + b, lo, hi) for b in range(lanes)},
                      t_now=[hi] * lanes)
            det, nk = stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], t_now=s["t_now"],
                                         image=img)
            det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
            ids, hits = stream.track_ids.cpu().numpy(), stream.track_hits.cpu().numpy()
            want_ids, want_hits = d.step(det, nk, s["t_now"])
            now = set()
            for b in range(lanes):
                n = int(nk[b])
                assert np.array_equal(ids[b, :n], want_ids[b, :n]), (k, b)
                assert np.array_equal(hits[b, :n], want_hits[b, :n]), (k, b)
                now |= {(b, int(v)) for v in ids[b, :n] if v}
            if img is None:                                      # a held step: ids that came over from the step before
                carried.append(len(now & previous))
            previous = now
            print("step", k, "frame" if img is not None else "held", "n_keep", nk.tolist(), "ids", len(now), d.events)
    assert (stream.frame_steps, stream.held_steps) == (2, 3)
    assert carried[0] > 0 and carried[2] > 0, carried            # ... from a frame step into the held step behind it
    for got, want in zip(stream.tracks(), d.tracks()):
        assert got.tobytes() == want.tobytes()
    assert np.array_equal(stream.untracked(), d.untracked)
    stream.check_status()
    if latency:
        assert graphs[0] is not None and graphs[1] is not None and eng._wg is graphs[0] and eng._hg is graphs[1]
    model.engine().set_low_latency(True)


def test_event_stream_refuses_bad_track_options_by_name():
    model = _model(B)
    for bad, name in ((dict(iou=0.0), "iou"), (dict(max_age_us=-5), "max_age_us"), (dict(max_tracks=1000), "max_tracks"),
                      (dict(min_score="high"), "min_score"), (dict(age=5), "age"), ("yes", "track")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, track=bad)
    stream = EventStream(model, window_us=WINDOW_US, track=True)
    assert stream.track == _track_options(True, "t") and stream.state.track_state.numel() == 40 * B * 64 + 8 * B


# ------------------------------------------------------------------------------------------------ waits and calls
def test_a_tracking_step_on_device_inputs_waits_for_nothing():
    """torch's sync debug mode turns every host synchronisation torch makes into an error: first a probe that it does so
    on this build (an .item()), then step_device of a tracking stream on device-resident events under it."""
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
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK)
    pushes = [(_dev(np.stack([s["x"], s["y"]], -1)), _dev(s["t"]), _dev(s["p"]), _dev(s["batch"].astype(np.int32)),
               _dev(s["t_now"])) for s in _pushes()[:6]]
    seen = []

    def step(xy, t, p, batch, t_now):
        det, nk = stream.step_device(xy, t, p, batch=batch, t_now=t_now)
        seen.append((det.clone(), nk.clone(), stream.track_ids.clone(), stream.track_hits.clone()))       # (no wait either)
    with torch.no_grad():
        for push in pushes[:4]:                                # two eager steps, the capture, one replay
            step(*push)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for push in pushes[4:]:
                step(*push)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    d = TrackDefinition(B, TRACK)
    for k, ((det, nk, ids, hits), s) in enumerate(zip(seen, _pushes())):
        want_ids, want_hits = d.step(det.cpu().numpy(), nk.cpu().numpy(), s["t_now"])
        for b in range(B):
            n = int(nk[b])
            assert np.array_equal(ids[b, :n].cpu().numpy(), want_ids[b, :n]), (k, b)
            assert np.array_equal(hits[b, :n].cpu().numpy(), want_hits[b, :n]), (k, b)
    assert d.events["spawned"] > 0 and d.events["matched"] > 0, d.events
    stream.check_status()


STEP_ENTRIES = ("dagr_stream_denoise", "dagr_stream_downsample", "dagr_stream_frame", "dagr_stream_stage",
                "dagr_stream_stage_capped", "dagr_stream_stage_dev", "dagr_stream_stage_dev_capped", "dagr_stream_track")


def _record_calls(monkeypatch):
    """Every entry of the library, wrapped to note its name."""
    L, calls = _lib.lib(), []
    for name in _lib.SIGNATURES:
        def wrapper(*a, _f=getattr(L, name), _n=name):
            calls.append(_n)
            return _f(*a)
        monkeypatch.setattr(L, name, wrapper)
    return calls


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_tracking_adds_one_library_call_a_step_and_nothing_when_off(latency, monkeypatch):
    """Step for step a tracking stream issues the library calls of a stream without track= plus ONE dagr_stream_track, the
    step's last call (and asks once, when its state is allocated, where the state keeps t_ref); a stream without track=
    -- None or left out -- issues neither and owns no track state."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    calls = _record_calls(monkeypatch)
    per_stream = {}
    # (the first stream warms the engine up -- eager steps, the capture -- so that the three after it meet the same engine)
    for name, kw in (("warm-up", dict()), ("left out", dict()), ("none", dict(track=None)), ("tracking", dict(track=TRACK))):
        stream = EventStream(model, window_us=WINDOW_US, **kw)
        steps = []
        with torch.no_grad():
            for s in _pushes()[:6]:
                del calls[:]
                _step(stream, s)
                steps.append(list(calls))
        torch.cuda.synchronize()
        per_stream[name] = steps
        if name != "tracking":
            st = stream.state
            assert st.track is None and st.track_state is None and st.lane_untracked is None and st.track_ids is None
    off = per_stream["left out"]
    assert per_stream["none"] == off
    assert not any("track" in c or c == "dagr_stream_t_ref" for step in off for c in step)
    assert all([c for c in step if c in STEP_ENTRIES] == ["dagr_stream_stage"] for step in off), off
    for k, (with_, without) in enumerate(zip(per_stream["tracking"], off)):
        assert with_[-1] == "dagr_stream_track", (k, with_)
        extra = ["dagr_stream_t_ref"] if k == 0 else []
        assert with_[:-1] == without + extra, (k, with_, without)
    model.engine().set_low_latency(True)


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_writes_the_tracks_next_to_unchanged_detections(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    import re
    model = _model(1)
    base = ["--step_us", "1000", "--window_us", "20000", "--steps", "10", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "200000", "--sequence", "trk"]
    paths = {}
    for name, extra in (("plain", []), ("track", ["--track", "--track_max_age_us", "2500", "--max_tracks", "32", "--track_min_score", "0.3"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        source = R.SyntheticStream(C.flags("", argv, extra=R.stream_options))
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    printed = capsys.readouterr().out
    with open(paths["plain"], "rb") as f, open(paths["track"], "rb") as g:
        assert f.read() == g.read()                      # detections_<sequence>.npy is byte for byte what it was
    assert not os.path.exists(os.path.join(os.path.dirname(str(paths["plain"])), "tracks_trk.npy"))
    rec = np.load(paths["track"])
    trk = np.load(os.path.join(os.path.dirname(str(paths["track"])), "tracks_trk.npy"))
    assert trk.dtype == np.dtype(R.TRACK_RECORD_DTYPE) and len(trk) == len(rec) > 0
    for name in rec.dtype.names:
        assert trk[name].tobytes() == rec[name].tobytes(), name
    ids = np.unique(trk["track_id"])
    n_ids = len(ids[ids != 0])
    assert n_ids > 0 and int(trk["hits"].max()) >= 3               # a track lives through several steps
    assert np.all((trk["track_id"] == 0) == (trk["hits"] == 0))
    for t in np.unique(trk["t"]):                                   # inside a step an id is given once
        step_ids = trk["track_id"][(trk["t"] == t) & (trk["track_id"] != 0)]
        assert len(step_ids) == len(set(step_ids.tolist())), t
    said = re.search(rf"; {n_ids} distinct track ids, (\d+) detections untracked -> \S*tracks_trk\.npy", printed)
    assert said, printed
    eligible = trk["class_confidence"] >= np.float32(0.3)
    assert np.all(trk["track_id"][~eligible] == 0)
    assert int(said.group(1)) == int((trk["track_id"][eligible] == 0).sum())
