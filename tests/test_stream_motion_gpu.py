"""The event stream's motion model on the GPU: dagr_stream_track_cv through the binding against the numpy definition
(dagr_amd/streaming.py: TrackDefinition(motion=)) bit for bit after every step of every case of
tests/stream_motion_cases.py and of its seeded walks; against dagr_stream_track itself where the two must agree;
EventStream(track=, motion=) against an untracked stream on the same pushes and against a definition fed with every step's
own detections, in latency and in throughput mode and behind the frame and held steps of a --use_image model; the absence
of host waits; the library calls of streams with and without the motion model; and scripts/run_stream.py --track_motion."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from dagr_amd import _lib
from dagr_amd.streaming import (COAST_DTYPE, TRACK_DTYPE, TRACK_MOTION_DTYPE, EventStream, TrackDefinition,
                                _motion_options, _track_options)
from dagr_amd.utils import synthetic as syn
from tests import stream_motion_cases as mc
from tests.test_stream_track_gpu import STEP_ENTRIES, TRACK, _pushes, _record_calls, _step
from tests.test_stream_track_gpu import _Tracker as _PlainTracker
from tests.test_streaming_gpu import _chunk, _dev, _model, _push

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 320, 215, 3
WINDOW_US = 20000
SENTINEL = -7


# ------------------------------------------------------------------------------------------------ the kernel, case by case
class _Tracker:
    """dagr_stream_track_cv on a state of its own; the state starts out as garbage in front of its reset, every output as
    the sentinel -7."""

    def __init__(self, B_, A, track, motion):
        self.L, self.dev = _lib.lib(), torch.device("cuda:0")
        self.B, self.A, self.o = B_, A, _track_options(track, "test")
        self.m = _motion_options(motion, self.o, "test")
        self.M = M = self.o["max_tracks"]
        self.nbytes = self.L.dagr_stream_track_cv_bytes(B_, M)
        assert self.nbytes == 56 * B_ * M + 8 * B_
        self.state = torch.full((self.nbytes,), 0x5a, dtype=torch.uint8, device=self.dev)
        _lib.check(self.L.dagr_stream_track_cv_reset(_lib.ptr(self.state), self.nbytes, B_, M, _lib.cur_stream(self.dev)),
                   "stream_track_cv_reset")
        full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device=self.dev)           # noqa: E731
        self.out = dict(ids=full((B_, A), torch.int64), hits=full((B_, A), torch.int32), box=full((B_, A, 4), torch.float32),
                        vel=full((B_, A, 4), torch.float32), coast_id=full((B_, M), torch.int64),
                        coast_box=full((B_, M, 4), torch.float32), coast_label=full((B_, M), torch.int32),
                        coast_age=full((B_, M), torch.int64), n_coast=full((B_,), torch.int32))
        self.untracked = torch.zeros((B_,), dtype=torch.int64, device=self.dev)

    def refill(self):
        for t in self.out.values():
            t.fill_(SENTINEL)

    def call(self, s, **over):
        P = _lib.ptr
        det, n_keep, t_ref = _dev(s["det"]), _dev(s["n_keep"]), _dev(s["t_ref"])
        a = dict(tracks=P(self.state), bytes=self.nbytes, B=self.B, M=self.M, iou=self.o["iou"], age=self.o["max_age_us"],
                 min_score=self.o["min_score"], alpha=self.m["alpha"], beta=self.m["beta"], det=P(det), n_keep=P(n_keep),
                 A=self.A, t_ref=P(t_ref), untracked=P(self.untracked), **{k: P(v) for k, v in self.out.items()})
        a.update(over)
        rc = self.L.dagr_stream_track_cv(a["tracks"], a["bytes"], a["B"], a["M"], a["iou"], a["age"], a["min_score"],
                                         a["alpha"], a["beta"], a["det"], a["n_keep"], a["A"], a["t_ref"], a["ids"], a["hits"],
                                         a["box"], a["vel"], a["coast_id"], a["coast_box"], a["coast_label"], a["coast_age"],
                                         a["n_coast"], a["untracked"], _lib.cur_stream(self.dev))
        torch.cuda.synchronize()                    # (the inputs above live until here)
        return rc

    def slots(self):
        """The state through the layout include/dagr_hip.h documents."""
        n, raw, B_, M = self.B * self.M, self.state, self.B, self.M
        return (raw[:8 * n].view(torch.int64).view(B_, M).cpu().numpy(),
                raw[8 * n:16 * n].view(torch.int64).view(B_, M).cpu().numpy(),
                raw[16 * n:32 * n].view(torch.float32).view(B_, M, 4).cpu().numpy(),
                raw[32 * n:48 * n].view(torch.float32).view(B_, M, 4).cpu().numpy(),
                raw[48 * n:52 * n].view(torch.int32).view(B_, M).cpu().numpy(),
                raw[52 * n:56 * n].view(torch.int32).view(B_, M).cpu().numpy(),
                raw[56 * n:].view(torch.int64).cpu().numpy())


def _same(a, b):
    """Equal arrays; floats as bits, so a NaN equals itself and -0.0 is not 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        a, b = mc.bits(a), mc.bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _assert_same_slots(got, want, where):
    """Slot by slot: the ids (0: free) and next_id everywhere, the other fields -- vel among them -- where a track lives."""
    assert _same(got[0], want[0]), (where, "ids of the slots")
    assert _same(got[6], want[6]), (where, "next_id")
    live = want[0] != 0
    for k, name in ((1, "t_last"), (2, "box"), (3, "vel"), (4, "label"), (5, "hits")):
        assert _same(got[k][live], want[k][live]), (where, name)


def _assert_step(out, untracked, want, s, A, where):
    """One step's outputs (numpy, by name) against the definition's: the rows below n_keep and the first n_coast coast
    entries are the definition's, everything behind them is still the sentinel."""
    for b in range(len(s["n_keep"])):
        n = min(max(int(s["n_keep"][b]), 0), A)
        for name in ("ids", "hits", "box", "vel"):
            assert _same(out[name][b, :n], want[name][b, :n]), (where, b, name)
            assert np.all(out[name][b, n:] == SENTINEL), (where, b, name, "behind n_keep")
        c = int(want["n_coast"][b])
        assert int(out["n_coast"][b]) == c, (where, b, "n_coast")
        for name, ref in zip(("coast_id", "coast_box", "coast_label", "coast_age"), want["coast"]):
            assert _same(out[name][b, :c], ref[b, :c]), (where, b, name)
            assert np.all(out[name][b, c:] == SENTINEL), (where, b, name, "behind n_coast")
    assert _same(untracked, want["untracked"]), (where, "untracked")


def _run_case(case):
    tr = _Tracker(case["B"], case["A"], case["track"], case["motion"])
    fresh = tr.slots()
    assert not fresh[0].any() and not fresh[3].any() and fresh[6].tolist() == [1] * case["B"]
    steps, d = mc.run_definition(case)
    for k, (s, want) in enumerate(zip(case["steps"], steps)):
        where = (case["name"], k)
        tr.refill()
        _lib.check(tr.call(s), "stream_track_cv")
        out = {name: t.cpu().numpy() for name, t in tr.out.items()}
        _assert_step(out, tr.untracked.cpu().numpy(), want, s, case["A"], where)
        _assert_same_slots(tr.slots(), want["slots"], where)
        if case["expect"] is not None:
            mc.tc.check_expectation(case, k, out["ids"], out["hits"], tr.untracked.cpu().numpy())
    return tr, d


@pytest.mark.parametrize("name", [c["name"] for c in mc.cases()])
def test_track_cv_equals_the_definition_after_every_step(name):
    """Bit for bit after every step: ids, hits, filtered boxes and velocities of the rows, the coast list, `untracked`,
    the slots with their velocities; the sentinel behind n_keep and behind n_coast.  Among the cases: A = 300 rows against
    256 slots, 130 slots (three slot registers, the last with a tail of two), a NaN box, and a clock that goes back by
    more than 2**24 us, which shows the int64 -> fp32 conversion of the age."""
    _run_case(next(c for c in mc.cases() if c["name"] == name))


@pytest.mark.parametrize("max_tracks", [8, 64, 130])
def test_the_walk_equals_the_definition_at_every_step(max_tracks):
    """B = 3, A = 64: boxes on constant-velocity paths with jitter that vanish for some steps and come back; 8 slots
    overflow, 130 slots fill a thread's second register.  tests/test_stream_motion_cpu.py holds the walk to matches,
    spawns, retirements, slots taken again, coasts and matches only the prediction gives."""
    _, d = _run_case(mc.random_walk(max_tracks))
    e = d.events
    assert e["matched"] > 0 and e["retired"] > 0 and e["reused"] > 0 and e["coasted"] > 0 and e["motion_only"] > 0, e


@pytest.mark.parametrize("max_tracks", [8, 64])
def test_at_one_shared_instant_track_cv_gives_what_dagr_stream_track_gives(max_tracks):
    """Every step at one t_ref, alpha = 1: dt is 0, the prediction is the box, no velocity changes.  Both launches on the
    same steps: ids, hits and `untracked` are equal (and so are the slots' common fields)."""
    case = mc.shared_instant(max_tracks)
    cv = _Tracker(case["B"], case["A"], case["track"], case["motion"])
    plain = _PlainTracker(case["B"], case["A"], case["track"])
    matched = 0
    for k, s in enumerate(case["steps"]):
        cv.refill()
        plain.ids.fill_(SENTINEL)
        plain.hits.fill_(SENTINEL)
        _lib.check(cv.call(s), "stream_track_cv")
        _lib.check(plain.call(s), "stream_track")
        assert torch.equal(cv.out["ids"], plain.ids) and torch.equal(cv.out["hits"], plain.hits), k
        assert torch.equal(cv.untracked, plain.untracked), k
        a, p = cv.slots(), plain.slots()
        live = p[0] != 0
        assert _same(a[0], p[0]) and _same(a[6], p[5]) and not a[3].any(), k
        for x, y in ((a[1], p[1]), (a[2], p[2]), (a[4], p[3]), (a[5], p[4])):
            assert _same(x[live], y[live]), k
        matched += int((plain.hits > 1).sum())
    assert matched > 50 and (int(plain.untracked.sum()) > 0) == (max_tracks == 8)


def test_argument_errors_launch_nothing_and_reset_empties():
    case = next(c for c in mc.cases() if c["name"] == "lanes-are-independent")
    tr, d = _run_case(case)
    assert tr.slots()[0].any()
    before, s = tr.state.clone(), case["steps"][-1]
    outs, untracked = {k: v.clone() for k, v in tr.out.items()}, tr.untracked.clone()
    bad = _lib.ENUMS["DAGR_ERR_INVALID_ARG"]
    off = lambda name, by: ctypes.c_void_p(tr.out[name].data_ptr() + by)          # noqa: E731
    nan = float("nan")
    for over, text in ((dict(tracks=None), b"NULL"), (dict(n_keep=None), b"NULL"), (dict(t_ref=None), b"NULL"),
                       (dict(ids=None), b"NULL"), (dict(det=None), b"NULL"), (dict(bytes=tr.nbytes - 1), b"smaller"),
                       (dict(M=0), b"max_tracks"), (dict(M=257), b"max_tracks"), (dict(iou=0.0), b"iou"),
                       (dict(iou=1.5), b"iou"), (dict(iou=nan), b"iou"), (dict(age=-1), b"max_age_us"),
                       (dict(B=0), b"out of range"), (dict(A=-1), b"A out of range"),
                       (dict(tracks=ctypes.c_void_p(tr.state.data_ptr() + 8)), b"aligned"),
                       # what the motion model adds
                       (dict(alpha=0.0), b"alpha"), (dict(alpha=1.0001), b"alpha"), (dict(alpha=nan), b"alpha"),
                       (dict(alpha=-0.5), b"alpha"), (dict(beta=-0.001), b"beta"), (dict(beta=1.5), b"beta"),
                       (dict(beta=nan), b"beta"), (dict(age=1 << 24), b"max_age_us"), (dict(box=None), b"track_box"),
                       (dict(vel=None), b"track_vel"), (dict(box=off("box", 4)), b"track_box"),
                       (dict(vel=off("vel", 8)), b"track_vel"), (dict(coast_box=off("coast_box", 4)), b"coast_box"),
                       (dict(coast_id=off("coast_id", 4)), b"coast_id"), (dict(coast_age=off("coast_age", 4)), b"coast_age_us"),
                       (dict(coast_label=off("coast_label", 2)), b"coast_label"), (dict(n_coast=off("n_coast", 2)), b"n_coast"),
                       (dict(coast_id=None), b"coast_id"), (dict(coast_box=None), b"coast_box"),
                       (dict(coast_label=None), b"coast_label"), (dict(coast_age=None), b"coast_age_us"),
                       (dict(n_coast=None), b"n_coast"),
                       (dict(coast_id=None, coast_box=None, coast_label=None, coast_age=None), b"n_coast")):
        assert tr.call(s, **over) == bad, over
        assert text in tr.L.dagr_last_error(), (over, tr.L.dagr_last_error())
    assert torch.equal(tr.state, before) and torch.equal(tr.untracked, untracked)
    assert all(torch.equal(tr.out[k].view(torch.uint8), outs[k].view(torch.uint8)) for k in outs)
    L, P = tr.L, _lib.ptr
    assert L.dagr_stream_track_cv_bytes(0, 8) == 0 and L.dagr_stream_track_cv_bytes(3, 0) == 0
    assert L.dagr_stream_track_cv_bytes(3, 257) == 0 and L.dagr_stream_track_cv_bytes(3, 256) == 56 * 3 * 256 + 24
    assert L.dagr_stream_track_cv_bytes(65536, 8) == 0 and L.dagr_stream_track_cv_bytes(1, 1) == 64
    assert L.dagr_stream_track_cv_reset(None, tr.nbytes, tr.B, tr.M, None) == bad
    assert L.dagr_stream_track_cv_reset(P(tr.state), tr.nbytes - 1, tr.B, tr.M, _lib.cur_stream(tr.dev)) == bad
    assert L.dagr_stream_track_cv_reset(P(tr.state), tr.nbytes, tr.B, 300, _lib.cur_stream(tr.dev)) == bad
    assert L.dagr_stream_track_cv_reset(ctypes.c_void_p(tr.state.data_ptr() + 8), tr.nbytes, tr.B, tr.M, None) == bad
    torch.cuda.synchronize()
    assert torch.equal(tr.state, before)
    # the age bound itself is accepted
    assert tr.call(s, age=(1 << 24) - 1) == 0
    _lib.check(L.dagr_stream_track_cv_reset(P(tr.state), tr.nbytes, tr.B, tr.M, _lib.cur_stream(tr.dev)), "stream_track_cv_reset")
    fresh = tr.slots()
    assert not fresh[0].any() and not fresh[3].any() and fresh[6].tolist() == [1] * tr.B
    # the coast arrays may be NULL together, and so may untracked: the step is the same, no coast list is written
    tr.refill()
    none = dict(coast_id=None, coast_box=None, coast_label=None, coast_age=None, n_coast=None, untracked=None)
    for k in (0, 1, 2):
        assert tr.call(case["steps"][k], **none) == 0
    want = mc.run_definition(case)[0][2]
    assert _same(tr.out["ids"].cpu().numpy()[2, :2], want["ids"][2, :2]) and tr.slots()[0].any()
    _assert_same_slots(tr.slots(), want["slots"], "NULL coast arrays")
    assert all(bool((tr.out[k] == SENTINEL).all()) for k in ("coast_id", "coast_box", "coast_label", "coast_age", "n_coast"))


# ------------------------------------------------------------------------------------------------ the stream
MOTION = dict(alpha=1.0, beta=0.25)


def _compare_stream_step(stream, d, det, nk, t_now, where):
    """The stream's last step against the definition fed the step's own detections: rows, coast lists."""
    ids, hits = stream.track_ids.cpu().numpy(), stream.track_hits.cpu().numpy()
    boxes, vel = stream.track_boxes.cpu().numpy(), stream.track_vel.cpu().numpy()
    assert stream.track_boxes.dtype == torch.float32 and boxes.shape == det.shape[:2] + (4,) == vel.shape
    want_ids, want_hits = d.step(det, nk, t_now)
    for b in range(d.B):
        n = int(nk[b])
        assert _same(ids[b, :n], want_ids[b, :n]) and _same(hits[b, :n], want_hits[b, :n]), (where, b)
        assert _same(boxes[b, :n], d.track_box[b, :n]) and _same(vel[b, :n], d.track_vel[b, :n]), (where, b)
    n_coast, c_id, c_box, c_label, c_age = (t.cpu().numpy() for t in stream.coast_device())
    assert _same(n_coast, d.n_coast), where
    for b in range(d.B):
        c = int(n_coast[b])
        assert _same(c_id[b, :c], d.coast_id[b, :c]) and _same(c_box[b, :c], d.coast_box[b, :c]), (where, b)
        assert _same(c_label[b, :c], d.coast_label[b, :c]) and _same(c_age[b, :c], d.coast_age_us[b, :c]), (where, b)
    for got, want in zip(stream.coasting(), d.coasting()):
        assert got.dtype == np.dtype(COAST_DTYPE) == want.dtype and got.tobytes() == want.tobytes(), where
    return ids, hits


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_a_motion_stream_changes_nothing_else_and_equals_the_definition(latency):
    """Boxes, scores and labels of a motion stream are bit-equal to those of a stream without track= on the same pushes;
    ids, hits, filtered boxes, velocities and coast lists equal a TrackDefinition(motion=) fed with every step's own
    detections and t_now; tracks() (with velocities) and untracked() equal the definition's; nothing is captured again;
    after reset() the ids start at 1 again."""
    model = _model(B)                                   # (conf_threshold = 0.001: every step has detections)
    eng = model.engine()
    eng.set_low_latency(latency)
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK, motion=True)
    assert stream.motion == MOTION and stream.track == _track_options(TRACK, "t")
    assert stream.track_boxes is None and stream.track_vel is None and all(len(c) == 0 for c in stream.coasting())
    assert stream.tracks()[0].dtype == np.dtype(TRACK_MOTION_DTYPE) and not stream.untracked().any()
    assert stream.state.track_state.numel() == 56 * B * TRACK["max_tracks"] + 8 * B
    d = TrackDefinition(B, TRACK, motion=True)
    tracked, longest, graph = [], 0, None
    with torch.no_grad():
        for rnd in range(2):
            for k, s in enumerate(_pushes()):
                det, nk = _step(stream, s)
                det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
                ids, hits = _compare_stream_step(stream, d, det, nk, s["t_now"], (rnd, k))
                longest = max(longest, int(hits.max(initial=0)))
                if rnd == 0:
                    tracked.append((det, nk))
            print("round", rnd, "longest track", longest, d.events, "untracked", d.untracked.tolist())
            for got, want in zip(stream.tracks(), d.tracks()):
                assert got.dtype == want.dtype == np.dtype(TRACK_MOTION_DTYPE) and got.tobytes() == want.tobytes(), rnd
            assert np.array_equal(stream.untracked(), d.untracked), rnd
            stream.check_status()
            assert d.events["matched"] > 0 and d.events["spawned"] > 0 and d.events["coasted"] > 0 and longest >= 3, d.events
            if rnd == 0:
                graph = eng._wg
            elif latency:
                assert graph is not None and eng._wg is graph          # no re-capture
            stream.reset()
            assert all(len(t) == 0 for t in stream.tracks()) and not stream.untracked().any()
            assert all(len(c) == 0 for c in stream.coasting())
            d.reset()                                   # the second round must give ids from 1 again
        # step(): the dicts carry the filtered boxes and the velocities, cut by n_keep
        p0 = _pushes()[0]
        out = stream.step(np.stack([p0["x"], p0["y"]], -1), p0["t"], p0["p"], batch=p0["batch"], t_now=p0["t_now"])
        for b, lane in enumerate(out):
            n = len(lane["scores"])
            assert sorted(lane) == ["boxes", "labels", "scores", "track_boxes", "track_hits", "track_ids", "track_vel"]
            assert lane["track_boxes"].shape == (n, 4) == lane["track_vel"].shape and lane["track_boxes"].dtype == torch.float32
            assert torch.equal(lane["track_boxes"], lane["boxes"]) and not lane["track_vel"].any(), b       # a fresh stream
        # the same pushes through a stream that does not track, and through one that tracks without the motion model
        plain = EventStream(model, window_us=WINDOW_US)
        assert plain.motion is None and plain.track_boxes is None and plain.state.coast is None
        for k, (s, (det_t, nk_t)) in enumerate(zip(_pushes(), tracked)):
            det, nk = _step(plain, s)
            nk = nk.cpu().numpy()
            assert np.array_equal(nk, nk_t), k
            for b in range(B):
                assert np.array_equal(det[b, :nk[b]].cpu().numpy(), det_t[b, :nk[b]]), (k, b)
        with pytest.raises(RuntimeError, match="no motion model"):
            plain.coasting()
        only = EventStream(model, window_us=WINDOW_US, track=TRACK)
        assert only.motion is None and only.state.track_state.numel() == 40 * B * TRACK["max_tracks"] + 8 * B
        _step(only, _pushes()[0])
        assert only.track_boxes is None and only.tracks()[0].dtype == np.dtype(TRACK_DTYPE)
        with pytest.raises(RuntimeError, match="no motion model"):
            only.coast_device()
    eng.set_low_latency(True)


def test_motion_behind_frame_steps_and_held_steps():
    """A --use_image model (resnet18, B = 2; tests/test_stream_hold_gpu.py's, warmed as that suite warms it, so that both
    bodies are captured graphs before the motion stream exists): frame step, two held steps, frame step, held step.  The
    image branch is not bit-reproducible, so nothing is compared with a second run: the tracker's outputs equal a
    TrackDefinition(motion=) fed with every step's own det / n_keep / t_now, the bodies are counted, and the captured graphs
    are the objects they were -- no re-capture."""
    from tests import test_stream_hold_gpu as hold
    from tests.test_stream_track_gpu import TRACK_IMAGE
    model = hold._image_model()
    eng = hold._warm(model, True)
    graphs = (eng._wg, eng._hg)
    lanes = hold.B
    imgs = hold._images(7, 8)
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK_IMAGE, motion=dict(alpha=0.75, beta=0.5))
    d = TrackDefinition(lanes, TRACK_IMAGE, motion=dict(alpha=0.75, beta=0.5))
    with torch.no_grad():
        for k, img in enumerate((imgs[0], None, None, imgs[1], None)):
            lo, hi = (0, 10000) if k == 0 else (10000 + 1000 * (k - 1), 10000 + 1000 * k)
            s = _push({b: _chunk(syn.edges_window, 1500 if k == 0 else 150, 500 + 2 * k + b, lo, hi) for b in range(lanes)},
                      t_now=[hi] * lanes)
            det, nk = stream.step_device(np.stack([s["x"], s["y"]], -1), s["t"], s["p"], batch=s["batch"], t_now=s["t_now"],
                                         image=img)
            det, nk = det.clone().cpu().numpy(), nk.clone().cpu().numpy()
            _compare_stream_step(stream, d, det, nk, s["t_now"], k)
            print("step", k, "frame" if img is not None else "held", "n_keep", nk.tolist(), d.events)
    assert (stream.frame_steps, stream.held_steps) == (2, 3)
    assert d.events["matched"] > 0 and d.events["spawned"] > 0, d.events
    for got, want in zip(stream.tracks(), d.tracks()):
        assert got.tobytes() == want.tobytes()
    assert np.array_equal(stream.untracked(), d.untracked)
    stream.check_status()
    assert graphs[0] is not None and graphs[1] is not None and eng._wg is graphs[0] and eng._hg is graphs[1]
    model.engine().set_low_latency(True)


def test_event_stream_refuses_bad_motion_options_by_name():
    model = _model(B)
    for kw, name in ((dict(motion=True), "motion= needs track="), (dict(track=True, motion=dict(alpha=0.0)), "alpha"),
                     (dict(track=True, motion=dict(alpha=1.5)), "alpha"), (dict(track=True, motion=dict(beta=-1.0)), "beta"),
                     (dict(track=True, motion=dict(beta=float("nan"))), "beta"), (dict(track=True, motion=dict(gain=1)), "gain"),
                     (dict(track=True, motion="yes"), "motion"),
                     (dict(track=dict(max_age_us=1 << 24), motion=True), "max_age_us")):
        with pytest.raises(ValueError, match=name):
            EventStream(model, window_us=WINDOW_US, **kw)
    stream = EventStream(model, window_us=WINDOW_US, track=dict(max_age_us=(1 << 24) - 1), motion=dict(beta=0))
    assert stream.motion == dict(alpha=1.0, beta=0.0) and stream.state.track_state.numel() == 56 * B * 64 + 8 * B


# ------------------------------------------------------------------------------------------------ waits and calls
def test_a_motion_step_on_device_inputs_waits_for_nothing():
    """torch's sync debug mode turns every host synchronisation torch makes into an error: first a probe that it does so
    on this build (an .item()), then step_device of a motion stream on device-resident events under it."""
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
    stream = EventStream(model, window_us=WINDOW_US, track=TRACK, motion=True)
    pushes = [(_dev(np.stack([s["x"], s["y"]], -1)), _dev(s["t"]), _dev(s["p"]), _dev(s["batch"].astype(np.int32)),
               _dev(s["t_now"])) for s in _pushes()[:6]]
    seen = []

    def step(xy, t, p, batch, t_now):
        det, nk = stream.step_device(xy, t, p, batch=batch, t_now=t_now)
        seen.append((det.clone(), nk.clone(), stream.track_ids.clone(), stream.track_hits.clone(), stream.track_boxes.clone(),
                     stream.track_vel.clone(), [t.clone() for t in stream.coast_device()]))          # (no wait either)
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
    d = TrackDefinition(B, TRACK, motion=True)
    for k, ((det, nk, ids, hits, boxes, vel, coast), s) in enumerate(zip(seen, _pushes())):
        want_ids, want_hits = d.step(det.cpu().numpy(), nk.cpu().numpy(), s["t_now"])
        for b in range(B):
            n = int(nk[b])
            assert _same(ids[b, :n].cpu().numpy(), want_ids[b, :n]) and _same(hits[b, :n].cpu().numpy(), want_hits[b, :n]), (k, b)
            assert _same(boxes[b, :n].cpu().numpy(), d.track_box[b, :n]) and _same(vel[b, :n].cpu().numpy(), d.track_vel[b, :n]), (k, b)
        assert _same(coast[0].cpu().numpy(), d.n_coast), k
    assert d.events["spawned"] > 0 and d.events["matched"] > 0, d.events
    stream.check_status()


@pytest.mark.parametrize("latency", [True, False], ids=["latency", "throughput"])
def test_motion_swaps_the_tracker_call_and_changes_no_other_stream(latency, monkeypatch):
    """Step for step a motion stream issues the library calls of a stream without track= plus ONE dagr_stream_track_cv,
    the step's last call, and no dagr_stream_track (it asks once where the state keeps t_ref, as a tracking stream does).
    A tracking stream without motion= still ends every step with its one dagr_stream_track and never calls the new entry;
    a stream without track= issues neither."""
    model = _model(B)
    model.engine().set_low_latency(latency)
    calls = _record_calls(monkeypatch)
    per_stream = {}
    # (the first stream warms the engine up -- eager steps, the capture -- so that the ones after it meet the same engine)
    for name, kw in (("warm-up", dict()), ("left out", dict()), ("none", dict(track=None, motion=None)),
                     ("tracking", dict(track=TRACK)), ("tracking, motion none", dict(track=TRACK, motion=None)),
                     ("motion", dict(track=TRACK, motion=True))):
        stream = EventStream(model, window_us=WINDOW_US, **kw)
        steps = []
        with torch.no_grad():
            for s in _pushes()[:6]:
                del calls[:]
                _step(stream, s)
                steps.append(list(calls))
        torch.cuda.synchronize()
        per_stream[name] = steps
        st = stream.state
        if name != "motion":
            assert st.motion is None and st.coast is None and st.track_boxes is None and st.track_vel is None
        if "tracking" not in name and name != "motion":
            assert st.track is None and st.track_state is None and st.lane_untracked is None and st.track_ids is None
    off = per_stream["left out"]
    entries = STEP_ENTRIES + ("dagr_stream_track_cv",)
    assert per_stream["none"] == off
    assert not any("track" in c or c == "dagr_stream_t_ref" for step in off for c in step)
    assert all([c for c in step if c in entries] == ["dagr_stream_stage"] for step in off), off
    assert per_stream["tracking, motion none"] == per_stream["tracking"]
    for k, (with_, without) in enumerate(zip(per_stream["tracking"], off)):
        assert with_[-1] == "dagr_stream_track" and "dagr_stream_track_cv" not in with_, (k, with_)
        assert with_[:-1] == without + (["dagr_stream_t_ref"] if k == 0 else []), (k, with_, without)
    for k, (with_, without) in enumerate(zip(per_stream["motion"], off)):
        assert with_[-1] == "dagr_stream_track_cv" and "dagr_stream_track" not in with_, (k, with_)
        assert with_[:-1] == without + (["dagr_stream_t_ref"] if k == 0 else []), (k, with_, without)
    model.engine().set_low_latency(True)


# ------------------------------------------------------------------------------------------------ the script
def test_run_stream_script_writes_tracks_with_motion_and_the_coast_lists(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import run_stream as R
    model = _model(1)
    base = ["--step_us", "1000", "--window_us", "20000", "--steps", "10", "--stream", "edges", "--width", str(W), "--height",
            str(H), "--events_per_window", "200000", "--sequence", "mot"]
    track = ["--track", "--track_max_age_us", "2500", "--max_tracks", "32", "--track_min_score", "0.3"]
    paths = {}
    for name, extra in (("plain", []), ("motion", track + ["--track_motion", "--track_beta", "0.5"])):
        argv = base + extra + ["--output_directory", str(tmp_path / name)]
        source = R.SyntheticStream(C.flags("", argv, extra=R.stream_options))
        paths[name] = R.main(argv, model_factory=lambda a_, ds, dev: (a_, model), source=source)
    printed = capsys.readouterr().out
    with open(paths["plain"], "rb") as f, open(paths["motion"], "rb") as g:
        assert f.read() == g.read()                      # detections_<sequence>.npy is byte for byte what it was
    there = os.path.dirname(str(paths["motion"]))
    assert not os.path.exists(os.path.join(os.path.dirname(str(paths["plain"])), "coasting_mot.npy"))
    rec = np.load(paths["motion"])
    trk = np.load(os.path.join(there, "tracks_mot.npy"))
    coast = np.load(os.path.join(there, "coasting_mot.npy"))
    assert trk.dtype == np.dtype(R.MOTION_RECORD_DTYPE) and len(trk) == len(rec) > 0
    assert coast.dtype == np.dtype(R.COAST_RECORD_DTYPE)
    for name in rec.dtype.names:
        assert trk[name].tobytes() == rec[name].tobytes(), name
    assert int(trk["hits"].max()) >= 3 and np.all((trk["track_id"] == 0) == (trk["hits"] == 0))
    lone = trk["hits"] <= 1                              # no track, or a new one: at rest at the detection's own box
    assert not any(trk[n][lone].any() for n in ("vx1", "vy1", "vx2", "vy2"))
    # (alpha = 1: the filtered box is the detection's; the records hold it as centre-less x, y, w, h of the row)
    assert np.all(trk["tx2"] >= trk["tx1"]) and np.all(trk["ty2"] >= trk["ty1"])
    said = re.search(r"; (\d+) coasted track-steps -> \S*coasting_mot\.npy", printed)
    assert said and int(said.group(1)) == len(coast), printed
    if len(coast):
        assert coast["lane"].max() == 0 and coast["step"].max() < 10 and np.all(coast["age_us"] > 0) and np.all(coast["id"] > 0)
        steps_t = np.unique(trk["t"])
        assert set(coast["t"].tolist()) <= set(range(int(steps_t.min()) - 10000, int(steps_t.max()) + 1))
        for t in np.unique(coast["t"]):                  # a coasting track is not one the step saw
            assert not set(coast["id"][coast["t"] == t].tolist()) & set(trk["track_id"][trk["t"] == t].tolist()), t
